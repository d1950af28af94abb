"""Records tests/golden/score_edges_ref.npz: the verdict of the reference's own MklFftEvaluator.h, through the evaluate-only mode
of score_probe.cpp, on the edge inputs of tests/score_edge_inputs.py (silence, single bins, band 0 consumed, dense combs, steps
over the 7 dB and the 6 localAvg tests, a dominating thr array).
    python tests/golden/make_score_edges_ref.py <reference source tree>
The probe is built into a temporary directory and is not kept.  The inputs are exact generators (score_edge_inputs.py), so the
file holds no rows: per case the five Result members and computeMaskingThreshold of every bin, and d_edge, the model's largest
deviation from the recorded members (score_model.deviation).  The script asserts that the probe read the rows the generators
make, and that every case stays further than 1e-9 from every data-dependent threshold (Result.margin); the caps are what some
cases are for and are reported, not refused.  It also runs the bounded search for an input with more than 128 masker candidates
(score_edge_inputs.cap_search) and prints what it reached."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
MARGIN = 1.0e-9
SEARCH_RATES = (44100.0, 48000.0, 88200.0, 96000.0, 176400.0, 192000.0, 384000.0)


def run_probe(exe, tmp, rate, names):
    import score_edge_inputs as E
    fin, fout, fecho = (os.path.join(tmp, f) for f in ("in.bin", "out.bin", "echo.bin"))
    parts = []
    for n in names:
        thr = E.thr(n)
        parts += [np.array([0.0 if thr is None else 1.0]), E.rows(n).ravel()] + ([] if thr is None else [thr])
    np.concatenate(parts).tofile(fin)
    subprocess.run([exe, "eval", repr(rate), fin, fout, fecho], check=True)
    out = np.fromfile(fout).reshape(len(names), 5 + 2049)
    echo = np.fromfile(fecho).reshape(len(names), 2, 4096)
    for i, n in enumerate(names):
        assert echo[i].tobytes() == E.rows(n).tobytes(), n                     # what is recorded is what the probe read
    return out[:, :5], out[:, 5:]


def main(ref):
    import score_edge_inputs as E
    import score_model as M
    out = {"margin": np.array(MARGIN)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "score_probe")
        subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-msse4.1", "-mavx2", "-mfma", "-I" + os.path.join(HERE, "score_shim"),
                        "-I" + os.path.join(HERE, "juce_shim"), "-I" + os.path.join(ref, "src"), os.path.join(HERE, "score_probe.cpp"), "-o", exe],
                       check=True)
        for rate in sorted({c[0] for c in E.CASES.values()}):
            names = E.cases(rate)
            members, thr = run_probe(exe, tmp, rate, names)
            t = M.Tables(rate)
            for i, n in enumerate(names):
                res = M.evaluate(E.rows(n), E.thr(n), t)
                assert res.margin > MARGIN, (n, res.margin)
                d = float(M.deviation(res.array(), members[i]).max())
                floor_equal, d_thr = M.threshold_deviation(M.masking_thresholds(E.rows(n), t), thr[i], t) if (thr[i] != t.ath_pow).any() else (True, 0.0)
                print(f"{n:14s} d_edge {d:.3e} d_thr {d_thr:.3e} floor {floor_equal} margin {res.margin:.2e} tonal {res.caps['tonal']:3d} bands {res.caps['bands']:2d} "
                      f"maskers {res.caps['maskers']:3d} softplus (x, log1p, exp) {res.branches}")
                out["members_" + n], out["thr_" + n], out["d_edge_" + n] = members[i], thr[i], np.array(d)
    assert list(E.THINNED_48K) == E.cap_search(48000.0)[1]
    for rate in SEARCH_RATES:
        n, peaks = E.cap_search(rate)
        print(f"cap search at {rate:g} Hz: {n} masker candidates ({len(peaks)} peaks)")
    path = os.path.join(HERE, "score_edges_ref.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
