"""Records tests/golden/score_ref.npz from the reference's own LatticeNoiseShaper.h and MklFftEvaluator.h through score_probe.cpp.
    python tests/golden/make_score_ref.py <reference source tree>
The probe binary is built into a temporary directory and is not kept.  The inputs are closed forms of integer counters and of
IEEE additions and multiplications only (no libm), so every machine makes the same samples: a parabolic "sine" per tone, the
project's counter noise through a one-pole low-pass, several levels, one stretch below the RMS gate, one transient.
A case is recorded only if every data-dependent comparison of every evaluation stays further than 1e-9 from its threshold
(tests/score_model.py reports the distance); the script stops otherwise."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_dither_ref import splitmix_noise  # noqa: E402

DEFAULT = [-0.003796, -0.006752, 0.008418, -0.010546, 0.004716, -0.007624, -0.020750, -0.002049, -0.003632]
STRONG = [0.82, -0.68, 0.55, -0.43, 0.33, -0.25, 0.18, -0.12, 0.07]
AT_CLAMP = [0.99, 0.97, 0.95, 0.93, 0.91, 0.9, 0.89, 0.88, 0.87]        # stable as given; setCoefficients clamps every one to 0.85
UNSTABLE = [0.2, -0.1, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
MARGIN = 1.0e-9
# name -> (audio, rate, bits, candidates recorded with their Result members)
RUNS = {"A16": ("A", 48000.0, 16, 18), "B24": ("B", 48000.0, 24, 3), "C16": ("C", 44100.0, 16, 3)}


def tone(n, period, phase=0):
    """a parabolic sine of `period` samples: 4 p (1 - p) arches of alternating sign, p in [0, 1) exact"""
    i = (np.arange(n, dtype=np.int64) * 2 + phase) % (2 * period)
    p = (i % period).astype(np.float64) / float(period)
    return np.where(i < period, 1.0, -1.0) * (4.0 * p * (1.0 - p))


def shaped_noise(n, stream, channel, pole):
    x = splitmix_noise(n, stream, channel)
    y = np.empty(n)
    acc = 0.0
    for i, v in enumerate(x.tolist()):
        acc = pole * acc + (1.0 - pole) * v
        y[i] = acc
    return 4.0 * y


def make_audio(which):
    """[2, n] rows of learner audio A (16 segments: a gated window, a transient), B (4 segments, broadband), C (8, tonal)"""
    if which == "A":
        n = 4096 + 2048 * 5
        level = np.repeat(np.array([0.5, 0.1, 1.0e-6, 1.0e-6, 1.0, 0.25, 0.5]), 2048)
        rows = []
        for ch in range(2):
            x = 0.2 * tone(n, 96, 7 * ch) + 0.05 * tone(n, 13, ch) + 0.3 * shaped_noise(n, 1, ch, 0.5 + 0.25 * ch)
            rows.append(x * level)
        x = np.stack(rows)
        x[0, 4 * 2048 + 300] += 0.9                     # the transient: its first window starts in the quiet stretch
        x[1, 4 * 2048 + 301] -= 0.8
        return x
    if which == "B":
        n = 4096 + 100
        return np.stack([splitmix_noise(n, 2, ch) + 0.02 * tone(n, 40, ch) for ch in range(2)])
    n = 4096 + 2048 + 7
    return np.stack([0.5 * tone(n, 24 + 8 * ch) + 0.001 * splitmix_noise(n, 3, ch) for ch in range(2)])


def candidates():
    """[18, 9] mapped sets: default, strong, at the clamp, unstable, then counter noise within +-0.3 times a decay"""
    out = [DEFAULT, STRONG, AT_CLAMP, UNSTABLE]
    u = splitmix_noise(14 * 9, 9, 0).reshape(14, 9) * 4.0          # +-1
    for c in range(14):
        out.append([float(0.3 * u[c, i] / (1.0 + 0.25 * i)) for i in range(9)])
    return np.array(out)


def run_probe(exe, tmp, audio, rate, bits, mode, cands):
    fin, fc, fout, frows = (os.path.join(tmp, f) for f in ("in.bin", "c.bin", "out.bin", "rows.bin"))
    audio.tofile(fin)
    np.ascontiguousarray(cands).tofile(fc)
    r = subprocess.run([exe, repr(rate), str(bits), str(mode), "1", fin, fc, str(len(cands)), fout, frows], check=True, capture_output=True, text=True)
    o = np.fromfile(fout)
    n_seg = int(o[0])
    table = o[1:1 + 4 * n_seg].reshape(n_seg, 4)
    at = 1 + 4 * n_seg
    thr = o[at:at + n_seg * 2049].reshape(n_seg, 2049)
    at += n_seg * 2049
    scores = o[at:at + len(cands)]
    results = o[at + len(cands):]
    ran = [c for c in range(len(cands)) if scores[c] != 1e18]
    results = results.reshape(len(ran), n_seg, 5)
    rows = np.fromfile(frows).reshape(len(ran), n_seg, 2, 4096)
    return {"table": table, "thr": thr, "scores": scores, "results": results, "rows": rows, "ran": ran, "log": r.stdout.strip()}


def main(ref):
    import score_model as M
    cands = candidates()
    out = {"candidates": cands, "margin": np.array(MARGIN)}
    worst = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "score_probe")
        subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-msse4.1", "-mavx2", "-mfma", "-I" + os.path.join(HERE, "score_shim"),
                        "-I" + os.path.join(HERE, "juce_shim"), "-I" + os.path.join(ref, "src"), os.path.join(HERE, "score_probe.cpp"), "-o", exe],
                       check=True)
        for name, (which, rate, bits, n_cand) in RUNS.items():
            audio = make_audio(which)
            fresh = run_probe(exe, tmp, audio, rate, bits, 0, cands[:n_cand])
            chained = run_probe(exe, tmp, audio, rate, bits, 1, cands[:n_cand])
            print(name, fresh["log"], "|", chained["log"])
            t = M.Tables(rate)
            # the recorded evaluations stay clear of every decision threshold, and the model agrees with them
            for ci, c in enumerate(fresh["ran"]):
                for s in range(len(fresh["table"])):
                    res = M.evaluate(fresh["rows"][ci, s], fresh["thr"][s], t)
                    assert res.margin > MARGIN, (name, c, s, res.margin)
                    assert res.caps["tonal"] < 128 and res.caps["maskers"] < 128 and res.caps["min_energy"] > 1.0e-20, (name, c, s, res.caps)
                    want = fresh["results"][ci, s]
                    dev = M.deviation(res.array(), want)
                    worst = max(worst, float(dev.max()))
            out["table_" + name] = fresh["table"]
            out["scores_fresh_" + name], out["scores_chained_" + name] = fresh["scores"], chained["scores"]
            out["ran_" + name] = np.array(fresh["ran"])
            out["results_" + name] = fresh["results"]
            out["thr_" + name] = fresh["thr"][[0, len(fresh["thr"]) - 1]]               # the first and the last segment
            if name == "A16":
                out["rows_A16"] = np.stack([fresh["rows"][0, 0], chained["rows"][2, 5]])   # (default, seg 0) fresh; (at clamp, seg 5) chained
    print("largest deviation of the model from the recorded members (d_ref):", worst)
    out["d_ref"] = np.array(worst)
    np.savez_compressed(os.path.join(HERE, "score_ref.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "score_ref.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
