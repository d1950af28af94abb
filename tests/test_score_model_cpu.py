"""CPU tests of the shaper scorer's host side: tests/score_model.py against what the reference's own headers recorded
(tests/golden/score_ref.npz, written by tests/golden/make_score_ref.py through score_probe.cpp), the decision margins of every
committed evaluation, score_design.cpp under the address and undefined-behaviour sanitizers as a program of its own against the
model, and the host entry points of the C ABI.

Tolerances: the segment table, the error rows and everything integer are exact.  Result members and scores are held to
score_model.D_REF, the largest deviation of the model (numpy FFT, host libm) from the recording (long-double transform) measured
when the fixture was made and stored in it; members that are differences of near-equal quantities (the two penalties, near 0)
are compared in absolute terms on their natural scale of 1 (score_model.deviation).  D_REF does not cover the masking thresholds:
they are single bins' powers, and in a bin that holds only leakage two transforms differ by more (2.5e-13 in C16).  They are
held to the device's bar, GPU_BAR, with the bins at the threshold in quiet bit-equal, and to the measured score_model.D_THR."""
import os
import subprocess
import sys

import numpy as np
import pytest

import score_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_score_ref import RUNS, candidates, make_audio  # noqa: E402


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "score_ref.npz"))


@pytest.fixture(scope="module")
def learners():
    """per run: tables and the model's learner (segments, levelled rows, thresholds), built once"""
    out = {}
    for name, (which, rate, bits, n_cand) in RUNS.items():
        t = M.Tables(rate)
        audio = make_audio(which)
        out[name] = (t, M.Learner(audio[0], audio[1], t), bits, n_cand)
    return out


@pytest.fixture(scope="module")
def scored(learners):
    """the model's fresh-mode run of every recorded candidate, once"""
    cands = candidates()
    return {name: M.score(lr, cands[:n_cand], t, bits) for name, (t, lr, bits, n_cand) in learners.items()}


def test_fixture_is_what_the_script_makes(fx):
    assert np.array_equal(fx["candidates"], candidates()) and float(fx["margin"]) == 1.0e-9
    assert 0.0 < float(fx["d_ref"]) <= M.D_REF and M.GPU_BAR == max(8.0 * M.D_REF, 2049.0 * 2.0 ** -52)
    assert os.path.getsize(os.path.join(HERE, "golden", "score_ref.npz")) < 300 * 1024
    assert [len(fx["table_" + n]) for n in RUNS] == [16, 4, 8]
    assert fx["scores_fresh_A16"][3] == 1e18 and list(fx["ran_A16"]) == [c for c in range(18) if c != 3]


@pytest.mark.parametrize("name", list(RUNS))
def test_segment_table_and_thresholds(fx, learners, name):
    t, lr, _, _ = learners[name]
    table = fx["table_" + name]
    assert [(s[0], s[1], s[3], s[2]) for s in lr.segs] == [(int(a), int(b), float(c), int(d)) for a, b, c, d in table]     # exact
    assert lr.counts == [len(table) // 4] * 4
    for k, s in enumerate((0, len(table) - 1)):
        floor_equal, dev = M.threshold_deviation(lr.thr[s], fx["thr_" + name][k], t)
        print(name, "segment", s, "thresholds, model against the recording:", dev)
        assert floor_equal and dev <= M.D_THR[name] <= M.GPU_BAR        # D_REF does not cover these: score_model.threshold_deviation
    if name == "A16":
        assert sorted(set(table[:, 0])) == [0.0, 2048.0, 6144.0, 8192.0]        # the window at 4096 is gated out
        assert set(table[:, 3]) == {0.0, 2.0} and (table[table[:, 0] == 6144.0, 3] == 2.0).all()       # the transient
        x = make_audio("A")
        peak = np.abs(x[:, 6144:6144 + 4096]).max()
        assert table[(table[:, 0] == 6144.0) & (table[:, 1] == 3.0), 2][0] == 0.95 / peak          # the peak-headroom cap
    if name == "C16":
        assert set(table[:, 3]) == {1.0}


def test_error_rows_bit_for_bit(fx, learners, scored):
    _, lr, bits, _ = learners["A16"]
    assert np.array_equal(scored["A16"][2][0, 0], fx["rows_A16"][0])
    peak = []
    rows, coef, rng, keys = M.chain_inputs(lr, dict(enumerate(candidates()[:3])), M.CHAINED)      # two candidates ran before it
    i = keys.index((2, 5, 0))
    err = M.lattice_errors(rows[i:i + 2], coef[i:i + 2], rng[i:i + 2], bits, peak=peak)
    assert np.array_equal(err, fx["rows_A16"][1])
    assert np.array_equal(coef[i], [0.85] * 9) and not np.array_equal(err, scored["A16"][2][2, 5])      # the other generator mode


def test_lattice_stage_is_lattice_model(learners):
    """all 4096 samples of every chain of the candidate at the +-0.85 clamp: the states run into the +-2 limit on the way"""
    _, lr, bits, _ = learners["B24"]
    rows, coef, rng, keys = M.chain_inputs(lr, {2: candidates()[2]}, M.FRESH)
    assert len(keys) == 8 and np.array_equal(coef[0], [0.85] * 9)
    peak = []
    got = M.lattice_errors(rows, coef, rng, bits, peak=peak)
    assert peak[0] == 2.0
    assert np.array_equal(got, M.lattice_model_errors(rows, coef, rng, bits))


@pytest.mark.parametrize("name", list(RUNS))
def test_members_scores_and_margins(fx, learners, scored, name):
    t, lr, bits, n_cand = learners[name]
    scores, results, _ = scored[name]
    ran = list(fx["ran_" + name])
    worst = 0.0
    for ci, c in enumerate(ran):
        for s in range(len(lr.segs)):
            res = results[c, s]
            assert res.margin > float(fx["margin"]), (c, s, res.margin)         # no committed evaluation sits on a decision
            assert res.caps["tonal"] < 128 and res.caps["maskers"] < 128 and res.caps["min_energy"] > 1e-20
            worst = max(worst, float(M.deviation(res.array(), fx["results_" + name][ci, s]).max()))
    want = fx["scores_fresh_" + name]
    worst = max(worst, float(np.abs(scores / want - 1.0).max()))
    print(name, "model against the recording:", worst)
    assert worst <= M.D_REF
    assert [c for c in range(n_cand) if scores[c] == M.UNSTABLE] == [c for c in range(n_cand) if c not in ran]


def test_chained_scores(fx, learners):
    t, lr, bits, _ = learners["C16"]
    scores, _, _ = M.score(lr, candidates()[:3], t, bits, mode=M.CHAINED)
    want = fx["scores_chained_C16"]
    assert np.abs(scores / want - 1.0).max() <= M.D_REF
    assert scores[0] == pytest.approx(fx["scores_fresh_C16"][0], rel=1e-12) and not np.array_equal(want[1:], fx["scores_fresh_C16"][1:])


def test_score_design_under_sanitizers(learners, tmp_path):
    """score_design.cpp == the model: tables at three rates, selections, generator table; a stand-alone program"""
    hexes = lambda a: " ".join(f"{v:x}" for v in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).reshape(-1).tolist())
    ints = lambda a: " ".join(str(int(v)) for v in a)
    dump = tmp_path / "score.txt"
    with open(dump, "w") as f:
        for rate in (44100.0, 48000.0, 96000.0):
            t = M.Tables(rate)
            f.write(f"tables {rate!r} {t.flat_start} {t.flat_end} {t.high_start} {t.ultra_start}\n")
            for a in (t.weight, t.bark, t.ath_db, t.width, [t.ultra_share, t.flat_weight, t.hf_weight, t.weight_sum]):
                f.write(hexes(a) + "\n")
            f.write(ints(t.band) + "\n" + ints(t.range) + "\n")
        audios = [make_audio(w) for w in "ABC"]
        audios.append(audios[0][:, :4095])                          # n < 4096
        audios.append(audios[0][:, 2 * 2048:4 * 2048] * 1.0)        # all quiet
        for x in audios:
            segs, counts = M.select_segments(x[0], x[1])
            f.write(f"audio {x.shape[1]} {len(segs)} {ints(counts)}\n{hexes(x[0])}\n{hexes(x[1])}\n")
            for s in segs:
                f.write(f"{s[0]} {s[1]} {s[2]} {hexes([s[3]])}\n")
        table = M.rng_table(5)
        f.write(f"rng 5\n{' '.join(f'{int(v):x}' for v in table.reshape(-1))}\n")
    exe = tmp_path / "score_design_check"
    csrc = os.path.join(ROOT, "convopeq_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "sanitize", "score_design_check.cpp"), os.path.join(csrc, "score_design.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "3 tables, 5 audio, 1 rng, 0 failed checks" in r.stdout and "FAILED" not in r.stdout


def test_host_entry_points(amd, learners):
    t, lr, _, _ = learners["A16"]
    d = amd.score_design(48000.0)
    assert np.array_equal(d["weight"], t.weight) and np.array_equal(d["bark"], t.bark) and np.array_equal(d["band"], t.band)
    assert list(d["bins"]) == [t.flat_start, t.flat_end, t.high_start, t.ultra_start] and d["scalars"][3] == t.weight_sum
    x = make_audio("A")
    segs, counts = amd.select_segments(x[0], x[1])
    assert segs == lr.segs and counts == lr.counts
    assert amd.select_segments(x[0, :100], x[1, :100]) == ([], [0, 0, 0, 0])
