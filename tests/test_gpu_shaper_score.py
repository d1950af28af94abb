"""The shaper scorer on the device, through the C ABI (cpq_scorer_*), against what the reference's own headers recorded
(tests/golden/score_ref.npz) and against tests/score_model.py, which the CPU tests hold to that recording and to
tests/lattice_model.py.

The lattice stage and everything integer are exact.  Floating results are held to score_model.GPU_BAR =
max(8 d_ref, 2049 * 2^-52) relative: d_ref is the model's own deviation from the recording (numpy FFT and host libm against the
long-double transform), the factor 8 covers a second libm and tree-ordered sums, the floor is the first-order bound for
reordering a sum of 2049 non-negative terms.  The two penalties are differences of near-equal quantities near 0 and are compared
in absolute terms on their natural scale of 1 (score_model.deviation); masking thresholds are held to the same bar, relative per
bin, and are the same bits where the threshold in quiet decides (score_model.threshold_deviation).  No evaluation is excused: the fixture holds none within 1e-9 of a decision threshold.

buildTrainingSegments gives every level the same windows until its bucket is full, so a learner holds 4 m segments, m per level:
the cases are 4 (one window), 8 and 16 segments -- 24, 48 and 96 chains with three candidates: below one workgroup's 64 lanes, no
multiple of them, and more than one workgroup."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import score_model as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_score_ref import candidates, make_audio  # noqa: E402

DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "score_ref.npz"))


@pytest.fixture(scope="module")
def audio():
    return {w: make_audio(w) for w in "ABC"}


@pytest.fixture(scope="module")
def model(audio):
    """tables and the model's learners, built once: (audio, rate) -> (tables, learner)"""
    out = {}
    for which, rate in (("A", 48000.0), ("B", 48000.0), ("C", 44100.0), ("C", 48000.0)):
        t = M.Tables(rate)
        out[which, rate] = (t, M.Learner(audio[which][0], audio[which][1], t))
    return out


def check_parts(parts, want, what):
    dev = M.deviation(parts, want)
    print(what, "parts deviation", float(dev.max()))
    assert dev.max() <= M.GPU_BAR, (what, np.unravel_index(np.argmax(dev), dev.shape), dev.max())


def check_scores(got, want, what):
    dev = np.abs(got / want - 1.0)
    print(what, "score deviation", float(dev.max()))
    assert dev.max() <= M.GPU_BAR, (what, dev)


@pytest.mark.parametrize("which,bits,mode", [("A", 16, M.FRESH), ("A", 16, M.CHAINED), ("C", 24, M.FRESH), ("C", 24, M.CHAINED), ("B", 16, M.CHAINED),
                                             ("B", 24, M.FRESH)])
def test_lattice_stage_bit_for_bit(amd, fx, audio, model, which, bits, mode):
    """every chain's error rows == the model's, and == tests/lattice_model.py's over all 4096 samples: every chain of the smallest
    case (B at 24 bits, 24 chains), elsewhere the chains of the candidate at the clamp on the first and the last segment
    (lattice_model's exact fused terms cost 0.2 s a chain); the recorded rows where the case has them.  Candidate 1 is the set at
    the +-0.85 clamp (0.99 ... 0.87 as given), whose states run into the +-2 limit at both bit depths."""
    t, lr = model[which, 48000.0]
    cands = candidates()[[0, 2, 5]]
    sc = amd.ShaperScorer(1, 3, 48000.0, bits, rng_mode=mode)
    n_seg = {"A": 16, "B": 4, "C": 8}[which]
    assert sc.buildTrainingSegments(0, *audio[which]) == len(lr.segs) == n_seg
    sc.score(cands[None])
    rows, coef, rng, keys = M.chain_inputs(lr, dict(enumerate(cands)), mode)
    assert len(keys) % 64 != 0
    peak = []
    want = M.lattice_errors(rows, coef, rng, bits, peak=peak)
    assert peak[0] == 2.0
    got = np.concatenate([sc.read_error(0, c, s) for c, s, _ in keys[::2]])
    for i in range(0, len(keys), 2):
        assert np.array_equal(got[i:i + 2], want[i:i + 2]), keys[i]
    every = (which, bits) == ("B", 24)
    through = [i for i, (c, s, _) in enumerate(keys) if every or (c == 1 and s in (0, n_seg - 1))]
    assert len(through) == (24 if every else 4)
    assert np.array_equal(got[through], M.lattice_model_errors(rows[through], coef[through], rng[through], bits))
    if which == "A" and bits == 16 and mode == M.FRESH:
        assert np.array_equal(sc.read_error(0, 0, 0), fx["rows_A16"][0])       # the recording itself
    sc.close()


def test_recorded_chained_rows(amd, fx, audio):
    """the recorded chained rows are candidate 2, segment 5: the generator index counts the candidates run before it"""
    sc = amd.ShaperScorer(1, 18, 48000.0, 16, rng_mode=M.CHAINED)
    sc.buildTrainingSegments(0, *audio["A"])
    sc.score(candidates()[None, :3])
    assert np.array_equal(sc.read_error(0, 2, 5), fx["rows_A16"][1])
    sc.close()


def test_scores_against_the_fixture_three_learners(amd, fx, audio, model):
    """3 learners with different audio (A, B, C: 16, 4 and 8 segments) and a fourth that holds none, 18 candidates, both generator
    modes.  Learner 0 against the recording; learners 1 and 2, which have no recording at 16 bits and 48 kHz, against the model
    (the CPU tests hold it to the recording within D_REF): the first three candidates, members and scores, in both modes."""
    cands = candidates()
    k = np.broadcast_to(cands, (4, 18, 9)).copy()
    ran = list(fx["ran_A16"])
    t, lb = model["B", 48000.0]
    _, lc = model["C", 48000.0]
    modes = (M.FRESH, M.CHAINED)
    want = M.score_batch([(lr, cands[:3], mode) for mode in modes for lr in (lb, lc)], t, 16)
    for mi, mode in enumerate(modes):
        sc = amd.ShaperScorer(4, 18, 48000.0, 16, rng_mode=mode)
        assert [sc.buildTrainingSegments(l, *audio[w]) for l, w in enumerate("ABC")] == [16, 4, 8]
        scores, parts = sc.score(k, parts=True)
        sc.close()
        check_scores(scores[0], fx["scores_fresh_A16" if mode == M.FRESH else "scores_chained_A16"], f"A16 mode {mode}")
        assert (scores[:, 3] == 1e18).all()                                     # exactly, and nothing ran; refused before DBL_MAX
        assert (parts[:, 3] == 0.0).all() and (parts[3] == 0.0).all() and (parts[1, :, 4:] == 0.0).all() and (parts[2, :, 8:] == 0.0).all()
        assert (scores[3, ran] == DBL_MAX).all()                                # no segments, while the others score normally
        if mode == M.FRESH:
            check_parts(parts[0][ran], fx["results_A16"], "A16")
        for l, n_seg, name in ((1, 4, "B"), (2, 8, "C")):
            w_scores, results, _ = want[2 * mi + l - 1]
            check_scores(scores[l, :3], w_scores, f"{name} at 16 bits, mode {mode}")
            check_parts(parts[l, :3, :n_seg], np.array([[results[c, s].array() for s in range(n_seg)] for c in range(3)]),
                        f"{name} at 16 bits, mode {mode}")


@pytest.mark.parametrize("name,which,rate,bits", [("B24", "B", 48000.0, 24), ("C16", "C", 44100.0, 16)])
def test_scores_against_the_fixture_one_learner(amd, fx, audio, name, which, rate, bits):
    """1 learner, 3 candidates and 1 candidate; 24 bits; 44100 Hz (other tables)"""
    cands = candidates()[:3]
    for mode in (M.FRESH, M.CHAINED):
        sc = amd.ShaperScorer(1, 3, rate, bits, rng_mode=mode)
        n = sc.buildTrainingSegments(0, *audio[which])
        scores, parts = sc.score(cands[None], parts=True)
        want = fx["scores_fresh_" + name if mode == M.FRESH else "scores_chained_" + name]
        check_scores(scores[0], want, f"{name} mode {mode}")
        if mode == M.FRESH:
            check_parts(parts[0, :, :n], fx["results_" + name], name)
        one = sc.score(cands[None, :1])
        assert one.shape == (1, 1) and one[0, 0] == scores[0, 0]                # candidate 0 starts both modes from rng_start
        sc.close()
    d = amd.score_design(44100.0)
    t = M.Tables(44100.0)
    assert np.array_equal(d["weight"], t.weight) and list(d["bins"]) == [t.flat_start, t.flat_end, t.high_start, t.ultra_start]


def test_special_values_and_the_stability_switch(amd, audio):
    cands = candidates()[:6].copy()
    on = amd.ShaperScorer(1, 6, 48000.0, 16)
    off = amd.ShaperScorer(1, 6, 48000.0, 16, stability_check=False)
    for sc in (on, off):
        sc.buildTrainingSegments(0, *audio["C"])
    a, b = on.score(cands[None])[0], off.score(cands[None])[0]
    assert a[3] == 1e18 and b[3] != 1e18 and np.isfinite(b[3])
    assert np.array_equal(np.delete(a, 3), np.delete(b, 3))                     # the neighbours are unaffected
    clamped = cands.copy()
    clamped[3] = M.clamp_coeffs(cands[3])                                       # 1.0 -> 0.85: what setCoefficients runs
    assert on.score(clamped[None])[0, 3] == b[3]
    on.score(cands[None])
    with pytest.raises(amd.CpqError):
        on.read_error(0, 3, 0)                                                  # a refused candidate leaves no rows
    # evaluateCandidate: tanh, then the margin, on the host
    raw = np.arctanh(np.clip(cands, -0.8, 0.8))
    mapped = np.array([[M.clamp_coeffs([math.tanh(v)])[0] for v in row] for row in raw])
    assert np.array_equal(on.score_raw(raw[None]), on.score(mapped[None]))
    on.close()
    off.close()


def test_repeatable_independent_and_bounded_output(amd, audio):
    cands = candidates()[[0, 1, 2, 4, 5]]
    solo = amd.ShaperScorer(1, 5, 48000.0, 16)
    trio = amd.ShaperScorer(3, 5, 48000.0, 16)
    solo.buildTrainingSegments(0, *audio["C"])
    trio.buildTrainingSegments(1, *audio["C"])
    trio.buildTrainingSegments(0, *audio["B"])
    s1, p1 = solo.score(cands[None], parts=True)
    s2, p2 = solo.score(cands[None], parts=True)
    assert s1.tobytes() == s2.tobytes() and p1.tobytes() == p2.tobytes()       # nothing is carried from call to call
    k3 = np.stack([cands[::-1], cands, cands])
    t1, q1 = trio.score(k3, parts=True)
    assert t1[1].tobytes() == s1[0].tobytes() and q1[1].tobytes() == p1[0].tobytes()    # whatever the other learners hold
    assert (t1[2] == DBL_MAX).all()
    trio.buildTrainingSegments(0, *audio["A"])                                  # replacing one learner's audio changes only it
    t2 = trio.score(k3)
    assert t2[1].tobytes() == t1[1].tobytes() and not np.array_equal(t2[0], t1[0])
    trio.buildTrainingSegments(0, audio["A"][0, :100], audio["A"][1, :100])     # fewer than 4096 samples: 0 segments, no error
    assert (trio.score(k3)[0] == DBL_MAX).all()
    # n_candidates < max_candidates: the call writes [n_learners][n_candidates] scores and parts and nothing behind them
    from convopeq_amd import _capi as K
    scores, parts = np.full(5 + 3, -7.0), np.full((5 + 1) * 16 * 5, -7.0)
    k2 = np.ascontiguousarray(cands[:2])
    rc = solo._lib.cpq_scorer_score(solo._h, k2.ctypes.data_as(K.c_double_p), 2, scores.ctypes.data_as(K.c_double_p),
                                    parts.ctypes.data_as(C.POINTER(K.ScoreParts)))
    assert rc == 0 and (scores[2:] == -7.0).all() and (parts[2 * 16 * 5:] == -7.0).all()
    assert scores[:2].tobytes() == s1[0, :2].tobytes() and parts[:2 * 80].tobytes() == p1[0, :2].tobytes()
    assert solo._lib.cpq_scorer_score(solo._h, k2.ctypes.data_as(K.c_double_p), 6, scores.ctypes.data_as(K.c_double_p), None) == -1
    solo.close()
    trio.close()


def test_set_audio(amd, fx, audio, model):
    import torch
    sc = amd.ShaperScorer(2, 1, 48000.0, 16)
    assert sc.buildTrainingSegments(0, *audio["A"]) == 16
    segs, counts = sc.segments(0)
    table = fx["table_A16"]
    assert [(s[0], s[1], s[3], s[2]) for s in segs] == [(int(a), int(b), float(c), int(d)) for a, b, c, d in table] and counts == [4] * 4
    t, _ = model["A", 48000.0]
    for k, s in enumerate((0, 15)):             # relative, one bar; the same bits where the threshold in quiet is the threshold
        floor_equal, dev = M.threshold_deviation(sc.thresholds(0, s), fx["thr_A16"][k], t)
        print("A16 segment", s, "threshold deviation", dev)
        assert floor_equal and dev <= M.GPU_BAR, (s, dev)
    # the _device variant: the same bits from the same rows
    assert sc.set_audio_device(1, torch.from_numpy(audio["A"]).cuda().contiguous()) == 16
    assert sc.segments(1) == (segs, counts)
    for s in range(16):
        assert sc.thresholds(1, s).tobytes() == sc.thresholds(0, s).tobytes()
    # only the most recent 4096 + 2048 * 15 samples count, on either side
    recent = np.concatenate([np.zeros((2, M.RECENT - audio["A"].shape[1])), audio["A"]], axis=1)
    longer = np.concatenate([np.full((2, 5001), 0.3), recent], axis=1)
    assert sc.buildTrainingSegments(0, *recent) == 16
    assert sc.set_audio_device(1, torch.from_numpy(longer).cuda().contiguous()) == 16
    assert sc.segments(1) == sc.segments(0) and sc.segments(0)[1] == counts and sc.segments(0)[0] != segs      # the starts moved
    for s in (0, 15):
        assert sc.thresholds(1, s).tobytes() == sc.thresholds(0, s).tobytes()
    segs = sc.segments(0)[0]
    k = candidates()[None, :1].repeat(2, axis=0)
    scores = sc.score(k)
    assert scores[0, 0] == scores[1, 0]
    assert sc.buildTrainingSegments(1, *audio["B"]) == 4 and sc.segments(0) == (segs, counts)
    after = sc.score(k)
    assert after[0, 0] == scores[0, 0] and after[1, 0] != scores[1, 0]
    print("lattice / spectrum ms:", sc.last_timing())
    sc.close()
