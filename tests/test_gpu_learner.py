"""cpq_learner on the device, through the C ABI: a generation's ask against the model (tests/learn_model.py) and the host entry
(cpq_learn_ask_host), its scores against cpq_scorer_score, its tell against cpq_learn_tell_host, and the properties of a run:
split runs, neighbours, parameter changes, inactive learners, the state round trip and the way to the dither stage.

Bit for bit everywhere but through the two library calls the sides do not share.  The ROCm tree documents no error figures for
its device math library, so the device side is taken at OpenCL full profile's maximum errors: log 3 ulp, tanh 5 ulp.  glibc
documents log 1 ulp and tanh 2 ulp on x86-64.
  z       = v * sqrt((-2 log s) / s).  A log within e ulp leaves (-2 log s) within e ulp (the product by 2 is exact), the quotient
            adds 1/2, the root halves what it is given and adds 1/2, the product by v adds 1/2: z is within (e + 1/2) / 2 + 1
            ulp of the exact value, below (e + 1) / 2 + 1.  Device e = 3: 3 ulp; host e = 1: 2 ulp; the two sides differ by at
            most their sum, 5 ulp, and an ulp is at most 2^-52 |z|:      Z_BAR = 5 * 2^-52 relative.
  mapped  = clampCoeff(tanh(candidate)) of the same candidate bits; the clamp moves no two values apart:
                                                                       MAP_BAR = (5 + 2) * 2^-52 relative.
Audio: make_score_ref.make_audio, B (4 segments: one window, every level) and A (16)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import learn_model as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_score_ref import make_audio  # noqa: E402

DBL_MAX = np.finfo(np.float64).max
Z_BAR = 5.0 * 2.0 ** -52
MAP_BAR = 7.0 * 2.0 ** -52
DEFAULT = [-0.003796, -0.006752, 0.008418, -0.010546, 0.004716, -0.007624, -0.020750, -0.002049, -0.003632]
STRONG = [0.82, -0.68, 0.55, -0.43, 0.33, -0.25, 0.18, -0.12, 0.07]
STD = (0.03, 0.30, 0.92, 0.0)


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


@pytest.fixture(scope="module")
def L():
    from convopeq_amd import learner
    return learner


@pytest.fixture(scope="module")
def audio():
    return {w: make_audio(w) for w in "AB"}


def make(amd, audio, n, which="B", silent=(), bits=16, **kw):
    """a scorer of n learners, all but `silent` holding audio `which`, and its learner"""
    sc = amd.ShaperScorer(n, 18, 48000.0, bits, **kw)
    for i in range(n):
        if i not in silent:
            assert sc.buildTrainingSegments(i, *audio[which]) == {"A": 16, "B": 4}[which]
    return sc, amd.ShaperLearner(sc)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def same_state(a, b, skip=()):
    for k in a:
        if k in skip:
            continue
        ok = np.array_equal(a[k], b[k]) if k == "rng" else (same(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k])
        if not ok:
            return k
    return None


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.abs(a - b)
    return np.where(d == 0.0, 0.0, d / np.maximum(np.minimum(np.abs(a), np.abs(b)), 1e-300))


def after_ask(before, after):
    """the state between ask and tell: only the generator and its counter have moved"""
    mid = dict(before)
    mid["rng"], mid["rejected_pairs"] = after["rng"], after["rejected_pairs"]
    return mid


@pytest.mark.parametrize("n", [1, 3])
def test_ask(amd, L, audio, n):
    sc, ln = make(amd, audio, n)
    ln.init(STRONG, 41)
    for i in range(n):
        before = ln.get_state(i)
        assert [int(w) for w in before["rng"]] == M.seed(41 + i)
    befores = [ln.get_state(i) for i in range(n)]
    ln.run(1)
    worst_z = worst_m = 0.0
    for i in range(n):
        gen, after = ln.read_generation(i), ln.get_state(i)
        rng = [int(w) for w in befores[i]["rng"]]
        want_z, _, rejected, _ = M.normals(rng)
        assert [int(w) for w in after["rng"]] == rng and after["rejected_pairs"] == rejected
        worst_z = max(worst_z, rel(gen["z"].ravel(), want_z).max())
        assert same(gen["candidates"], L.ask_host(befores[i], gen["z"])), i
        worst_m = max(worst_m, rel(gen["mapped"], M.map_candidates(gen["candidates"].tolist())).max())
    print(f"ask, {n} learners: z deviates by {worst_z / 2.0 ** -52:.2f} x 2^-52 relative, mapped by {worst_m / 2.0 ** -52:.2f} x 2^-52")
    assert worst_z <= Z_BAR and worst_m <= MAP_BAR


def test_ask_on_a_covariance_at_the_cholesky_floors(amd, L, audio):
    """diagonal entries at 0, below 0 and at 1e-20, loaded through set_state: both of computeCholesky's 1e-9 floors on the device"""
    sc, ln = make(amd, audio, 1)
    ln.init(DEFAULT, 6)
    a = np.array([[((3 * r + 5 * c + r * c) % 7 - 3) / 8.0 for c in range(9)] for r in range(9)])
    m = a @ a.T / 4.0 + 0.5 * np.eye(9)
    m[2, 2], m[5, 5], m[7, 7] = 0.0, -1.0, 1.0e-20
    st = ln.get_state(0)
    st["cov_upper"] = np.array([m[r, c] for r in range(9) for c in range(r, 9)])
    ln.set_state(0, st)
    ln.run(1)
    gen = ln.read_generation(0)
    assert same(gen["candidates"], L.ask_host(st, gen["z"])) and same(gen["candidates"], M.ask(st, gen["z"].tolist()))
    assert np.abs(gen["mapped"]).max() == 0.85                   # and candidates far enough out to sit on the safety margin


def test_scores_are_the_scorers(amd, audio):
    sc, ln = make(amd, audio, 2, "A")
    ln.init(DEFAULT, 5)
    ln.run(1)
    gens = [ln.read_generation(i) for i in range(2)]
    err = sc.read_error(1, 17, 15)                              # the last generation's rows
    want = sc.score(np.stack([g["mapped"] for g in gens]))
    for i in range(2):
        assert same(gens[i]["scores"], want[i]), i
    assert same(err, sc.read_error(1, 17, 15)) and np.isfinite(err).all() and np.abs(err).max() > 0.0


def test_tell_five_generations(amd, L, audio):
    sc, ln = make(amd, audio, 1)
    ln.init(DEFAULT, 77)
    p = L.make_params(*STD)
    minima = []
    for g in range(5):
        before = ln.get_state(0)
        ln.run(1)
        gen, after = ln.read_generation(0), ln.get_state(0)
        want, order = L.tell_host(after_ask(before, after), p, gen["candidates"], gen["scores"], gen["mapped"])
        assert same_state(want, after) is None, (g, same_state(want, after))
        assert list(gen["order"]) == list(order)
        minima.append(gen["scores"].min())
        assert same(ln.history(0), [minima[-1]])
        assert after["best_score"] == min(minima) and after["generations"] == g + 1
        best = int(np.argmin(gen["scores"]))
        if minima[-1] == min(minima) and minima.count(minima[-1]) == 1:
            assert same(after["best_scored"], gen["mapped"][best]) and same(after["best_raw"], gen["candidates"][best])
    assert same(ln.published(0), [math.tanh(M.sanitize(math.tanh(v))) for v in after["best_raw"]])         # the host's libm on both sides


def test_run_of_five_is_five_runs_of_one(amd, audio):
    sa, la = make(amd, audio, 1)
    sb, lb = make(amd, audio, 1)
    la.init(STRONG, 9)
    lb.init(STRONG, 9)
    la.run(5)
    minima = []
    for _ in range(5):
        lb.run(1)
        minima.append(lb.history(0)[0])
    a, b = la.get_state(0), lb.get_state(0)
    assert same_state(a, b) is None and a["generations"] == 5
    assert same(la.history(0), minima) and a["best_score"] == min(minima)
    ga, gb = la.read_generation(0), lb.read_generation(0)
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k


def test_a_learner_does_not_see_its_neighbours(amd, audio):
    results = []
    for n, at in ((1, 0), (3, 1), (65, 64)):
        sc, ln = make(amd, audio, n)
        ln.init(DEFAULT, 1000)
        ln.init(STRONG, 123 - at, learner=at)                   # init seeds learner i from seed + i
        ln.run(2)
        results.append((ln.get_state(at), ln.read_generation(at), ln.history(at)))
        ln.close()
        sc.close()
    for st, gen, hist in results[1:]:
        assert same_state(results[0][0], st) is None
        assert same(results[0][2], hist)
        for k in gen:
            assert np.array_equal(results[0][1][k], gen[k]), k


def test_set_params_acts_on_the_next_run(amd, L, audio):
    weights = (0.5, 0.3, 0.1, 0.1)
    sc, ln = make(amd, audio, 1)
    other = amd.ShaperScorer(1, 18, 48000.0, 16, level_weights=weights)
    other.buildTrainingSegments(0, *audio["B"])
    ln.init(DEFAULT, 3)
    ln.run(1)
    assert ln.get_state(0)["cov_retention"] == 0.92
    p = L.make_params(0.03, 0.30, 0.95, 0.01, weights)
    ln.set_params(p)
    before = ln.get_state(0)
    ln.run(1)
    gen, after = ln.read_generation(0), ln.get_state(0)
    assert after["cov_retention"] == min(0.95, 0.92 + 0.01)
    assert same(gen["scores"], other.score(gen["mapped"][None])[0])
    assert not same(gen["scores"], sc.score(gen["mapped"][None])[0])
    want, _ = L.tell_host(after_ask(before, after), p, gen["candidates"], gen["scores"], gen["mapped"])
    assert same_state(want, after) is None


def test_a_learner_without_audio_is_left_alone(amd, audio):
    sc, ln = make(amd, audio, 3, silent=(1,))
    lone_sc, lone = make(amd, audio, 1)
    ln.init(DEFAULT, 50)
    lone.init(DEFAULT, 50)
    idle = ln.get_state(1)
    ln.run(2)
    lone.run(2)
    assert same_state(idle, ln.get_state(1)) is None and ln.get_state(1)["generations"] == 0
    assert ln.history(1).size == 0
    with pytest.raises(amd.CpqError) as e:
        ln.read_generation(1)
    assert e.value.status == amd._capi.CPQ_ERR_NOT_READY
    assert same_state(lone.get_state(0), ln.get_state(0)) is None
    assert ln.get_state(2)["generations"] == 2 and same(lone.history(0), ln.history(0))


def test_state_round_trip(amd, audio):
    sa, la = make(amd, audio, 1)
    la.init(STRONG, 8)
    la.run(2)
    st = la.get_state(0)
    sb, lb = make(amd, audio, 2)
    lb.init(DEFAULT, 1)
    lb.set_state(1, st)
    assert same_state(st, lb.get_state(1)) is None
    la.run(2)
    lb.run(2)
    assert same_state(la.get_state(0), lb.get_state(1)) is None and same(la.history(0), lb.history(1))
    bad = dict(st)
    bad["rng"] = np.zeros(4, dtype=np.uint64)
    with pytest.raises(amd.CpqError):
        lb.set_state(0, bad)
    bad = dict(st)
    bad["sigma"] = float("nan")
    with pytest.raises(amd.CpqError):
        lb.set_state(0, bad)


def test_best_scored_reaches_the_dither_stage_unchanged(amd, audio):
    sc, ln = make(amd, audio, 1)
    ln.init(STRONG, 21)
    ln.run(2)
    best = ln.get_state(0)["best_scored"]
    assert np.abs(best).max() <= 0.85 and np.abs(best).max() > 0.0
    eng = amd.BatchedEngine(1, block_size=64, max_ir_len=1024, max_blocks_per_call=4, sample_rate=48000.0, call_mode=amd.CPQ_CALLS_ANY)
    eng.set_dither(amd.CPQ_DITHER_ADAPTIVE9, 16)
    eng.dither_set_adaptive_coeffs(0, best)
    assert same(eng.dither_get_adaptive_coeffs(0), best)
    eng.close()


def test_multi_start_keeps_the_best_state(amd, audio):
    sc, ln = make(amd, audio, 1)
    ln.init(DEFAULT, 4)
    scores = ln.multi_start(seeds=(11, 12), generations=2)
    st = ln.get_state(0)
    assert scores[0] < DBL_MAX and st["generations"] in (1, 2) and st["best_score"] <= scores[0]


def test_creation_refusals(amd, audio):
    K = amd._capi
    lib, h = K.load(), C.c_void_p(1)
    sc = amd.ShaperScorer(1, 18, 48000.0, 16)
    assert lib.cpq_learner_create(None, C.byref(h)) == K.CPQ_ERR_INVALID_ARG and not h.value
    assert lib.cpq_learner_create(sc._h, None) == K.CPQ_ERR_INVALID_ARG
    for kw in (dict(max_candidates=17), dict(rng_mode=K.CPQ_SCORE_RNG_CHAINED)):
        bad = amd.ShaperScorer(**dict(dict(n_learners=1, max_candidates=18, sample_rate_hz=48000.0, bit_depth=16), **kw))
        h = C.c_void_p(1)
        assert lib.cpq_learner_create(bad._h, C.byref(h)) == K.CPQ_ERR_INVALID_ARG and not h.value
        assert lib.cpq_last_error(None) != b""
    ln = amd.ShaperLearner(sc)
    assert lib.cpq_learner_run(ln._h, 0) == K.CPQ_ERR_INVALID_ARG and lib.cpq_learner_run(ln._h, 4097) == K.CPQ_ERR_INVALID_ARG
    sc.buildTrainingSegments(0, *audio["B"])
    assert lib.cpq_learner_run(ln._h, 1) == K.CPQ_ERR_NOT_READY            # never initialised
    assert lib.cpq_learner_get_state(ln._h, 1, C.byref(K.LearnState())) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_learner_last_error(ln._h) != b""
