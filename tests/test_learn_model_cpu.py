"""The optimiser of cpq_learner on the host (cpq_learn_*_host, csrc/learn_plan.hpp) and its plain-Python restatement
(tests/learn_model.py) against what the reference's own CmaEsOptimizer.h recorded (tests/golden/learn_ref.npz, written by
tests/golden/make_learn_ref.py through learn_probe.cpp): sample() and update() bit for bit over every recorded generation --
identity and loaded covariances, a climbing retention, DBL_MAX fitness, sigma on both clamps, covariance entries that sanitize
zeroes, a covariance on computeCholesky's floors.  The recorded fitness vectors hold no ties among their finite values.

What involves a logarithm is held to the logarithm's rounding: initFromParcor within 2 ulp (glibc documents log within 1 ulp on
x86-64 and the recording ran a libm too; the quotient before it and the halving after it are exact operations on both sides),
the normal variates against the model within 3 ulp (one log within 1 ulp on either side, halved by the root: (1 + 1) / 2 ulp,
plus a rounding each of the quotient, the root and the product that may then differ: stated, not measured)."""
import math
import os

import numpy as np
import pytest

import learn_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("default", "strong", "loaded", "dblmax", "clamp_lo", "clamp_hi", "tiny", "floors")
DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "learn_ref.npz"))


@pytest.fixture(scope="module")
def L():
    from convopeq_amd import learner
    return learner


def state_of(rec, retention, generations=0):
    return {"mean": rec[:9].copy(), "cov_upper": rec[9:54].copy(), "sigma": float(rec[54]), "cov_retention": float(retention),
            "rng": np.array([1, 2, 3, 4], dtype=np.uint64), "best_score": DBL_MAX, "best_raw": np.zeros(9), "best_scored": np.zeros(9),
            "generations": generations, "rejected_pairs": 0}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.minimum(np.abs(a), np.abs(b)))


def test_the_record_covers_what_it_is_for(fx):
    assert fx["default_z"].shape[0] >= 5 and fx["strong_z"].shape[0] >= 5
    assert np.count_nonzero(fx["loaded_before"][0, 9:54]) >= 40         # a dense covariance
    assert (fx["dblmax_fit"] == DBL_MAX).sum(axis=1).min() >= 1 and (fx["dblmax_fit"] < DBL_MAX).sum(axis=1).min() >= 6
    assert fx["clamp_lo_after"][0, 54] == fx["clamp_lo_params"][0, 0] and fx["clamp_hi_after"][0, 54] == fx["clamp_hi_params"][0, 1]
    assert np.any((fx["tiny_before"][0, 9:54] != 0.0) & (fx["tiny_after"][0, 9:54] == 0.0))
    assert len(set(fx["strong_ret"])) > 2
    for name in CASES:
        for f in fx[name + "_fit"]:
            finite = f[f < DBL_MAX]
            assert len(set(finite)) == len(finite), name


@pytest.mark.parametrize("name", CASES)
def test_ask_bit_for_bit(fx, L, name):
    for g in range(fx[name + "_z"].shape[0]):
        st = state_of(fx[name + "_before"][g], fx[name + "_ret"][g])
        want = fx[name + "_cand"][g]
        assert same(L.ask_host(st, fx[name + "_z"][g]), want), (name, g, "library")
        assert same(M.ask(st, fx[name + "_z"][g].tolist()), want), (name, g, "model")


@pytest.mark.parametrize("name", CASES)
def test_tell_bit_for_bit(fx, L, name):
    G = fx[name + "_z"].shape[0]
    running = None
    for g in range(G):
        smin, smax, target, step = fx[name + "_params"][g]
        st = state_of(fx[name + "_before"][g], fx[name + "_ret"][g], g)
        if running is not None:
            for k in ("best_score", "best_raw", "best_scored"):
                st[k] = running[k]
        cand, fit = fx[name + "_cand"][g], fx[name + "_fit"][g]
        mapped = np.array(M.map_candidates(cand.tolist()))
        got, order = L.tell_host(st, L.make_params(smin, smax, target, step), cand, fit, mapped)
        model, morder = M.tell(st, (smin, smax, target, step), cand.tolist(), fit.tolist(), mapped.tolist())
        want = fx[name + "_after"][g]
        for who, s in (("library", got), ("model", model)):
            assert same(s["mean"], want[:9]) and same(s["cov_upper"], want[9:54]) and same([s["sigma"]], want[54:]), (name, g, who)
            assert s["generations"] == g + 1
        ret = min(target, fx[name + "_ret"][g] + step)
        assert got["cov_retention"] == model["cov_retention"] == ret
        if g + 1 < G:
            assert ret == fx[name + "_ret"][g + 1]
        n_finite = int((fit < DBL_MAX).sum())
        assert list(order[:n_finite]) == morder[:n_finite] == sorted(range(18), key=lambda i: fit[i])[:n_finite]
        assert list(order) == morder                                    # ours: ties by index
        best = int(np.argmin(fit))
        assert got["best_score"] == model["best_score"] == min(fit.min(), st["best_score"])
        if fit.min() < st["best_score"]:
            assert same(got["best_raw"], cand[best]) and same(got["best_scored"], mapped[best])
        assert same(got["best_raw"], model["best_raw"]) and same(got["best_scored"], model["best_scored"])
        running = got


def test_ties_nan_and_few_finite_values(L):
    """the order the library fixes where std::sort leaves it open, and the best tracking on them"""
    st = L.init_host(np.zeros(9), 3)
    z, st, _ = L.normals_host(st)
    cand = L.ask_host(st, z)
    p = L.make_params()
    for fit in (np.full(18, 2.0), np.array([3.0, 1.0, 1.0, float("nan"), 0.5, 0.5] * 3), np.array([DBL_MAX] * 15 + [2.0, 1.0, float("nan")]),
                np.full(18, DBL_MAX), np.full(18, float("nan")), np.array([1e18] * 9 + [float("inf")] * 9)):
        got, order = L.tell_host(st, p, cand, fit, cand)
        model, morder = M.tell(st, (0.03, 0.30, 0.92, 0.0), cand.tolist(), fit.tolist(), cand.tolist())
        assert list(order) == morder, fit
        for k in ("mean", "cov_upper", "best_raw", "best_scored"):
            assert same(got[k], model[k]), (k, fit)
        assert got["sigma"] == model["sigma"] and got["best_score"] == model["best_score"]
    got, _ = L.tell_host(st, p, cand, np.full(18, DBL_MAX), cand)
    assert got["best_score"] == DBL_MAX and not np.any(got["best_raw"])         # DBL_MAX replaces nothing
    got, order = L.tell_host(st, p, cand, np.full(18, 2.0), cand)
    assert list(order) == list(range(18)) and same(got["best_raw"], cand[0])    # the first strict minimum


@pytest.mark.parametrize("name", ("default", "strong", "wide"))
def test_init_against_the_recorded_initFromParcor(fx, L, name):
    parcor, want = fx["init_parcor_" + name], fx["init_state_" + name]
    got = L.init_host(parcor, 99)
    model = M.init(parcor.tolist(), 99)
    d = ulps(got["mean"], want[:9])
    print(name, "initFromParcor: ulps from the record", d.max())
    assert d.max() <= 2.0
    assert same(got["mean"], model["mean"])                     # both are this machine's libm
    assert same(got["cov_upper"], want[9:54]) and got["sigma"] == want[54] == 0.12 and got["cov_retention"] == 0.92
    assert [int(w) for w in got["rng"]] == model["rng"] == M.seed(99)
    assert got["best_score"] == DBL_MAX and got["generations"] == 0 and got["rejected_pairs"] == 0
    assert L.init_host(parcor, 99, L.make_params(cov_retention_target=0.8))["cov_retention"] == 0.8


def test_phase_tables(L):
    from convopeq_amd import _capi as K
    assert [K.CPQ_LEARN_SHORTEST, K.CPQ_LEARN_SHORT, K.CPQ_LEARN_MIDDLE, K.CPQ_LEARN_LONG, K.CPQ_LEARN_ULTRA, K.CPQ_LEARN_CONTINUOUS] == list(M.PHASE_TABLE)
    for mode, ((t1, t2), intervals, targets, step) in M.PHASE_TABLE.items():
        for seconds, want in ((0.0, 1), (math.nextafter(t1, 0.0), 1), (t1, 2), (math.nextafter(t2, 0.0), 2), (t2, 3), (1.0e9, 3), (-5.0, 1)):
            assert L.phase(mode, seconds) == want, (mode, seconds)
        for ph in (1, 2, 3):
            p, interval = L.phase_params(mode, ph)
            assert interval == intervals[ph - 1] and p.cov_retention_target == targets[ph - 1] and p.cov_retention_step == step
            assert (p.sigma_min, p.sigma_max) == (0.03, 0.30) and tuple(p.level_weights) == M.PHASE_WEIGHTS[ph]


def test_normals_against_the_model(L):
    worst = 0.0
    for s in (1, 2, 0xDEADBEEF, 2 ** 64 - 1):
        st = L.init_host(np.zeros(9), s)
        for _ in range(3):
            rng = [int(w) for w in st["rng"]]
            want, words, rejected, _ = M.normals(rng)
            z, st, got_words = L.normals_host(st)
            assert got_words == words and [int(w) for w in st["rng"]] == rng and st["rejected_pairs"] == rejected == 0
            worst = max(worst, ulps(z.ravel(), want).max())
    print("normals: ulps between the library and the model", worst)
    assert worst <= 3.0


def test_normals_from_a_dead_generator_end(L):
    st = L.init_host(np.zeros(9), 1)
    st["rng"] = np.zeros(4, dtype=np.uint64)
    z, after, words = L.normals_host(st)
    assert not z.any() and after["rejected_pairs"] == 81 and words == 81 * 2 * 32 and not after["rng"].any()
    assert M.normals([0, 0, 0, 0])[1:3] == (words, 81)


def test_normals_moments(L):
    st = L.init_host(np.zeros(9), 20240229)
    zs = []
    for _ in range(618):                                        # 618 * 162 = 100116 variates
        z, st, _ = L.normals_host(st)
        zs.append(z.ravel())
    z = np.concatenate(zs)
    n = z.size
    assert n >= 100000 and st["rejected_pairs"] == 0
    mean, var = z.mean(), z.var()
    print("normals:", n, "variates, mean", mean, "variance", var)
    assert abs(mean) <= 4.0 / math.sqrt(n)                      # standard error of the mean of N(0, 1)
    assert abs(var - 1.0) <= 4.0 * math.sqrt(2.0 / n)           # and of its variance
