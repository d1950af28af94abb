"""k_learn_tell alone (cpq_diag_learn_tell) against cpq_learn_tell_host, bit for bit in every field of every state, at 1, 63, 64, 65
and 129 learners -- a workgroup is a learner, so the counts walk the grid and not a tile -- with inputs no run produces on
demand: tied fitness, NaN and DBL_MAX fitness, fewer than six finite values, sigma on either clamp, a running best that is and
is not beaten, and covariances with entries on computeCholesky's floors and below sanitize's 1e-15.  The learners of a call
cycle through the fitness kinds, so every count holds all of them (but the single learner, which is parametrised over them)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DBL_MAX = np.finfo(np.float64).max
NAN = float("nan")
PARAMS = {"std": (0.03, 0.30, 0.92, 0.0), "clamp_lo": (0.25, 0.30, 0.80, 0.02), "clamp_hi": (0.01, 0.05, 1.0, 0.0)}


@pytest.fixture(scope="module")
def L():
    from convopeq_amd import learner
    return learner


def fitness(kind, i):
    base = np.array([1.0 + 0.37 * ((7 * j + 5 * i) % 18) + 0.01 * j for j in range(18)])
    if kind == 0:
        return base
    if kind == 1:                                               # ties, inside the elite and across its edge
        return np.floor(base)
    if kind == 2:
        base[[1, 4, 9]] = NAN
        base[[0, 7, 12, 13]] = DBL_MAX
        return base
    if kind == 3:                                               # four finite values: the elite takes DBL_MAX and NaN candidates
        out = np.full(18, DBL_MAX)
        out[[2, 3]] = NAN
        out[[5, 8, 11, 17]] = [4.0, 2.0, 2.0, 1e18]
        return out
    if kind == 4:
        return np.full(18, NAN)
    return np.full(18, DBL_MAX)


def covariance(kind):
    m = np.eye(9)
    if kind % 3 == 1:
        a = np.array([[((3 * r + 5 * c + r * c) % 7 - 3) / 8.0 for c in range(9)] for r in range(9)])
        m = a @ a.T / 4.0 + 0.5 * np.eye(9)
        m[2, 2], m[5, 5], m[7, 7] = 0.0, -1.0, 1.0e-20          # computeCholesky's floors
    elif kind % 3 == 2:
        m = np.full((9, 9), 1.0e-16) + np.eye(9)                # with retention 1 the update sanitizes these to 0
    return np.array([m[r, c] for r in range(9) for c in range(r, 9)])


def build(L, n, kinds):
    states, cands, mapped, fits = [], [], [], []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        st = L.init_host(0.05 * np.cos(np.arange(9) + i), 1000 + i)
        st["cov_upper"] = covariance(i)
        st["sigma"] = (0.12, 0.03, 0.30)[i % 3]
        z, st, _ = L.normals_host(st)
        c = L.ask_host(st, z)
        if i % 4 == 1:
            st["best_score"] = 1.5                              # beaten by some kinds only
            st["best_raw"], st["best_scored"] = np.full(9, 0.25), np.full(9, 0.125)
        st["generations"] = i
        states.append(st)
        cands.append(c)
        mapped.append(np.clip(np.tanh(c), -0.85, 0.85))
        fits.append(fitness(kind, i))
    return states, np.array(cands), np.array(mapped), np.array(fits)


def run(L, states, params, cands, mapped, fits):
    from convopeq_amd import _capi as K
    arr = (K.LearnState * len(states))(*[L.state_from_dict(s) for s in states])
    dp = lambda a: np.ascontiguousarray(a).ctypes.data_as(K.c_double_p)
    c, m, f = np.ascontiguousarray(cands), np.ascontiguousarray(mapped), np.ascontiguousarray(fits)
    rc = K.load().cpq_diag_learn_tell(len(states), arr, C.byref(params), dp(c), dp(m), dp(f))
    assert rc == K.CPQ_OK, K.load().cpq_last_error(None)
    return [L.state_to_dict(s) for s in arr]


def check(L, n, kinds, pname):
    params = L.make_params(*PARAMS[pname])
    states, cands, mapped, fits = build(L, n, kinds)
    got = run(L, states, params, cands, mapped, fits)
    clamped = 0
    for i in range(n):
        want, _ = L.tell_host(states[i], params, cands[i], fits[i], mapped[i])
        for k, v in want.items():
            a, b = np.atleast_1d(np.asarray(v)), np.atleast_1d(np.asarray(got[i][k]))
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), (n, i, k)
        clamped += want["sigma"] in PARAMS[pname][:2]
    return clamped


@pytest.mark.parametrize("kind", range(6))
def test_one_learner(L, kind):
    check(L, 1, [kind], "std")


@pytest.mark.parametrize("n", [63, 64, 65, 129])
@pytest.mark.parametrize("pname", ["std", "clamp_lo", "clamp_hi"])
def test_many_learners(L, n, pname):
    clamped = check(L, n, list(range(6)), pname)
    if pname != "std":
        assert clamped > n // 2                                 # the case is on its clamp


def test_refusals(L):
    from convopeq_amd import _capi as K
    lib = K.load()
    st, p, x = (K.LearnState * 1)(), L.make_params(), np.zeros(162)
    xp = x.ctypes.data_as(K.c_double_p)
    assert lib.cpq_diag_learn_tell(0, st, C.byref(p), xp, xp, xp) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_diag_learn_tell((1 << 20) + 1, st, C.byref(p), xp, xp, xp) == K.CPQ_ERR_INVALID_ARG
    for args in ((None, C.byref(p), xp, xp, xp), (st, None, xp, xp, xp), (st, C.byref(p), None, xp, xp), (st, C.byref(p), xp, None, xp),
                 (st, C.byref(p), xp, xp, None)):
        assert lib.cpq_diag_learn_tell(1, *args) == K.CPQ_ERR_INVALID_ARG
