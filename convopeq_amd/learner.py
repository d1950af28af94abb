"""ShaperLearner -- ctypes wrapper of cpq_learner (include/convopeq_mi355x.h): the reference's CMA-ES around a ShaperScorer, whole
generations on the device.  States travel as dicts of numpy arrays and numbers (state_to_dict / state_from_dict); the host side
of the optimiser (init_host, normals_host, ask_host, tell_host, phase, phase_params) needs no device."""
import ctypes as C

import numpy as np

from . import _capi as K
from ._handle import Handle
from .engine import CpqError

STATE_ARRAYS = ("mean", "cov_upper", "rng", "best_raw", "best_scored")
STATE_SCALARS = ("sigma", "cov_retention", "best_score", "generations", "rejected_pairs")


def _dp(a):
    return a.ctypes.data_as(K.c_double_p)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def state_to_dict(st):
    out = {k: np.array(getattr(st, k)[:], dtype=np.uint64 if k == "rng" else np.float64) for k in STATE_ARRAYS}
    out.update({k: getattr(st, k) for k in STATE_SCALARS})
    return out


def state_from_dict(d):
    st = K.LearnState()
    for k in STATE_ARRAYS:
        v = np.asarray(d[k])
        assert v.shape == (len(getattr(st, k)),), k
        for i, x in enumerate(v):
            getattr(st, k)[i] = int(x) if k == "rng" else float(x)
    for k in STATE_SCALARS:
        setattr(st, k, d[k])
    return st


def make_params(sigma_min=0.03, sigma_max=0.30, cov_retention_target=0.92, cov_retention_step=0.0, level_weights=(0.4, 0.3, 0.2, 0.1)):
    return K.LearnParams(sigma_min, sigma_max, cov_retention_target, cov_retention_step, (C.c_double * 4)(*level_weights))


def _host(rc, what):
    if rc < 0:
        raise CpqError(rc, what + ": " + K.load().cpq_last_error(None).decode())
    return rc


def init_host(parcor, seed, params=None):
    parcor = np.ascontiguousarray(parcor, dtype=np.float64)
    assert parcor.shape == (9,)
    st = K.LearnState()
    _host(K.load().cpq_learn_init_host(_dp(parcor), seed, C.byref(params) if params is not None else None, C.byref(st)), "cpq_learn_init_host")
    return state_to_dict(st)


def normals_host(state):
    """-> (z [18, 9], the state with its generator advanced, generator words drawn)"""
    st, z, words = state_from_dict(state), np.empty((18, 9)), C.c_int32()
    _host(K.load().cpq_learn_normals_host(C.byref(st), _dp(z), C.byref(words)), "cpq_learn_normals_host")
    return z, state_to_dict(st), words.value


def ask_host(state, z):
    st, z, cand = state_from_dict(state), np.ascontiguousarray(z, dtype=np.float64), np.empty((18, 9))
    assert z.shape == (18, 9)
    _host(K.load().cpq_learn_ask_host(C.byref(st), _dp(z), _dp(cand)), "cpq_learn_ask_host")
    return cand


def tell_host(state, params, candidates, fitness, mapped=None):
    """-> (the state after update() and the best tracking, the sort [18])"""
    st = state_from_dict(state)
    cand, fit = np.ascontiguousarray(candidates, dtype=np.float64), np.ascontiguousarray(fitness, dtype=np.float64)
    assert cand.shape == (18, 9) and fit.shape == (18,)
    if mapped is not None:
        mapped = np.ascontiguousarray(mapped, dtype=np.float64)
        assert mapped.shape == (18, 9)
    order = np.empty(18, dtype=np.int32)
    _host(K.load().cpq_learn_tell_host(C.byref(st), C.byref(params), _dp(cand), _dp(mapped) if mapped is not None else None, _dp(fit), _ip(order)),
          "cpq_learn_tell_host")
    return state_to_dict(st), order


def phase(mode, playback_seconds):
    return _host(K.load().cpq_learn_phase(mode, float(playback_seconds)), "cpq_learn_phase")


def phase_params(mode, ph):
    """-> (LearnParams, generation interval in seconds)"""
    p, iv = K.LearnParams(), C.c_double()
    _host(K.load().cpq_learn_phase_params(mode, ph, C.byref(p), C.byref(iv)), "cpq_learn_phase_params")
    return p, iv.value


class ShaperLearner(Handle):
    """CMA-ES over the scorer's learners.  The scorer is borrowed and kept alive by this object."""
    _PREFIX = "cpq_learner"

    def __init__(self, scorer):
        self.scorer = scorer
        self._open(scorer._h)
        self.n_learners = scorer.n_learners

    def init(self, parcor, seed, learner=K.CPQ_ALL_STREAMS):
        parcor = np.ascontiguousarray(parcor, dtype=np.float64)
        assert parcor.shape == (9,)
        self._check(self._lib.cpq_learner_init(self._h, learner, _dp(parcor), seed))

    def set_params(self, params):
        self._check(self._lib.cpq_learner_set_params(self._h, C.byref(params)))

    def run(self, n_generations):
        """enqueues n_generations of ask, score, tell for every learner holding two or more segments, and returns"""
        self._check(self._lib.cpq_learner_run(self._h, n_generations))

    def get_state(self, learner):
        st = K.LearnState()
        self._check(self._lib.cpq_learner_get_state(self._h, learner, C.byref(st)))
        return state_to_dict(st)

    def set_state(self, learner, state):
        st = state_from_dict(state)
        self._check(self._lib.cpq_learner_set_state(self._h, learner, C.byref(st)))

    def read_generation(self, learner):
        """the last generation: dict of z, candidates, mapped [18, 9], scores [18], order [18]"""
        z, cand, mapped, scores, order = np.empty((18, 9)), np.empty((18, 9)), np.empty((18, 9)), np.empty(18), np.empty(18, dtype=np.int32)
        self._check(self._lib.cpq_learner_read_generation(self._h, learner, _dp(z), _dp(cand), _dp(mapped), _dp(scores), _ip(order)))
        return {"z": z, "candidates": cand, "mapped": mapped, "scores": scores, "order": order}

    def history(self, learner):
        n = C.c_int32()
        self._check(self._lib.cpq_learner_read_history(self._h, learner, None, C.byref(n)))
        out = np.empty(n.value)
        if n.value:
            self._check(self._lib.cpq_learner_read_history(self._h, learner, _dp(out), C.byref(n)))
        return out

    def published(self, learner):
        k = np.empty(9)
        self._check(self._lib.cpq_learner_published(self._h, learner, _dp(k)))
        return k

    def last_timing(self):
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.cpq_learner_last_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def multi_start(self, seeds=(1, 2, 3, 4, 5), generations=3):
        """The reference's multi-start (src/NoiseShaperLearner.cpp:772-835): from the states held now, every seed runs
        `generations` generations one at a time; after each, a learner whose generation's best score is below its best so far
        keeps that state.  Every learner ends in its best state (its initial one if no generation scored below DBL_MAX).
        Returns the best restart score per learner."""
        L = self.n_learners
        initial = [self.get_state(i) for i in range(L)]
        best_state = [dict(s) for s in initial]
        best_score = [np.finfo(np.float64).max] * L
        for seed in seeds:
            for i in range(L):
                s = dict(initial[i])
                s["rng"] = init_host(np.zeros(9), seed + i)["rng"]
                self.set_state(i, s)
            for _ in range(generations):
                self.run(1)
                for i in range(L):
                    h = self.history(i)
                    if h.size and h[0] < best_score[i]:
                        best_score[i] = float(h[0])
                        best_state[i] = self.get_state(i)
        for i in range(L):
            self.set_state(i, best_state[i])
        return best_score
