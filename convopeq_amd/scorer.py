"""ShaperScorer -- ctypes wrapper of cpq_scorer (include/convopeq_mi355x.h): the fitness function of the adaptive noise shaper's
learner, for every candidate of every learner in one call.  Host numpy arrays in and out; set_audio_device takes a torch tensor.
No fallback: without a gfx950 device the constructor raises."""
import ctypes as C

import numpy as np

from . import _capi as K
from ._handle import Handle
from .engine import CpqError

PARTS = ("noise_power", "spectral_flatness_penalty", "hf_penalty", "time_domain_rms", "composite_score")


def _dp(a):
    return a.ctypes.data_as(K.c_double_p)


def score_design(sample_rate_hz):
    """configureForSampleRate on the host: dict of the per-bin tables and scalars"""
    n = K.CPQ_SCORE_BINS
    w, bark, ath, width = (np.empty(n) for _ in range(4))
    band, rng = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    bins, scalars = np.empty(4, dtype=np.int32), np.empty(4)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = K.load().cpq_score_design(float(sample_rate_hz), _dp(w), _dp(bark), _dp(ath), _dp(width), ip(band), ip(rng), ip(bins), _dp(scalars))
    if rc != K.CPQ_OK:
        raise CpqError(rc, "cpq_score_design")
    return {"weight": w, "bark": bark, "ath_db": ath, "width": width, "band": band, "range": rng, "bins": bins, "scalars": scalars}


def _segments(fn, *head):
    segs = (K.ScoreSegment * K.CPQ_SCORE_MAX_SEGMENTS)()
    n, counts = C.c_int32(), (C.c_int32 * 4)()
    rc = fn(*head, segs, C.byref(n), counts)
    if rc != K.CPQ_OK:
        raise CpqError(rc, fn.__name__)
    return [(s.start, s.level, s.type, s.gain) for s in segs[:n.value]], list(counts)


def select_segments(left, right):
    """buildTrainingSegments' selection on the host: ([(start, level, type, gain)], counts per level)"""
    left, right = np.ascontiguousarray(left, dtype=np.float64), np.ascontiguousarray(right, dtype=np.float64)
    assert left.shape == right.shape and left.ndim == 1
    return _segments(K.load().cpq_score_select_segments, _dp(left), _dp(right), left.size)


class ShaperScorer(Handle):
    _PREFIX = "cpq_scorer"

    def __init__(self, n_learners=1, max_candidates=18, sample_rate_hz=48000.0, bit_depth=16, level_weights=(0.4, 0.3, 0.2, 0.1),
                 coeff_safety_margin=0.85, stability_check=True, rng_mode=K.CPQ_SCORE_RNG_FRESH):
        desc = K.ScorerDesc(n_learners, max_candidates, sample_rate_hz, bit_depth, (C.c_double * 4)(*level_weights), coeff_safety_margin,
                            int(bool(stability_check)), rng_mode)
        self._open(C.byref(desc))
        self.n_learners, self.max_candidates = n_learners, max_candidates

    def buildTrainingSegments(self, learner, left, right):
        """the learner's segments from the most recent samples of the two rows; returns how many it holds"""
        left, right = np.ascontiguousarray(left, dtype=np.float64), np.ascontiguousarray(right, dtype=np.float64)
        assert left.shape == right.shape and left.ndim == 1
        n = C.c_int32()
        self._check(self._lib.cpq_scorer_set_audio(self._h, learner, _dp(left), _dp(right), left.size, C.byref(n)))
        return n.value

    set_audio = buildTrainingSegments

    def set_audio_device(self, learner, rows):
        """rows: a contiguous float64 device tensor [2, n]"""
        assert rows.dim() == 2 and rows.shape[0] == 2 and rows.is_contiguous()
        n_samples, n = rows.shape[1], C.c_int32()
        base = rows.data_ptr()
        self._check(self._lib.cpq_scorer_set_audio_device(self._h, learner, C.c_void_p(base), C.c_void_p(base + 8 * n_samples), n_samples, C.byref(n)))
        return n.value

    def segments(self, learner):
        return _segments(self._lib.cpq_scorer_get_segments, self._h, learner)

    def thresholds(self, learner, segment):
        out = np.empty(K.CPQ_SCORE_BINS)
        self._check(self._lib.cpq_scorer_read_thresholds(self._h, learner, segment, _dp(out)))
        return out

    def _score(self, fn, k, with_parts):
        k = np.ascontiguousarray(k, dtype=np.float64)
        assert k.ndim == 3 and k.shape[0] == self.n_learners and k.shape[2] == 9
        n_cand = k.shape[1]
        scores = np.empty((self.n_learners, n_cand))
        parts = np.empty((self.n_learners, n_cand, K.CPQ_SCORE_MAX_SEGMENTS, 5)) if with_parts else None
        pp = parts.ctypes.data_as(C.POINTER(K.ScoreParts)) if with_parts else None
        self._check(fn(self._h, _dp(k), n_cand, _dp(scores), pp))
        return (scores, parts) if with_parts else scores

    def evaluateCandidateMapped(self, mapped, parts=False):
        """mapped [n_learners, n_candidates, 9] -> scores [n_learners, n_candidates] (and parts [.., 16, 5], columns PARTS)"""
        return self._score(self._lib.cpq_scorer_score, mapped, parts)

    def evaluateCandidate(self, raw, parts=False):
        return self._score(self._lib.cpq_scorer_score_raw, raw, parts)

    score, score_raw = evaluateCandidateMapped, evaluateCandidate

    def set_rng_start(self, state):
        state = np.ascontiguousarray(state, dtype=np.uint64)
        assert state.shape == (2, 4)
        self._check(self._lib.cpq_scorer_set_rng_start(self._h, state.ctypes.data_as(C.POINTER(C.c_uint64))))

    def read_error(self, learner, candidate, segment):
        out = np.empty((2, K.CPQ_SCORE_SEGMENT_LEN))
        self._check(self._lib.cpq_scorer_read_error(self._h, learner, candidate, segment, _dp(out[0]), _dp(out[1])))
        return out

    def last_timing(self):
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.cpq_scorer_last_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value
