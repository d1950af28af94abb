"""ctypes callers of cpq_diag_score_spectrum / _score_lattice / _score_reduce and the table of their refusals (every "Refused
unless" rule of include/convopeq_mi355x.h once, with a piece of the message cpq_last_error(NULL) must hold).  The CPU test walks
the table without a device -- the arguments are checked before one is looked for -- and the device test walks it again."""
import ctypes as C

import numpy as np

from convopeq_amd import _capi as K

LEN, BINS = 4096, 2049
INVALID, NO_DEVICE = K.CPQ_ERR_INVALID_ARG, K.CPQ_ERR_NO_DEVICE
FILL = b"\xff" * 8


def _dp(a):
    return a.ctypes.data_as(K.c_double_p)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def spectrum(lib, rate, rows, thr, evals, n_slots, thresholds_only=False, n_rows=None, n_thr=None):
    """rows [n, 2, 4096], thr [m, 2049], evals [(row, thr, slot, alpha)] -> (rc, thr after, parts [n_slots, 5], blended [n_slots])"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    thr = np.array(thr, dtype=np.float64, order="C")
    table = (K.DiagScoreEval * max(1, len(evals)))(*[K.DiagScoreEval(r, t, s, 0, a) for r, t, s, a in evals])
    parts, blended = np.zeros((max(n_slots, 1), 5)), np.zeros(max(n_slots, 1))
    rc = lib.cpq_diag_score_spectrum(rate, len(rows) if n_rows is None else n_rows, _dp(rows), len(thr) if n_thr is None else n_thr, _dp(thr),
                                     len(evals), table, n_slots, int(thresholds_only), parts.ctypes.data_as(C.POINTER(K.ScoreParts)), _dp(blended))
    return rc, thr, parts, blended


def lattice(lib, bits, seg, n_dst, chains, coef, rng, n_src=None, n_coef=None, n_rng=None):
    """seg [n, 4096], chains [(src, dst, coef, rng)], coef [c, 9], rng [r, 4] uint64 -> (rc, err [n_dst, 4096])"""
    seg = np.ascontiguousarray(seg, dtype=np.float64)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    rng = np.ascontiguousarray(rng, dtype=np.uint64)
    table = (K.DiagScoreChain * max(1, len(chains)))(*[K.DiagScoreChain(*map(int, c)) for c in chains])
    err = np.zeros((max(n_dst, 1), LEN))
    rc = lib.cpq_diag_score_lattice(bits, len(seg) if n_src is None else n_src, _dp(seg), n_dst, _dp(err), len(chains), table,
                                    len(coef) if n_coef is None else n_coef, _dp(coef), len(rng) if n_rng is None else n_rng,
                                    rng.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, err


def reduce(lib, n_learners, n_cand, counts, state, blended, weights):
    """counts [L, 4], state [L * C], blended [L * C, 16], weights [4] -> (rc, scores [L * C])"""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    state = np.ascontiguousarray(state, dtype=np.int32)
    blended = np.ascontiguousarray(blended, dtype=np.float64)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    scores = np.zeros(max(1, n_learners * n_cand))
    rc = lib.cpq_diag_score_reduce(n_learners, n_cand, _ip(counts), _ip(state), _dp(blended), _dp(weights), _dp(scores))
    return rc, scores


def _spectrum_bad(lib, **kw):
    a = dict(rate=48000.0, rows=np.zeros((2, 2, LEN)), thr=np.zeros((2, BINS)), evals=[(0, 0, 0, 0.5), (1, 1, 1, 0.5)], n_slots=2)
    a.update(kw)
    return spectrum(lib, **a)[0]


def _lattice_bad(lib, **kw):
    a = dict(bits=16, seg=np.zeros((2, LEN)), n_dst=2, chains=[(0, 0, 0, 0), (1, 1, 1, 1)], coef=np.zeros((2, 9)), rng=np.ones((2, 4), dtype=np.uint64))
    a.update(kw)
    return lattice(lib, **a)[0]


def _reduce_bad(lib, **kw):
    a = dict(n_learners=2, n_cand=3, counts=[[4, 4, 4, 4], [1, 0, 0, 0]], state=np.zeros(6), blended=np.zeros((6, 16)), weights=[0.4, 0.3, 0.2, 0.1])
    a.update(kw)
    return reduce(lib, **a)[0]


# (entry, what is wrong, call, piece of the message)
REFUSALS = [
    ("spectrum", "rate 0", lambda l: _spectrum_bad(l, rate=0.0), "sample rate"),
    ("spectrum", "rate inf", lambda l: _spectrum_bad(l, rate=float("inf")), "sample rate"),
    ("spectrum", "rate nan", lambda l: _spectrum_bad(l, rate=float("nan")), "sample rate"),
    ("spectrum", "no rows", lambda l: _spectrum_bad(l, n_rows=0), ">= 1"),
    ("spectrum", "no thr", lambda l: _spectrum_bad(l, n_thr=0), ">= 1"),
    ("spectrum", "no evals", lambda l: _spectrum_bad(l, evals=[]), ">= 1"),
    ("spectrum", "no slots", lambda l: _spectrum_bad(l, n_slots=0), ">= 1"),
    ("spectrum", "too many rows", lambda l: _spectrum_bad(l, n_rows=(1 << 15) + 1), "2^28"),
    ("spectrum", "row past the end", lambda l: _spectrum_bad(l, evals=[(2, 0, 0, 0.5)]), "row 2 outside 0..1"),
    ("spectrum", "row negative", lambda l: _spectrum_bad(l, evals=[(-1, 0, 0, 0.5)]), "row -1"),
    ("spectrum", "thr past the end", lambda l: _spectrum_bad(l, evals=[(0, 2, 0, 0.5)]), "thr 2 outside 0..1"),
    ("spectrum", "thr negative", lambda l: _spectrum_bad(l, evals=[(0, -1, 0, 0.5)]), "thr -1"),
    ("spectrum", "slot past the end", lambda l: _spectrum_bad(l, evals=[(0, 0, 2, 0.5)]), "slot 2 outside 0..1"),
    ("spectrum", "slot negative", lambda l: _spectrum_bad(l, evals=[(0, 0, -1, 0.5)]), "slot -1"),
    ("spectrum", "slot twice", lambda l: _spectrum_bad(l, evals=[(0, 0, 1, 0.5), (1, 1, 1, 0.5)]), "slot 1 named twice"),
    ("spectrum", "thr twice, thresholds only", lambda l: _spectrum_bad(l, evals=[(0, 1, 0, 0.5), (1, 1, 1, 0.5)], thresholds_only=True), "thr 1 written twice"),
    ("lattice", "bits 0", lambda l: _lattice_bad(l, bits=0), "bit depth 0"),
    ("lattice", "bits 33", lambda l: _lattice_bad(l, bits=33), "bit depth 33"),
    ("lattice", "no src", lambda l: _lattice_bad(l, n_src=0), ">= 1"),
    ("lattice", "no dst", lambda l: _lattice_bad(l, n_dst=0), ">= 1"),
    ("lattice", "no chains", lambda l: _lattice_bad(l, chains=[]), ">= 1"),
    ("lattice", "no coef", lambda l: _lattice_bad(l, n_coef=0), ">= 1"),
    ("lattice", "no rng", lambda l: _lattice_bad(l, n_rng=0), ">= 1"),
    ("lattice", "too many src", lambda l: _lattice_bad(l, n_src=(1 << 16) + 1), "2^28"),
    ("lattice", "src past the end", lambda l: _lattice_bad(l, chains=[(2, 0, 0, 0)]), "src 2 outside 0..1"),
    ("lattice", "src negative", lambda l: _lattice_bad(l, chains=[(-1, 0, 0, 0)]), "src -1"),
    ("lattice", "dst past the end", lambda l: _lattice_bad(l, chains=[(0, 2, 0, 0)]), "dst 2 outside 0..1"),
    ("lattice", "dst negative", lambda l: _lattice_bad(l, chains=[(0, -1, 0, 0)]), "dst -1"),
    ("lattice", "coef past the end", lambda l: _lattice_bad(l, chains=[(0, 0, 2, 0)]), "coef 2 outside 0..1"),
    ("lattice", "coef negative", lambda l: _lattice_bad(l, chains=[(0, 0, -1, 0)]), "coef -1"),
    ("lattice", "rng past the end", lambda l: _lattice_bad(l, chains=[(0, 0, 0, 2)]), "rng 2 outside 0..1"),
    ("lattice", "rng negative", lambda l: _lattice_bad(l, chains=[(0, 0, 0, -1)]), "rng -1"),
    ("lattice", "dst twice", lambda l: _lattice_bad(l, chains=[(0, 1, 0, 0), (1, 1, 1, 1)]), "dst 1 named twice"),
    ("reduce", "no learners", lambda l: _reduce_bad(l, n_learners=0), ">= 1"),
    ("reduce", "no candidates", lambda l: _reduce_bad(l, n_cand=0), ">= 1"),
    ("reduce", "too many pairs", lambda l: _reduce_bad(l, n_learners=1, n_cand=(1 << 20) + 1, counts=[[0] * 4], state=np.zeros(1), blended=np.zeros((1, 16))), "2^20"),
    ("reduce", "negative count", lambda l: _reduce_bad(l, counts=[[4, 4, 4, 4], [0, -1, 0, 0]]), "learner 1, level 1: count -1"),
    ("reduce", "counts above 16", lambda l: _reduce_bad(l, counts=[[4, 4, 4, 5], [0, 0, 0, 0]]), "learner 0: counts sum to 17"),
    ("reduce", "one count above 16", lambda l: _reduce_bad(l, counts=[[0, 0, 0, 0], [0, 0, 17, 0]]), "count 17"),
]

_NULL_D, _NULL_I = K.c_double_p(), C.POINTER(C.c_int32)()


def _null_calls(lib):
    """every pointer of every entry null once, the rest valid"""
    z, zi = np.zeros(2 * 2 * LEN), np.zeros(64, dtype=np.int32)
    ev, ch = (K.DiagScoreEval * 1)(K.DiagScoreEval(0, 0, 0, 0, 0.5)), (K.DiagScoreChain * 1)(K.DiagScoreChain(0, 0, 0, 0))
    u = np.ones(4, dtype=np.uint64)
    parts = np.zeros(5)
    sp = [_dp(z), _dp(z), ev, parts.ctypes.data_as(C.POINTER(K.ScoreParts)), _dp(z)]
    for i in range(5):
        a = list(sp)
        a[i] = None
        yield "spectrum", lib.cpq_diag_score_spectrum(48000.0, 1, a[0], 1, a[1], 1, a[2], 1, 0, a[3], a[4])
    la = [_dp(z), _dp(z), ch, _dp(z), u.ctypes.data_as(C.POINTER(C.c_uint64))]
    for i in range(5):
        a = list(la)
        a[i] = None
        yield "lattice", lib.cpq_diag_score_lattice(16, 1, a[0], 1, a[1], 1, a[2], 1, a[3], 1, a[4])
    re = [_ip(zi), _ip(zi), _dp(z), _dp(z), _dp(z)]
    for i in range(5):
        a = list(re)
        a[i] = None
        yield "reduce", lib.cpq_diag_score_reduce(1, 1, *a)


def walk_refusals(lib):
    """-> [(entry, what, rc, message)]"""
    out = []
    for entry, what, call, piece in REFUSALS:
        rc = call(lib)
        out.append((entry, what, rc, lib.cpq_last_error(None).decode()))
    for entry, rc in _null_calls(lib):
        out.append((entry, "null pointer", rc, lib.cpq_last_error(None).decode()))
    return out


def check_refusals(lib):
    res = walk_refusals(lib)
    assert len(res) == len(REFUSALS) + 15
    pieces = [p for _, _, _, p in REFUSALS] + ["null buffer"] * 15
    bad = [(e, w, rc, msg) for (e, w, rc, msg), p in zip(res, pieces) if rc != INVALID or p not in msg or ("score_" + e) not in msg]
    assert bad == [], bad


def valid_calls(lib):
    """the defaults of the table: -> [rc]"""
    return [_spectrum_bad(lib), _spectrum_bad(lib, thresholds_only=True), _lattice_bad(lib), _reduce_bad(lib)]
