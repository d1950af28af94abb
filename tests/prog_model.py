"""numpy restatement of the programme loudness of convopeq_amd/csrc/prog_plan.hpp (EBU R 128: BS.1770-4 gating, EBU Tech 3342
range), independent of the C++: the K-weighting is tests/meter_model.py's sequential Direct Form I (the reference's coefficients),
run in fp64 or np.longdouble; hop sums, blocks, gates and percentiles follow the header's definition.

  hop_sums(x, rate, dtype)   x [2 S, n] -> E [S, n // H]: K-weighted squares of both channels per hop of H = rate / 10
  finish(E, H, dtype)        one stream's hop sums -> the figures, the mean squares behind them, and how far every block stands
                             from the gates

Gates are decided on mean squares (z > zAbs, z > 0.1 m, z > 0.01 m), blocks are added left to right, the percentile index is
(p (n - 1) + 50) // 100: all as the header states.  Means are numpy sums: the device's tree adds in another order."""
import math

import numpy as np

import meter_model as M

Z_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)
NEG_INF = -math.inf


def hop_len(rate):
    assert rate == int(rate) and 8000 <= rate <= 768000 and int(rate) % 10 == 0
    return int(rate) // 10


def _biquad_scalar(coef, x):
    """meter_model.Biquad.run for one fp64 row from a zero state, as a loop over Python floats (the same operations in the
    same order; much faster than numpy for a few long rows)"""
    b0, b1, b2, a1, a2 = (float(v) for v in coef)
    out = [0.0] * len(x)
    x1 = x2 = y1 = y2 = 0.0
    for i, v in enumerate(x.tolist()):
        y = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        out[i] = y
        x2, x1 = x1, v
        y2, y1 = y1, y
    return np.array(out)


def kweighted(x, rate, dtype=np.float64):
    x = M.scrub(np.atleast_2d(x))
    if dtype is np.float64 and x.shape[0] <= 4:
        pre, rlb = M.kweighting(float(rate))
        return np.stack([_biquad_scalar(rlb, _biquad_scalar(pre, row)) for row in x])
    assert x.shape[0] % 2 == 0
    return M.LoudnessMeter(float(rate), x.shape[0] // 2, dtype).weighted(x)


def hop_sums(x, rate, dtype=np.float64, lengths=None):
    """E [S, n // H] in dtype.  lengths: the samples of each stream that count (rows padded with anything behind them)"""
    H = hop_len(rate)
    y = kweighted(x, rate, dtype)
    n = y.shape[1] // H
    sq = (y[:, :n * H] * y[:, :n * H]).reshape(y.shape[0], n, H).sum(axis=2)
    E = sq[0::2] + sq[1::2]
    if lengths is None:
        return E
    return [E[s, :lengths[s] // H] for s in range(E.shape[0])]


def blocks(E, w, H):
    """z[b - (w - 1)] for b >= w - 1: (E[b - w + 1] + ... + E[b]) / (w H), added left to right"""
    n = len(E) - (w - 1)
    if n <= 0:
        return E[:0].copy()
    s = E[0:n].copy()
    for i in range(1, w):
        s = s + E[i:i + n]
    return s / E.dtype.type(w * H)


def loudness(z):
    if isinstance(z, float):
        return -0.691 + 10.0 * math.log10(z) if z > 0.0 else NEG_INF
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def _dist(z, gate):
    """smallest |L(z) - L(gate)| over the blocks (inf where there is none, or no gate)"""
    if len(z) == 0 or not gate > 0.0:
        return math.inf
    with np.errstate(divide="ignore"):
        return float(np.min(np.abs(10.0 * np.log10(np.asarray(z, dtype=np.float64) / float(gate)))))


def finish(E, H, dtype=np.float64):
    E = np.asarray(E, dtype=dtype)
    lf = (lambda v: loudness(float(v))) if dtype is np.float64 else (lambda v: float(loudness(np.longdouble(v))) if v > 0 else NEG_INF)
    r = dict(n_hops=len(E))
    zm = blocks(E, 4, H)
    r["n_blocks"] = len(zm)
    a = zm[zm > Z_ABS]
    r["n_abs"] = len(a)
    m1 = a.sum() / dtype(len(a)) if len(a) else dtype(0.0)
    g = a[a > 0.1 * m1]
    r["n_rel"] = len(g)
    r["z_gate"], r["z_int"] = m1, (g.sum() / dtype(len(g)) if len(g) else dtype(0.0))
    r["relative_gate"] = lf(m1) - 10.0 if len(a) else NEG_INF
    r["integrated"] = lf(r["z_int"]) if len(g) else NEG_INF
    r["z_mom_max"] = zm.max() if len(zm) else dtype(0.0)
    r["momentary_max"] = lf(r["z_mom_max"]) if len(zm) else NEG_INF
    zs = blocks(E, 30, H)
    r["z_short_max"] = zs.max() if len(zs) else dtype(0.0)
    r["short_term_max"] = lf(r["z_short_max"]) if len(zs) else NEG_INF
    c = zs[0::10]                                   # b = 29, 39, ...
    ca = c[c > Z_ABS]
    ms = ca.sum() / dtype(len(ca)) if len(ca) else dtype(0.0)
    k = np.sort(ca[ca > 0.01 * ms])
    n = len(k)
    r["n_cand"], r["n_short_abs"], r["z_short_mean"] = len(c), len(ca), ms
    r["n_short_kept"] = n
    r["z_lo"], r["z_hi"] = (k[(10 * (n - 1) + 50) // 100], k[(95 * (n - 1) + 50) // 100]) if n else (dtype(0.0), dtype(0.0))
    r["range"] = lf(r["z_hi"]) - lf(r["z_lo"]) if n else 0.0
    # how far the decisions stand from their gates, in LU (hop sums of inf leave nan here: no distance)
    with np.errstate(invalid="ignore", divide="ignore"):
        r["gate_margin"] = min(_dist(zm, Z_ABS), _dist(a, 0.1 * float(m1)), _dist(c, Z_ABS), _dist(ca, 0.01 * float(ms)))
        r["short_gap"] = float(np.min(np.diff(10.0 * np.log10(k.astype(np.float64))))) if n > 1 else math.inf
    return r
