"""numpy restatement of the adaptive shaper of the dither stage (convopeq_amd/csrc/dither_design.cpp, latticeProcess):
LatticeNoiseShaper of the reference, vectorised over channels, sample after sample, in the reference's operation order, with
coefficients per stream.

Per sample and channel, states s[0..8], coefficients c[0..8]: x = in * headroom; p_j = fma(s[4+j], c[4+j], s[j] * c[j]), j < 4;
fb = ((p_0 + p_2) + (p_1 + p_3)) + s[8] * c[8]; y = x + fb; v = y clamped to [-1, 1 - scale] by two comparisons (a NaN passes)
plus (u1 + u2 - 1) * scale; q = rint(v * inv) clamped to [-inv, inv - 1] (a NaN stays); yq = q * scale; err = yq - y, 0 when not
finite, clamped to +-2 scale; f = err, and for i < 9: b = s[i], nf = f + c[i] b, s[i] = clamp(c[i] f + b, -2, 2), f = nf.

Python floats and numpy's elementwise operations are IEEE fp64 without contraction.  The four fused terms are the exception: the
interpreter has no fma, so each is computed in exact rational arithmetic and rounded once (float() of a Fraction rounds
correctly).  States and coefficients are always finite, so the rational route never meets a NaN or an infinity.

Every stream is a DSPCore of its own: all L channels start from one generator state, all R channels from another; the states are
LatticeNoiseShaper::rngState, the constants of the 4-tap shaper."""
import math
from fractions import Fraction

import numpy as np

from dither_model import H, SEEDS4, _uniform, encode16, scrub  # noqa: F401  (encode16 and scrub are handed on to the tests)

ADAPTIVE9 = 4
ORDER = 9
LIMIT = 0.85
DEFAULT = (-0.003796, -0.006752, 0.008418, -0.010546, 0.004716, -0.007624, -0.020750, -0.002049, -0.003632)


def clamp_coeffs(k):
    """setCoefficients: clampCoeff of what is given (not finite -> 0, else clamped to +-0.85), the missing trailing ones 0"""
    k = [float(v) for v in k]
    assert len(k) <= ORDER
    out = [0.0 if not math.isfinite(v) else LIMIT if v > LIMIT else -LIMIT if v < -LIMIT else v for v in k]
    return out + [0.0] * (ORDER - len(out))


def fma(a, b, c):
    """round(a * b + c), one rounding, for finite floats"""
    if a == 0.0 or b == 0.0:
        return a * b + c                        # a signed zero plus c: exact as it stands
    r = Fraction(a) * Fraction(b) + Fraction(c)
    return float(r) if r else 0.0               # an exact cancellation is +0 in round-to-nearest


def _fma_rows(a, b, c):
    return np.array([fma(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])


def recorded(fx, case, bits):
    """tests/golden/lattice_ref.npz: the reference's output rows of one case: codes * scale, NaN where it delivered one"""
    key = f"{case}_{bits}"
    n = fx["input"].shape[1]
    y = fx["codes_" + key].astype(np.float64) / float(1 << (bits - 1))
    bad = np.unpackbits(fx["bad_" + key], axis=1)[:, :n].astype(bool)
    negzero = np.unpackbits(fx["negzero_" + key], axis=1)[:, :n].astype(bool)
    return np.where(bad, np.nan, np.where(negzero, -0.0, y))


class Lattice:
    def __init__(self, n_streams, bits):
        assert 1 <= bits <= 32
        self.S, self.bits = n_streams, bits
        self.inv = math.ldexp(1.0, bits - 1)
        self.scale = 1.0 / self.inv
        self.rng = np.array([[SEEDS4[c % 2][k] for c in range(2 * n_streams)] for k in range(4)], dtype=np.uint64)
        self.coef = np.empty((ORDER, 2 * n_streams))
        self.coef[:] = np.array(DEFAULT)[:, None]
        self.reset()

    def reset(self):
        self.state = np.zeros((ORDER, 2 * self.S))

    prepare = reset     # DSPCore::prepare: the published set is applied again at the first callback; no reseed

    def set_coeffs(self, stream, k):
        """applyMatchedCoefficients of one stream (None: all): both of its channels, states cleared; the generators run on"""
        cols = slice(None) if stream is None else slice(2 * stream, 2 * stream + 2)
        self.coef[:, cols] = np.array(clamp_coeffs(k))[:, None]
        self.state[:, cols] = 0.0

    def coeffs(self, stream):
        return self.coef[:, 2 * stream].copy()

    def process(self, x, headroom=H, scrubbed=False):
        """x [2 S, n] -> the shaper's output; state carried"""
        x = np.asarray(x, dtype=np.float64)
        y_out = np.empty_like(x)
        c, st, s, sc, inv = self.coef, self.state, self.rng, self.scale, self.inv
        max_v, lim = 1.0 - (1.0 / inv), 2.0 * sc
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(x.shape[1]):
                xi = x[:, i] * headroom
                p = [_fma_rows(st[4 + j], c[4 + j], st[j] * c[j]) for j in range(4)]
                fb = ((p[0] + p[2]) + (p[1] + p[3])) + st[8] * c[8]
                y = xi + fb
                v = np.where(y < -1.0, -1.0, np.where(y > max_v, max_v, y))
                u1 = _uniform(s)
                u2 = _uniform(s)
                v = v + (u1 + u2 - 1.0) * sc
                q = np.rint(v * inv)
                yq = np.where(q < -inv, -inv, np.where(inv - 1.0 < q, inv - 1.0, q)) * sc
                err = yq - y
                err = np.where(np.isfinite(err), err, 0.0)
                f = np.where(err < -lim, -lim, np.where(lim < err, lim, err))
                for k in range(ORDER):
                    b = st[k].copy()
                    nf = f + c[k] * b
                    nb = c[k] * f + b
                    st[k] = np.where(nb < -2.0, -2.0, np.where(2.0 < nb, 2.0, nb))
                    f = nf
                y_out[:, i] = yq
        return scrub(y_out) if scrubbed else y_out
