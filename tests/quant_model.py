"""numpy restatement of cpq_quantizer (include/convopeq_mi355x.h, "word-length reduction of delivered rows"): dither_model /
lattice_model composed with pcm_model, plus the stream's gain and the caller's pitch.  Nothing of the shapers or of the pack is
restated here.

    u  = x * gain[s]                      one rounding
    yq = the shaper's process(u, headroom 1.0, no scrub)
    b  = rint(yq * 2^(w-1)), ties to even, saturated, NaN -> 0, w = the container's width
    bytes: planar [2 S] rows of n samples, interleaved [S] rows of n stereo frames, rows `pitch` bytes apart"""
import numpy as np

import dither_model as D
import lattice_model as L
import pcm_model as P

FIXED4, FIXED15, ADAPTIVE9 = D.FIXED4, D.FIXED15, L.ADAPTIVE9
SHAPERS = (FIXED4, FIXED15, ADAPTIVE9)
S16, S24, S32 = P.S16, P.S24, P.S32
PLANAR, INTERLEAVED = P.PLANAR, P.INTERLEAVED
WIDTH = {S16: 16, S24: 24, S32: 32}
DTYPE = {S16: np.int16, S32: np.int32}


def encode(yq, fmt):
    """float64 -> codes at the container's width (int16 / int32; S24: int32 codes)"""
    return D.encode16(yq) if fmt == S16 else P.encode(yq, fmt)


def packed_shape(fmt, layout, n_streams, n):
    bps = P.BYTES[fmt]
    return (n_streams, 2 * n * bps) if layout == INTERLEAVED else (2 * n_streams, n * bps)


def to_rows(codes, fmt, layout):
    """codes [2 S][n] -> uint8 [packed rows, width]"""
    c, n = codes.shape
    r, width = packed_shape(fmt, layout, c // 2, n)
    return P.to_bytes(codes, fmt, layout).reshape(r, width)


def decode(rows, fmt, layout, n_streams):
    """uint8 [packed rows, width] -> codes [2 S][n] as int64"""
    rows = np.ascontiguousarray(rows)
    n = rows.shape[1] // (P.BYTES[fmt] * (2 if layout == INTERLEAVED else 1))
    return P.from_bytes(rows.reshape(-1), fmt, layout, 2 * n_streams, n).astype(np.int64)


class Quantizer:
    def __init__(self, rate, n_streams, shaper, bits, fmt):
        assert shaper in SHAPERS and 1 <= bits <= WIDTH[fmt]
        self.rate, self.S, self.shaper, self.bits, self.fmt = rate, n_streams, shaper, bits, fmt
        self.sh = L.Lattice(n_streams, bits) if shaper == ADAPTIVE9 else D.Dither(rate, n_streams, shaper, bits)
        self.gains = np.ones(n_streams)

    def reset(self):
        """as new: errors cleared, generators reseeded; gains and coefficients stay"""
        if self.shaper == ADAPTIVE9:
            coef = self.sh.coef
            self.sh = L.Lattice(self.S, self.bits)
            self.sh.coef = coef
        else:
            self.sh = D.Dither(self.rate, self.S, self.shaper, self.bits)

    def set_gains(self, gains):
        self.gains = np.asarray(gains, dtype=np.float64).copy()

    def set_adaptive_coeffs(self, stream, k):
        self.sh.set_coeffs(None if stream == -1 else stream, k)

    def shaped(self, x):
        """x [2 S][n] -> yq, the shaper's rows"""
        with np.errstate(invalid="ignore", over="ignore"):
            u = np.asarray(x, dtype=np.float64) * np.repeat(self.gains, 2)[:, None]
        return self.sh.process(u, 1.0)

    def process(self, x, layout=PLANAR, out=None):
        """x [2 S][n] -> uint8 [packed rows, width]; out: uint8 [packed rows, pitch], written in place up to the width"""
        rows = to_rows(encode(self.shaped(x), self.fmt), self.fmt, layout)
        if out is None:
            return rows
        out[:, :rows.shape[1]] = rows
        return out[:, :rows.shape[1]]
