"""numpy restatement of the packed PCM conversions of include/convopeq_mi355x.h ("packed PCM in and out") and nothing else.
Formats and layouts by their C values: F64 0, F32 1, S16 2, S24 3 (packed little-endian), S32 4; planar 0 ([2 S][n]),
interleaved 1 ([S][n][2])."""
import numpy as np

F64, F32, S16, S24, S32 = 0, 1, 2, 3, 4
PLANAR, INTERLEAVED = 0, 1
BYTES = {F64: 8, F32: 4, S16: 2, S24: 3, S32: 4}
DTYPE = {F64: np.float64, F32: np.float32, S16: np.int16, S32: np.int32}


def s24_to_bytes(codes):
    """int array of 24-bit codes (-2^23 .. 2^23 - 1) -> uint8 [..., 3], little-endian"""
    u = np.asarray(codes).astype(np.int64) & 0xFFFFFF
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)


def s24_from_bytes(b):
    """uint8 [..., 3] -> int32 codes, sign-extended"""
    b = np.asarray(b, dtype=np.uint8).astype(np.int64)
    u = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return (u - ((u & 0x800000) << 1)).astype(np.int32)


def decode(samples, fmt):
    """samples: array of the format's dtype (S24: int codes) -> float64, the widened input"""
    if fmt == F64:
        return np.asarray(samples, dtype=np.float64).copy()
    if fmt == F32:
        return np.asarray(samples, dtype=np.float32).astype(np.float64)
    shift = {S16: 16, S24: 8, S32: 0}[fmt]
    fixed = (np.asarray(samples).astype(np.int64) << shift).astype(np.int32)          # left-justified to 32 bits
    k = np.float32(1.0) / np.float32(0x7fffffff)                                      # float(0x7fffffff) = 2^31
    return (fixed.astype(np.float32) * k).astype(np.float64)                          # int -> float rounds to nearest


def sanitize(rows, cb):
    """applyHighQuality64BitTransform(gain 1) per callback of cb samples along the last axis (the last callback of a row may be
    shorter): NaN and |v| < 1e-20 -> +0.0, clamp to [-1, 1]; an infinity clamps in the 4-wide body of a callback and is 0 in
    its scalar tail, the last len % 4 samples."""
    v = np.array(rows, dtype=np.float64)
    n = v.shape[-1]
    i = np.arange(n)
    start = i // cb * cb
    length = np.minimum(cb, n - start)
    tail = (i - start) >= length // 4 * 4
    with np.errstate(invalid="ignore"):
        zero = np.isnan(v) | (np.abs(v) < 1.0e-20) | (np.isinf(v) & tail)
    v[zero] = 0.0
    return np.minimum(1.0, np.maximum(-1.0, v))


def encode(rows, fmt):
    """float64 -> the format's dtype (S24: int32 codes)"""
    x = np.asarray(rows, dtype=np.float64)
    if fmt == F64:
        return x.copy()
    if fmt == F32:
        with np.errstate(over="ignore", invalid="ignore"):
            return x.astype(np.float32)
    bits = {S24: 24, S32: 32}[fmt]                   # no 16-bit output
    scale = float(1 << (bits - 1))
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.rint(x * scale)                       # ties to even
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(v, -scale, scale - 1.0).astype(np.int64).astype(np.int32)


def to_layout(a, layout):
    """[2 S][n] in sample units -> the packed order"""
    if layout == PLANAR:
        return np.ascontiguousarray(a)
    c, n = a.shape
    return np.ascontiguousarray(a.reshape(c // 2, 2, n).transpose(0, 2, 1))


def from_layout(a, layout, channels, n):
    if layout == PLANAR:
        return np.ascontiguousarray(a).reshape(channels, n)
    return np.ascontiguousarray(a.reshape(channels // 2, n, 2).transpose(0, 2, 1)).reshape(channels, n)


def to_bytes(samples, fmt, layout):
    """[2 S][n] of the format's dtype (S24: codes) -> the packed buffer as uint8"""
    a = to_layout(np.asarray(samples), layout)
    if fmt == S24:
        return s24_to_bytes(a).reshape(-1)
    return np.ascontiguousarray(a.astype(DTYPE[fmt], copy=False)).view(np.uint8).reshape(-1)


def from_bytes(buf, fmt, layout, channels, n):
    """the packed buffer (uint8) -> [2 S][n] of the format's dtype (S24: codes)"""
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    a = s24_from_bytes(buf.reshape(-1, 3)) if fmt == S24 else buf.view(DTYPE[fmt])
    return from_layout(a, layout, channels, n)
