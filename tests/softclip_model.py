"""numpy model of DSPCore's soft clipper (softClipBlockAVX2 / musicalSoftClipScalar,
src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:107-224), both arithmetic paths, bit for bit.

A callback of len samples takes its first len // 4 * 4 samples through the 4-wide body and the rest through the scalar tail:
  body   reciprocals of the knee, t clamped to [0, 1] by max_pd / min_pd, ks = t^2 * fnmadd(2, t, 3), the Pade tanh on an
         argument clamped to +-4.5, clipped = fma(knee, tanh, threshold), mixed = fma(clipped - |x|, ks, |x|), the result selected
         over x where |x| > threshold - knee (an ordered compare: a NaN passes)
  tail   true divisions, nothing fused, the knee shape only below threshold + knee, tanh = 1 from 4.5 on
The three fused operations are libm's fma, element by element; everything else is numpy's fp64, which rounds every operation.
An infinity becomes a NaN on both paths (inf - inf in the body's mix, inf * 0 in the tail's); NaNs are compared as NaNs, not by
payload: x86 and the GPU give the default NaN opposite signs."""
import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma = np.frompyfunc(_libm.fma, 3, 1)


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), b, c)
    return _fma(a, b, c).astype(np.float64) if a.size else np.zeros(a.shape)


def params(amount):
    """(threshold, knee, asymmetry) of a saturation amount, a float32 widened as the reference widens it"""
    sat = float(np.float32(amount))
    return 0.95 - 0.45 * sat, 0.05 + 0.35 * sat, 0.10 * sat


def _pade(a):
    a2 = a * a
    return a * (10395.0 + a2 * (1260.0 + a2 * 21.0)) / (10395.0 + a2 * (4725.0 + a2 * (210.0 + a2)))


def body(x, amount):
    thr, knee, asym = params(amount)
    x = np.asarray(x, dtype=np.float64)
    y = x.copy()
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        start = thr - knee
        m = ax > start                                  # False for a NaN
        v, av = x[m], ax[m]
        sign = np.where(v > 0.0, 1.0, -1.0)
        t = (av - start) * (1.0 / (2.0 * knee))
        t = np.where(t > 0.0, t, 0.0)
        t = np.where(t < 1.0, t, 1.0)
        ks = (t * t) * fma(-2.0, t, 3.0)
        a = (av - thr) * (1.0 / knee)
        a = np.where(a > -4.5, a, -4.5)
        a = np.where(a < 4.5, a, 4.5)
        clipped = fma(knee, _pade(a), thr)
        mixed = fma(clipped - av, ks, av)
        factor = asym * (1.0 - sign) * 0.5 * ks
        y[m] = sign * (mixed * (1.0 - factor))
    return y


def tail(x, amount):
    thr, knee, asym = params(amount)
    x = np.asarray(x, dtype=np.float64)
    y = x.copy()
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        start = thr - knee
        m = ax > start
        v, av = x[m], ax[m]
        sign = np.where(v > 0.0, 1.0, -1.0)
        t = (av - start) / (2.0 * knee)
        ks = np.where(av < thr + knee, t * t * (3.0 - 2.0 * t), 1.0)
        a = (av - thr) / knee
        th = np.where(a >= 4.5, 1.0, np.where(a <= -4.5, -1.0, _pade(a)))
        clipped = thr + knee * th
        gain = 1.0 - asym * (1.0 - sign) * 0.5 * ks
        y[m] = sign * (av * (1.0 - ks) + clipped * ks) * gain
    return y


def tail_mask(n, cb):
    """True where a sample of a row of n samples, walked in callbacks of cb (the last one shorter), takes the scalar tail"""
    i = np.arange(n)
    start = i - i % cb
    length = np.minimum(cb, n - start)
    return i % cb >= length // 4 * 4


def clip(x, cb, amount):
    """one row through the block walk"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(tail_mask(x.size, cb), tail(x, amount), body(x, amount))


def clip_rows(rows, cb, amounts, on=None):
    """rows [2 S][n]; stream s clips with amounts[s] unless on[s] is false"""
    rows = np.asarray(rows, dtype=np.float64)
    out = rows.copy()
    for c in range(rows.shape[0]):
        if on is None or on[c // 2]:
            out[c] = clip(rows[c], cb, amounts[c // 2])
    return out


def same(a, b):
    """bit for bit, a NaN matching any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))
