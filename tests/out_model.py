"""Restatement of the output stage (convopeq_amd/csrc/out_design.cpp): the base-rate steps of DSPCore::processOutputDouble with
dither off (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:577-744), sequential, in the reference's operation order.

  DC_BLOCK   UltraHighRateDCBlocker::init(fs, 3.0) / process (src/UltraHighRateDCBlocker.h): per channel two one-pole sections,
             s = s + alpha * (x - s); x = x - s; at the end of a callback a state that is not finite or not below 1e15 becomes 0.
             killDenormal is the identity (the reference's release build).
  HEADROOM   x *= 0.8912509381337456, then: not finite or |x| >= 1e300 becomes 0
  LIMITER    SimplePeakLimiter::prepare(fs, 100.0) / processBlock (src/audioengine/SimplePeakLimiter.h), threshold
             0.8413951287507587, knee 0.108748; one envelope per stream
  CLAMP      min(max(x, -H), H) as the reference's 4-wide body computes it (a NaN becomes -H)

Python floats and numpy's elementwise operations are IEEE fp64 without contraction, so the fp64 model is bit-exact; with
dtype=np.longdouble the DC blocker runs in extended precision on the same fp64 coefficients (the yardstick of the scan's bar)."""
import math

import numpy as np

DC_BLOCK, HEADROOM, LIMITER, CLAMP, ALL = 1, 2, 4, 8, 15
H = 0.8912509381337456
THRESHOLD = 0.8413951287507587
KNEE = 0.108748
CLIP_START = THRESHOLD - KNEE * 0.5


def design(rate):
    """(alpha[2], release coefficient) with the reference's fallbacks"""
    alpha = [1.0e-6, 1.0e-6]
    if math.isfinite(rate) and rate > 0.0:
        for i, ratio in enumerate((1.0 - 0.1, 1.0 + 0.1)):
            fc = 3.0 * ratio
            omega = 2.0 * math.pi * fc / rate
            a = -math.expm1(-omega)
            if not math.isfinite(a) or a <= 0.0 or a >= 1.0:
                a = 1.0e-6
            alpha[i] = a
    release_sec = 100.0 * 0.001
    release = math.exp(-1.0 / (rate * release_sec)) if (release_sec > 0.0 and rate > 0.0) else 0.0
    return alpha, release


def _jmax(a, b):
    return np.where(a < b, b, a)


def desired_gain(l, r):
    """SimplePeakLimiter's desiredGain of stereo samples (arrays)"""
    l, r = np.asarray(l, dtype=np.float64), np.asarray(r, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        peak = _jmax(np.abs(l), np.abs(r))
        sp = _jmax(peak, 1.0e-12)
        t = (sp - CLIP_START) / KNEE
        shape = t * t * (3.0 - 2.0 * t)
        knee = 1.0 - (1.0 - THRESHOLD / sp) * shape
        hard = THRESHOLD / sp
        return np.where(sp > CLIP_START, np.where(sp <= THRESHOLD, knee, hard), 1.0)


def envelope_run(d, env, release):
    """the envelope after every sample of d, from env"""
    out = np.empty(len(d))
    for i, di in enumerate(d.tolist()):
        env = di if di < env else 1.0 + (env - 1.0) * release
        out[i] = env
    return out, env


def scrub(v):
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(v) < 1.0e300, v, 0.0)


def clamp(v):
    with np.errstate(invalid="ignore"):
        t = np.where(v > -H, v, -H)
        return np.where(t < H, t, H)


def dc_block(x, alpha, state, dtype=np.float64):
    """one callback of one channel; returns (y, state after the callback's guard)"""
    if dtype is np.float64:
        s0, s1, a0, a1 = float(state[0]), float(state[1]), float(alpha[0]), float(alpha[1])
        seq = x.tolist()
    else:
        s0, s1, a0, a1 = dtype(state[0]), dtype(state[1]), dtype(alpha[0]), dtype(alpha[1])
        seq = x.astype(dtype)
    y = np.empty(len(x), dtype=dtype)
    for i, v in enumerate(seq):
        s0 = s0 + a0 * (v - s0)
        v = v - s0
        s1 = s1 + a1 * (v - s1)
        v = v - s1
        y[i] = v
    keep = lambda s: s if (math.isfinite(float(s)) and abs(float(s)) < 1.0e15) else type(s)(0.0)
    return y, [keep(s0), keep(s1)]


class OutStage:
    def __init__(self, rate, n_streams, dtype=np.float64):
        self.alpha, self.release = design(rate)
        self.S, self.dtype = n_streams, dtype
        self.reset()

    def reset(self):
        self.dc = [[0.0, 0.0] for _ in range(2 * self.S)]
        self.env = [1.0] * self.S

    def process(self, x, cb, flags=ALL):
        """x [2 S, n]: one call, callbacks of cb samples (the last one shorter when n is no multiple)"""
        y = np.array(x, dtype=self.dtype)
        n = y.shape[1]
        for o in range(0, n, cb):
            blk = y[:, o:min(o + cb, n)]
            if flags & DC_BLOCK:
                for ch in range(2 * self.S):
                    blk[ch], self.dc[ch] = dc_block(blk[ch], self.alpha, self.dc[ch], self.dtype)
            if flags & HEADROOM:
                blk[:] = scrub(blk * self.dtype(H))
            if flags & LIMITER:
                for s in range(self.S):
                    g, self.env[s] = envelope_run(desired_gain(blk[2 * s], blk[2 * s + 1]), self.env[s], self.release)
                    blk[2 * s] = blk[2 * s] * g
                    blk[2 * s + 1] = blk[2 * s + 1] * g
            if flags & CLAMP:
                blk[:] = clamp(blk)
        return y
