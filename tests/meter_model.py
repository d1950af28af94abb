"""numpy restatement of the two meters DSPCore runs on its final block (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:
695-701), written from the reference text and independent of the C++ port:

  LoudnessMeter (src/LoudnessMeter.{h,cpp}): updateCoefficients, the two Direct-Form-I biquads in series, mean square and
  peak per callback, blockCounter and the ring of 4096 that drops what finds it full;
  TruePeakDetector (src/TruePeakDetector.{h,cpp}): prepareStage for 63 and 31 taps at 100 dB, interpolateStage to the
  letter, the max over both channels and the decaying hold.

Both reference files include JuceHeader.h and cannot be compiled stand-alone, so parity with them is by restatement only.

Two properties of interpolateStage that are the reference's and are kept (TruePeakDetector.cpp, interpolateStage):
  * its window reaches 16 samples past the output's own sample; at the end of a callback it reads the pad of the history
    buffer that no call ever writes -- zeros, as long as every callback has the same length.  A callback therefore sees
    zeros where the next callback's first samples will be: the result is NOT that of a continuous stream;
  * it is not a textbook polyphase interpolator (both branches carry the 0.5 centre tap and the same FIR branch).
Callbacks of varying length make the history shift land on stale memory; that case is not modelled.

Every sample is read as 0 when it is not finite or |v| >= 1e300 (the scrub at DSPCoreDouble.cpp:665-693)."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

RING = 4096
U = 2.0 ** -53


def scrub(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x) & (np.abs(x) < 1.0e300), x, 0.0)


# ---------------------------------------------------------------------------------------------------------- loudness
def kweighting(fs):
    """updateCoefficients(fs): (pre[5], rlb[5]) = {b0, b1, b2, a1, a2} / a0, in the reference's operation order"""
    w0 = 2.0 * math.pi * 38.0 / fs
    cos_w0, sin_w0 = math.cos(w0), math.sin(w0)
    alpha = sin_w0 / (2.0 * 0.50)
    b0 = (1.0 + cos_w0) / 2.0
    b1 = -(1.0 + cos_w0)
    b2 = (1.0 + cos_w0) / 2.0
    a0 = 1.0 + alpha
    a1 = -2.0 * cos_w0
    a2 = 1.0 - alpha
    inv = 1.0 / a0
    rlb = np.array([b0 * inv, b1 * inv, b2 * inv, a1 * inv, a2 * inv])
    w0 = 2.0 * math.pi * 1500.0 / fs
    cos_w0, sin_w0 = math.cos(w0), math.sin(w0)
    A = math.pow(10.0, 4.0 / 40.0)
    alpha = sin_w0 / (2.0 * 0.7071067811865476)
    sqrt_a = math.sqrt(A)
    b0 = A * ((A + 1.0) + (A - 1.0) * cos_w0 + 2.0 * sqrt_a * alpha)
    b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cos_w0)
    b2 = A * ((A + 1.0) + (A - 1.0) * cos_w0 - 2.0 * sqrt_a * alpha)
    a0 = (A + 1.0) - (A - 1.0) * cos_w0 + 2.0 * sqrt_a * alpha
    a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cos_w0)
    a2 = (A + 1.0) - (A - 1.0) * cos_w0 - 2.0 * sqrt_a * alpha
    inv = 1.0 / a0
    pre = np.array([b0 * inv, b1 * inv, b2 * inv, a1 * inv, a2 * inv])
    return pre, rlb


class Biquad:
    """processKWeightingStage for a batch of rows: y = b0 x + b1 x1 + b2 x2 - a1 y1 - a2 y2, state carried"""

    def __init__(self, coef, rows, dtype):
        self.c = [dtype(v) for v in coef]
        self.x1 = np.zeros(rows, dtype)
        self.x2 = np.zeros(rows, dtype)
        self.y1 = np.zeros(rows, dtype)
        self.y2 = np.zeros(rows, dtype)

    def run(self, x):
        b0, b1, b2, a1, a2 = self.c
        n = x.shape[1]
        xm1 = np.concatenate([self.x1[:, None], x[:, :-1]], axis=1)
        xm2 = np.concatenate([self.x2[:, None], self.x1[:, None], x[:, :-2]], axis=1)[:, :n]
        f = b0 * x + b1 * xm1 + b2 * xm2            # the same three products and two sums as the sequential form
        y = np.empty_like(x)
        y1, y2 = self.y1, self.y2
        for i in range(n):
            v = f[:, i] - a1 * y1 - a2 * y2
            y[:, i] = v
            y2, y1 = y1, v
        self.y1, self.y2 = y1, y2
        ext = np.concatenate([self.x2[:, None], self.x1[:, None], x], axis=1)
        self.x1, self.x2 = ext[:, -1].copy(), ext[:, -2].copy()
        return y


class LoudnessMeter:
    """LoudnessMeter for `streams` stereo streams at once (rows 2 s, 2 s + 1); dtype = the arithmetic of the filters"""

    def __init__(self, fs, streams=1, dtype=np.float64):
        self.dtype = dtype
        self.streams = streams
        self.pre_c, self.rlb_c = kweighting(fs)
        self.reset()

    def reset(self):
        self.pre = Biquad(self.pre_c, 2 * self.streams, self.dtype)
        self.rlb = Biquad(self.rlb_c, 2 * self.streams, self.dtype)
        self.counter = 0

    def weighted(self, x):
        return self.rlb.run(self.pre.run(scrub(x).astype(self.dtype)))

    def process_block(self, x):
        """one callback, x [2 streams, n] -> (mean_square [streams], peak_linear [streams], block_index)"""
        y = self.weighted(x)
        n = x.shape[1]
        ss = (y * y).sum(axis=1)
        ms = (ss[0::2] * self.dtype(1.0) + ss[1::2] * self.dtype(1.0)) / self.dtype(n)
        pk = np.abs(y).max(axis=1)
        idx = self.counter
        self.counter += 1
        return ms, np.maximum(pk[0::2], pk[1::2]), idx

    def process(self, x, callback):
        """a call cut into callbacks (the last may be short): lists of the per-callback results"""
        return [self.process_block(x[:, o:o + callback]) for o in range(0, x.shape[1], callback)]


class Ring:
    """LockFreeRingBuffer<BlockPower, 4096>: push drops on full, pop takes the oldest"""

    def __init__(self):
        self.w = self.r = 0
        self.buf = [None] * RING

    def push(self, item):
        if self.w - self.r >= RING:
            return False
        self.buf[self.w % RING] = item
        self.w += 1
        return True

    def pop(self):
        if self.r == self.w:
            return None
        item = self.buf[self.r % RING]
        self.r += 1
        return item


# --------------------------------------------------------------------------------------------------------- true peak
def bessel_i0(x):
    s, term, xx = 1.0, 1.0, x * x
    for n in range(1, 100):
        term *= xx / (4.0 * float(n) * float(n))
        s += term
        if term < s * 1.0e-18:
            break
    return s


def design_stage(taps_in, atten=100.0):
    """prepareStage(stage, taps, attenuationDb, .) in the reference's operation order"""
    taps = max(3, taps_in | 1)
    ct = (taps - 1) // 2
    cpar = ct & 1
    vpar = 1 - cpar
    if atten > 50.0:
        beta = 0.1102 * (atten - 8.7)
    elif atten >= 21.0:
        beta = 0.5842 * (atten - 21.0) ** 0.4 + 0.07886 * (atten - 21.0)
    else:
        beta = 0.0
    i0b = bessel_i0(beta)
    raw = [0.0] * taps
    for n in range(taps):
        t = float(n - ct)
        sinc = 0.5 if n == ct else math.sin(math.pi * 0.5 * t) / (math.pi * t)
        frac = float(n - ct) / float(ct)
        raw[n] = sinc * (bessel_i0(beta * math.sqrt(max(0.0, 1.0 - frac * frac))) / i0b)
    for n in range(taps):
        if n != ct and (n & 1) == cpar:
            raw[n] = 0.0
    s = 0.0
    for v in raw:
        s += v
    if abs(s) > 1e-20:
        inv = 1.0 / s
        raw = [v * inv for v in raw]
    raw[ct] = 0.5
    ncs = 0.0
    for i, v in enumerate(raw):
        if i != ct:
            ncs += v
    if abs(ncs) > 1e-20:
        sc = 0.5 / ncs
        raw = [v if i == ct else v * sc for i, v in enumerate(raw)]
    raw[ct] = 0.5
    cc = (taps - vpar + 1) // 2
    conv = np.array([raw[vpar + 2 * r] if vpar + 2 * r < taps else 0.0 for r in range(cc)])
    cdi = (ct - cpar) // 2
    return dict(taps=taps, center_tap=ct, center_parity=cpar, conv_parity=vpar, conv_count=cc, center_delay_input=cdi,
                history_up_keep=max(cc - 1, cdi), attenuation_db=atten, center_coeff=raw[ct], raw=np.array(raw), conv=conv,
                rev=conv[::-1].copy())


def tp_stages():
    """TruePeakDetector::prepare(rate, maxBlock, taps = 63): stage 0 = 63 taps, stage 1 = max(15, 63 / 2) | 1 = 31"""
    return [design_stage(63), design_stage(max(15, 63 // 2))]


def gamma(n):
    g = n * U / (1.0 - n * U)
    return g * (1.0 + 2.0 * g)


def interpolate(st, hist, x, dhist=None, dx=None, future=None, dtype=np.longdouble):
    """interpolateStage for one channel: hist = the stage's history (history_up_keep values), x = the callback.
    Returns (out [2 n] in dtype, new history, E [2 n], new history's error): E bounds what any fp64 evaluation of the same
    sums may differ from the exact value by -- gamma(C + 1) * sum |c| (|x| + d) + sum |c| d, d = the operands' own error
    (tests/os_exact.py).  future: what stands after the callback instead of the reference's 16 zeros (for the test that
    shows the difference)."""
    H, C, cd, p = st["history_up_keep"], st["conv_count"], st["center_delay_input"], st["conv_parity"]
    n = len(x)
    pad = np.zeros(16) if future is None else np.asarray(future, dtype=np.float64)[:16]
    pad = np.concatenate([pad, np.zeros(16 - len(pad))])
    e = np.concatenate([hist, x, pad])
    d = np.concatenate([np.zeros(H) if dhist is None else dhist, np.zeros(n) if dx is None else dx, np.zeros(16)])
    rev = st["rev"].astype(dtype)
    arev = np.abs(st["rev"])
    ew = sliding_window_view(e.astype(dtype), C)
    mw = sliding_window_view(np.abs(e) + d, C)
    dw = sliding_window_view(d, C)
    base = H - cd + np.arange(n)                    # index of base[0] in e
    out = np.empty(2 * n, dtype)
    E = np.empty(2 * n)
    g = gamma(C + 1)
    for q, (ci, wi) in enumerate(((base, base - p), (base + 1, base - 1 + p))):
        out[q::2] = e[ci].astype(dtype) * dtype(st["center_coeff"]) + ew[wi] @ rev
        mag = mw[wi] @ arev + 0.5 * (np.abs(e[ci]) + d[ci])
        dsum = dw[wi] @ arev + 0.5 * d[ci]
        E[q::2] = g * mag + dsum * (1.0 + 2.0 * g)
    keep = np.concatenate([hist, x])[-H:]
    dkeep = np.concatenate([np.zeros(H) if dhist is None else dhist, np.zeros(n) if dx is None else dx])[-H:]
    return out, keep, E, dkeep


class TruePeakDetector:
    """one stereo instance; process_block(x [2, n]) -> (true_peak, hold, bound on |an fp64 kernel's true_peak - ours|)"""

    def __init__(self, dtype=np.longdouble):
        self.dtype = dtype
        self.st = tp_stages()
        self.reset()

    def reset(self):
        self.hist = [[np.zeros(s["history_up_keep"]) for _ in range(2)] for s in self.st]
        self.dhist = [[np.zeros(s["history_up_keep"]) for _ in range(2)] for s in self.st]
        self.hold = 0.0

    def process_block(self, x):
        x = scrub(x)
        peak, bound = 0.0, 0.0
        for ch in range(2):
            o0, self.hist[0][ch], e0, self.dhist[0][ch] = interpolate(self.st[0], self.hist[0][ch], x[ch], self.dhist[0][ch],
                                                                    None, dtype=self.dtype)
            f = o0.astype(np.float64)                       # the stage hands fp64 samples on
            d0 = e0 + np.abs((o0 - f.astype(self.dtype)).astype(np.float64))
            o1, self.hist[1][ch], e1, self.dhist[1][ch] = interpolate(self.st[1], self.hist[1][ch], f, self.dhist[1][ch], d0,
                                                                    dtype=self.dtype)
            peak = max(peak, float(np.abs(o1).max()))
            bound = max(bound, float(e1.max()))
        tp = float(np.float64(peak))
        self.hold = tp if tp > self.hold else self.hold * 0.999
        return tp, self.hold, bound


def hold_replay(peaks, hold=0.0):
    out = []
    for p in peaks:
        hold = p if p > hold else hold * 0.999
        out.append(hold)
    return out
