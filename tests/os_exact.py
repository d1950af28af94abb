"""Exact reference of the oversampler stages: interpolateStage / decimateStage / processDown as in os_model, with every
convolution sum computed exactly and a rigorous bound on what any fp64 implementation may return.

Each product c_r x is split exactly (Dekker's two-product) and the products are summed with math.fsum, so an output is
held as hi + lo (hi = the correctly rounded sum, lo = the rounded residual).  Alongside it goes the bound

    E = gamma_C * sum_r |c_r| (|x_r| + d_r) + sum_r |c_r| d_r,   gamma_C = C u / (1 - C u), u = 2^-53,

the standard bound for a length-C fp64 dot product (any order, with or without FMA), plus the effect of input errors
d_r where the operands are themselves the outputs of an earlier stage.  The decimator's centre term 0.5 h is one more
(exact) product, so its dot has C + 1 terms.  Where a window holds at most one non-zero product and its operands are
exact, every implementation returns the same double -- fl(c_r x), or fl(cen + fl(c_r x)) at the decimator -- and the
reference holds that double with E = 0: the kernel must then be bit-equal.

Guards, flushes and the silence test are applied to hi + lo only where the decision is determined, i.e. the whole
interval [S - E, S + E] lies on one side of the threshold; `undetermined` counts the decisions that are not.  A test
input is only valid if that count stays 0.

cheap=True replaces the exact sums by the model's own np.convolve arithmetic (for sizes where fsum costs too much);
the reference value is then itself within E of the exact sum, so a kernel must be within 2 E of it, and the
decisions are judged with that 2 E."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import os_model as M

U = 2.0 ** -53
LIMIT = 2.0 ** 53                   # isBadSample: |v| > 2^53 is bad, 2^53 itself passes
D = M.DENORM                        # double(1e-20)


def gamma(n):
    return n * U / (1.0 - n * U)


def _split(a):
    t = 134217729.0 * a             # 2^27 + 1
    hi = t - (t - a)
    return hi, a - hi


def two_prod(a, b):
    """p + e == a * b exactly (no overflow or underflow in the operands used here)"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


class Val:
    """per-output reference value hi + lo and bound E (arrays of one shape)"""

    def __init__(self, hi, lo=None, E=None):
        self.hi = np.asarray(hi, dtype=np.float64)
        self.lo = np.zeros_like(self.hi) if lo is None else lo
        self.E = np.zeros_like(self.hi) if E is None else E

    @property
    def delta(self):
        """bound on |kernel value - hi|: the next stage's input error"""
        return (self.E + np.abs(self.lo)) * (1.0 + 4 * U)


def _above(v, margin, t):
    """|value| > t for values within `margin` of v: (decision, determined).  Non-finite is above."""
    with np.errstate(invalid="ignore"):
        nf = ~np.isfinite(v)
        diff = np.abs(v) - t
        above = nf | (diff > margin)
        det = above | (diff <= -margin)
    return above, det


def _below(v, margin, t):
    """|value| < t: (decision, determined).  Non-finite is not below."""
    with np.errstate(invalid="ignore"):
        nf = ~np.isfinite(v)
        diff = np.abs(v) - t
        below = ~nf & (diff < -margin)
        det = below | nf | (diff >= margin)
    return below, det


def _window_sums(ops, dops, c, first, n, cen=None, dcen=None, cheap=False):
    """S[i] = cen[i] + sum_r c[r] ops[first + i - r] (i < n) as a Val, plus the mask of windows holding a non-finite
    operand; dops bounds the operands' own errors"""
    C = len(c)
    fin = np.isfinite(ops)
    opsf = np.where(fin, ops, 0.0)
    ac = np.abs(c)
    sl = slice(first, first + n)
    nf = np.convolve((~fin).astype(np.float64), np.ones(C))[sl] > 0.5
    mag = np.convolve(np.abs(opsf) + dops, ac)[sl]
    dsum = np.convolve(dops, ac)[sl]
    terms = C
    cen_f = None
    if cen is not None:
        nf |= ~np.isfinite(cen)
        cen_f = np.where(np.isfinite(cen), cen, 0.0)
        mag += np.abs(cen_f) + dcen
        dsum += dcen
        terms += 1
    g = gamma(terms) * (1.0 + 2 * gamma(terms))
    lo = np.zeros(n)
    if cheap:
        E = 2.0 * g * mag + dsum * (1.0 + 2 * gamma(terms))      # kernel vs this fp64 reference: both within g * mag
        hi = np.convolve(opsf, c)[sl]
        if cen is not None:
            hi = cen_f + hi
        return Val(hi, lo, E), nf
    hi = np.empty(n)
    Wf = sliding_window_view(opsf, C)[first - C + 1:first - C + 1 + n][:, ::-1]
    E = g * mag + dsum * (1.0 + 2 * gamma(terms))
    nnz = np.count_nonzero(Wf, 1)
    exact = (nnz <= 1) & (dsum == 0.0)
    step = max(1, (1 << 20) // C)
    for a in range(0, n, step):
        b = min(n, a + step)
        p, e = two_prod(Wf[a:b], c[None, :])
        psum = p.sum(1)                                          # one non-zero product: exactly that product
        rows = np.concatenate([p, e], axis=1)
        if cen is not None:
            rows = np.concatenate([rows, cen_f[a:b, None]], axis=1)
        for k, row in enumerate(rows.tolist()):
            i = a + k
            if exact[i]:
                hi[i] = psum[k] if cen is None else cen_f[i] + psum[k]
                continue
            h = math.fsum(row)
            hi[i] = h
            lo[i] = math.fsum(row + [-h])
    E[exact] = 0.0
    return Val(hi, lo, E), nf


class ExactOversampler:
    """os_model.Oversampler with exact sums and bounds; up() / down() return Val arrays [2, n]."""

    def __init__(self, factor, os_type=M.IIR, cheap=False):
        self.factor = factor
        self.cheap = cheap
        self.stages = [M.design_stage(i, os_type) for i in range({1: 0, 2: 1, 4: 2, 8: 3}[factor])]
        self.events = 0
        self.auto_clears = 0
        self.silent_paths = 0
        self.undetermined = 0
        self.decisions = 0
        self.trace = []                 # (direction, stage, channel, Val of the stage output) of the last call
        self.last_silent = set()        # (stage, channel) that took the silence path in the last down call
        self.reset()

    def reset(self):
        self.up_hist = [[(np.zeros(s["history_up_keep"]), np.zeros(s["history_up_keep"])) for _ in range(2)]
                        for s in self.stages]
        self.down_hist = [[(np.zeros(s["history_down_keep"]), np.zeros(s["history_down_keep"])) for _ in range(2)]
                          for s in self.stages]
        self.flag = False
        self.consecutive = 0
        self.hard = False

    def _count(self, det, where=None):
        det = det if where is None else det[where]
        self.decisions += int(det.size)
        self.undetermined += int((~det).sum())

    def _interp(self, i, ch, x, dx):
        st = self.stages[i]
        keep, C, cdi, n = st["history_up_keep"], st["conv_count"], st["center_delay_input"], len(x)
        h, dh = self.up_hist[i][ch]
        ext, dext = np.concatenate([h, x]), np.concatenate([dh, dx])
        conv, nf = _window_sums(ext, dext, st["conv"], keep, n, cheap=self.cheap)
        mc = conv.E + np.abs(conv.lo)
        with np.errstate(invalid="ignore"):
            conv.hi = np.where(nf, np.nan, conv.hi)
        bad_conv, det = _above(conv.hi, mc, LIMIT)
        self._count(det)
        low, det = _below(conv.hi, mc, D)
        self._count(det, ~bad_conv)
        z = bad_conv | low
        conv = Val(np.where(z, 0.0, 2.0 * conv.hi), np.where(z, 0.0, 2.0 * conv.lo), np.where(z, 0.0, 2.0 * conv.E))
        cen = 0.5 * ext[keep - cdi:keep - cdi + n]
        dcen = 0.5 * dext[keep - cdi:keep - cdi + n]
        bad, det = _above(cen, dcen, LIMIT)
        self._count(det)
        self.events += int(bad.sum())
        if bad.any():
            self.flag = True
        low2, det = _below(conv.hi, conv.E + np.abs(conv.lo), D)         # cannot fire (kept sums are >= 1e-20)
        self._count(det, ~bad)
        lowc, det = _below(cen, dcen, D)
        self._count(det, ~bad)
        ze, zo = bad | low2, bad | lowc
        out = Val(np.empty(2 * n), np.zeros(2 * n), np.zeros(2 * n))
        out.hi[0::2] = np.where(ze, 0.0, conv.hi)
        out.lo[0::2] = np.where(ze, 0.0, conv.lo)
        out.E[0::2] = np.where(ze, 0.0, conv.E)
        out.hi[1::2] = np.where(zo, 0.0, cen)
        out.E[1::2] = np.where(zo, 0.0, dcen)
        self.up_hist[i][ch] = (ext[len(ext) - keep:], dext[len(ext) - keep:])
        return out

    def _decim(self, i, ch, x, dx):
        st = self.stages[i]
        keep, C, ct, m = st["history_down_keep"], st["conv_count"], st["center_tap"], len(x)
        n = m // 2
        h, dh = self.down_hist[i][ch]
        ax, dax = _above(np.concatenate([h, x]), np.concatenate([dh, dx]), D)
        with np.errstate(invalid="ignore"):
            ax &= ~np.isnan(np.concatenate([h, x]))                  # fabs(NaN) > t is false
            dax |= np.isnan(np.concatenate([h, x]))
        loud = ax.any()
        self.decisions += 1
        if not loud and not dax.all():
            self.undetermined += 1
        if not loud:
            self.down_hist[i][ch] = (np.zeros(keep), np.zeros(keep))
            self.silent_paths += 1
            self.last_silent.add((i, ch))
            return Val(np.zeros(n))
        ext, dext = np.concatenate([h, x]), np.concatenate([dh, dx])
        ci = keep + 2 * np.arange(n) - ct
        cen, dcen = st["center_coeff"] * ext[ci], st["center_coeff"] * dext[ci]
        bad_c, det = _above(cen, dcen, LIMIT)
        self._count(det)
        a, nf = _window_sums(ext[0::2], dext[0::2], st["conv"], keep // 2, n, cen, dcen, cheap=self.cheap)
        with np.errstate(invalid="ignore"):
            a.hi = np.where(nf, np.nan, a.hi)
        ma = a.E + np.abs(a.lo)
        bad_a, det = _above(a.hi, ma, LIMIT)
        self._count(det, ~bad_c)
        bad = bad_c | bad_a
        self.events += int(bad.sum())
        if bad.any():
            self.flag = True
        low, det = _below(a.hi, ma, D)
        self._count(det, ~bad)
        z = bad | low
        self.down_hist[i][ch] = (ext[len(ext) - keep:], dext[len(ext) - keep:])
        return Val(np.where(z, 0.0, a.hi), np.where(z, 0.0, a.lo), np.where(z, 0.0, a.E))

    @staticmethod
    def _stack(vals):
        return Val(np.stack([v.hi for v in vals]), np.stack([v.lo for v in vals]), np.stack([v.E for v in vals]))

    def up(self, x):
        """processUp: x [2, n] (exact inputs) -> Val [2, n * factor]"""
        x = np.asarray(x, dtype=np.float64)
        self.trace = []
        if self.hard:
            return Val(np.zeros((2, x.shape[1] * self.factor)))
        out = []
        for ch in range(2):
            v = Val(x[ch])
            for i in range(len(self.stages)):
                v = self._interp(i, ch, v.hi, v.delta)
                self.trace.append(("up", i, ch, v))
            out.append(v)
        return self._stack(out)

    def down(self, y):
        """processDown: y [2, n * factor] (exact inputs) -> Val [2, n]"""
        y = np.asarray(y, dtype=np.float64)
        self.trace = []
        self.last_silent = set()
        n = y.shape[1] // self.factor
        if self.hard:
            return Val(np.zeros((2, n)))
        if self.flag:
            self.flag = False
            self.auto_clears += 1
            self.consecutive += 1
            if self.consecutive >= M.HARD_FALLBACK_THRESHOLD:
                self.hard = True
            for st in self.up_hist + self.down_hist:
                for ch in range(2):
                    st[ch] = (np.zeros_like(st[ch][0]), np.zeros_like(st[ch][1]))
            return Val(np.zeros((2, n)))
        self.consecutive = 0
        out = []
        for ch in range(2):
            v = Val(y[ch])
            for i in reversed(range(len(self.stages))):
                v = self._decim(i, ch, v.hi, v.delta)
                self.trace.append(("down", i, ch, v))
            out.append(v)
        return self._stack(out)

    def telemetry(self):
        return (self.events, self.auto_clears, int(self.flag), int(self.hard), self.consecutive)


def model_telemetry(m):
    return (m.events, m.auto_clears, int(m.flag), int(m.hard), m.consecutive)


def gpu_telemetry(t):
    return (t["corruption_events"], t["auto_clears"], t["corruption_pending"], t["hard_fallback"],
            t["consecutive_auto_clears"])


def error_ratio(k, ref):
    """worst |k - (hi + lo)| / E over the outputs (E = 0: any difference is inf); raises on a mismatch of zeros"""
    k = np.asarray(k, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs((k - ref.hi) - ref.lo)
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / ref.E)
    return float(r.max()) if r.size else 0.0
