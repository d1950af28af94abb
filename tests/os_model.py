"""numpy restatement of CustomInputOversampler (src/CustomInputOversampler.cpp), written from the reference text and
independent of the C++ port: prepareStage (:287-390), interpolateStage (:492-568, the shipped AVX2 branch),
decimateStage (:570-723) and the processDown state machine (:785-872) of one stereo instance.

Documented deviation of the product, reproduced here: a stream in hard fallback outputs silence and does not advance."""
import math

import numpy as np

IIR, LINEAR_PHASE = 0, 1
TAPS = {IIR: (511, 127, 31), LINEAR_PHASE: (1023, 255, 63)}
ATTEN = {IIR: (140.0, 110.0, 90.0), LINEAR_PHASE: (160.0, 140.0, 120.0)}
DENORM = 1.0e-20
HARD_FALLBACK_THRESHOLD = 4


def bessel_i0(x):
    s, term, xx = 1.0, 1.0, x * x
    for n in range(1, 100):
        term *= xx / (4.0 * float(n) * float(n))
        s += term
        if term < s * 1.0e-18:
            break
    return s


def design_stage(stage, os_type=IIR):
    taps = max(3, TAPS[os_type][stage] | 1)
    atten = ATTEN[os_type][stage]
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
    conv_count = (taps - vpar + 1) // 2
    conv = np.array([raw[vpar + 2 * r] if vpar + 2 * r < taps else 0.0 for r in range(conv_count)])
    cdi = (ct - cpar) // 2
    return dict(taps=taps, center_tap=ct, center_parity=cpar, conv_parity=vpar, conv_count=conv_count,
                center_delay_input=cdi, history_up_keep=max(conv_count - 1, cdi),
                history_down_keep=max(ct, vpar + 2 * (conv_count - 1) + 6), attenuation_db=atten, center_coeff=raw[ct],
                raw=np.array(raw), conv=conv)


def is_bad(v):
    """isBadSample: non-finite or |v| > 2^53 (element-wise)"""
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(v) | (np.abs(v) > 2.0 ** 53)


def _fir(ext, c, first, n):
    """sum_r c[r] * ext[first + i - r] for i < n"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.convolve(ext, c)[first:first + n]


class Oversampler:
    """One CustomInputOversampler instance (one stereo stream, two channels sharing the corruption flag)."""

    def __init__(self, factor, os_type=IIR):
        self.factor = factor
        self.stages = [design_stage(i, os_type) for i in range({1: 0, 2: 1, 4: 2, 8: 3}[factor])]
        self.events = 0
        self.auto_clears = 0
        self.silent_paths = 0                       # decimator calls that took the silence path (channels x stages)
        self.silent_discards = 0                    # ... of those, the ones whose input or history held a non-zero value
        self.reset()

    def reset(self):
        self.up_hist = [np.zeros((2, s["history_up_keep"])) for s in self.stages]
        self.down_hist = [np.zeros((2, s["history_down_keep"])) for s in self.stages]
        self.flag = False
        self.consecutive = 0
        self.hard = False

    def _interp(self, i, ch, x):
        st = self.stages[i]
        keep, n = st["history_up_keep"], len(x)
        ext = np.concatenate([self.up_hist[i][ch], x])
        conv = _fir(ext, st["conv"], keep, n)
        with np.errstate(invalid="ignore", over="ignore"):
            conv = np.where(is_bad(conv) | (np.abs(conv) < DENORM), 0.0, conv)
            cen = st["center_coeff"] * ext[keep - st["center_delay_input"]:keep - st["center_delay_input"] + n]
        bad = is_bad(cen)
        self.events += int(bad.sum())
        if bad.any():
            self.flag = True
        conv = conv * 2.0
        conv = np.where(np.abs(conv) < DENORM, 0.0, conv)
        with np.errstate(invalid="ignore"):
            cen = np.where(np.abs(cen) < DENORM, 0.0, cen)
        out = np.empty(2 * n)
        out[0::2] = np.where(bad, 0.0, conv)
        out[1::2] = np.where(bad, 0.0, cen)
        self.up_hist[i][ch] = ext[len(ext) - keep:]
        return out

    def _decim(self, i, ch, x):
        st = self.stages[i]
        keep, m = st["history_down_keep"], len(x)
        n = m // 2
        hist = self.down_hist[i][ch]
        with np.errstate(invalid="ignore"):
            if not np.any(np.abs(x) > DENORM) and not np.any(np.abs(hist) > DENORM):
                self.silent_discards += int(np.any(x != 0.0) or np.any(hist != 0.0))
                self.down_hist[i][ch] = np.zeros(keep)
                self.silent_paths += 1
                return np.zeros(n)
        ext = np.concatenate([hist, x])
        assert keep % 2 == 0 and st["conv_parity"] == 0
        dot = _fir(ext[0::2], st["conv"], keep // 2, n)
        ci = keep + 2 * np.arange(n) - st["center_tap"]
        with np.errstate(invalid="ignore", over="ignore"):
            cen = st["center_coeff"] * ext[ci]
            acc = cen + dot
        bad_c = is_bad(cen)
        bad = bad_c | is_bad(acc)
        self.events += int(bad.sum())
        if bad.any():
            self.flag = True
        with np.errstate(invalid="ignore"):
            out = np.where(bad, 0.0, np.where(np.abs(acc) < DENORM, 0.0, acc))
        self.down_hist[i][ch] = ext[len(ext) - keep:]
        return out

    def up(self, x):
        """processUp: x [2, n] -> [2, n * factor]"""
        x = np.asarray(x, dtype=np.float64)
        if self.hard:
            return np.zeros((2, x.shape[1] * self.factor))
        out = []
        for ch in range(2):
            y = x[ch]
            for i in range(len(self.stages)):
                y = self._interp(i, ch, y)
            out.append(y)
        return np.stack(out)

    def down(self, y):
        """processDown: y [2, n * factor] -> [2, n]"""
        y = np.asarray(y, dtype=np.float64)
        n = y.shape[1] // self.factor
        if self.hard:
            return np.zeros((2, n))
        if self.flag:
            self.flag = False
            self.auto_clears += 1
            self.consecutive += 1
            if self.consecutive >= HARD_FALLBACK_THRESHOLD:
                self.hard = True
            for h in self.up_hist + self.down_hist:
                h[:] = 0.0
            return np.zeros((2, n))
        self.consecutive = 0
        out = []
        for ch in range(2):
            v = y[ch]
            for i in reversed(range(len(self.stages))):
                v = self._decim(i, ch, v)
            out.append(v)
        return np.stack(out)


def latency(factor, os_type=IIR):
    return sum(2.0 * design_stage(i, os_type)["center_tap"] / 2 ** (i + 1) for i in range({1: 0, 2: 1, 4: 2, 8: 3}[factor]))
