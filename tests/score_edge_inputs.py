"""The edge inputs of the scorer's spectrum kernel (tests/golden/make_score_edges_ref.py records the reference's verdict on them,
tests/test_score_edges_cpu.py and tests/test_gpu_score_kernels.py read it): error-row pairs [2, 4096] and, for some, a masking
threshold array [2049].  Every sample is the same bits on every machine: zeros, powers of two, the project's counter noise
(integer hash, one multiplication), or a designed spectrum laid down with an integer cosine table -- round(2^26 cos(2 pi j / 4096))
from a Taylor series in 160-bit fixed point, Python integers only -- as sum_k amp_k T[(k n + phase_k) mod 4096], an int64 below
2^53, times a power of two.  A component of amplitude `a` at bin 0 < k < 2048 has |X[k]| = a * 2^26 * 2048 * scale up to the
table's rounding (about -160 dB).

CASES: name -> (rate, rows(), thr() or None, what it is for).  cases(rate) lists the names of one rate in recording order."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_dither_ref import splitmix_noise  # noqa: E402

LEN, BINS = 4096, 2049
_PI_E75 = 3141592653589793238462643383279502884197169399375105820974944592307816406286       # floor(pi * 10^75)
_F = 1 << 160
_T_BITS = 26


def _cos_fixed(x):
    """cos of the fixed-point angle x (0 <= x <= pi / 2) by its Taylor series, integers only"""
    x2 = x * x // _F
    term, total, k = _F, _F, 0
    while term:
        k += 2
        term = -(term * x2 // (_F * (k - 1) * k))
        total += term
    return total


def _table():
    pi = _PI_E75 * _F // 10 ** 75
    quarter = [(_cos_fixed(pi * j // 2048) + (1 << (160 - _T_BITS - 1))) >> (160 - _T_BITS) for j in range(1025)]
    quarter[1024] = 0
    t = np.empty(LEN, dtype=np.int64)
    for j in range(LEN):
        m = j if j <= 2048 else LEN - j
        t[j] = quarter[m] if m <= 1024 else -quarter[2048 - m]
    return t


_T = None


def _hash(seed, k):
    x = ((seed << 32) ^ k) + 0x9E3779B97F4A7C15 & (1 << 64) - 1
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (1 << 64) - 1
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (1 << 64) - 1
    return x ^ (x >> 31)


def phase(seed, k):
    return _hash(seed, k) & (LEN - 1)


def synth(amps, seed, shift):
    """one row: amps {bin: integer amplitude}, phases from the integer hash of (seed, bin), scaled by 2^-(26 + shift)"""
    global _T
    if _T is None:
        _T = _table()
    n = np.arange(LEN, dtype=np.int64)
    acc = np.zeros(LEN, dtype=np.int64)
    for k, a in amps.items():
        if a:
            acc += int(a) * _T[(k * n + phase(seed, k)) & (LEN - 1)]
    assert int(np.abs(acc).max()) < 1 << 53
    return acc.astype(np.float64) * 2.0 ** -(_T_BITS + shift)


def pair(amps, seed, shift=30):
    """both rows from one amplitude design, different phases"""
    return np.stack([synth(amps, 2 * seed, shift), synth(amps, 2 * seed + 1, shift)])


def flat(level, lo=0, hi=BINS):
    return {k: level for k in range(lo, hi)}


def noise(stream, scale=2.0 ** -12):
    return np.stack([splitmix_noise(LEN, stream, ch) * scale for ch in range(2)])


def comb_bins(rng_bins, first=3, gap=0, keep=None):
    """greedy comb from `first`: the next peak is the first bin further than max(range[i], range[j]) + gap from the last; keep(bin)
    thins it"""
    out, last = [], None
    for i in range(first, BINS - 3):
        if keep is not None and not keep(i):
            continue
        if last is None or i - last > max(int(rng_bins[i]), int(rng_bins[last])) + gap:
            out.append(i)
            last = i
    return out


def cap_search(rate):
    """the largest number of masker candidates (tonal maskers plus Bark bands that keep an unabsorbed bin) a comb placement
    reaches on the tables of `rate`, by a bounded search: bands left to right, in every band the comb either runs on at its
    closest spacing (the band is absorbed) or one gap is widened, by 1 .. 24 bins at every possible peak, until a bin of the band
    stays free; of a band's placements the one with most candidates so far is kept, the earlier last peak on a tie.  Counts on the
    tables alone (peaks 40 dB over a flat floor decide every test clearly).  -> (candidates, peak bins)"""
    import score_model as M
    t = M.Tables(rate)

    def absorbed(peaks):
        c = np.zeros(BINS, dtype=bool)
        for p in peaks:
            j = np.arange(max(0, p - 8), min(BINS - 1, p + 8) + 1)
            c[j[np.abs(t.bark[j] - t.bark[p]) <= 0.5]] = True
        return c

    def extend(peaks, upto, widen_at=None, extra=0):
        """greedy peaks up to bin `upto` (exclusive); the gap in front of the widen_at-th new peak is `extra` bins longer"""
        peaks = list(peaks)
        i = peaks[-1] + 1 if peaks else 3
        new = 0
        while i < min(upto, BINS - 3):
            last = peaks[-1] if peaks else None
            need = 0 if last is None else max(int(t.range[i]), int(t.range[last])) + (extra if new == widen_at else 0)
            if last is None or i - last > need:
                peaks.append(i)
                new += 1
            i += 1
        return peaks

    def count(peaks, upto_band):
        c = absorbed(peaks)
        return len(peaks) + sum(1 for b in range(upto_band + 1) if (~c[t.band == b]).any())

    peaks = []
    for band in range(24):
        end = int(np.nonzero(t.band == band)[0][-1]) + 1
        best = None
        for widen_at in [None] + list(range(0, 12)):
            for extra in ([0] if widen_at is None else range(1, 25)):
                cand = extend(peaks, end, widen_at, extra)
                look = extend(cand, min(BINS, end + 30))           # what the next band's first peaks absorb counts too
                key = (count(look, band) - (len(look) - len(cand)), -(cand[-1] if cand else 0))
                if best is None or key > best[0]:
                    best = (key, cand)
        peaks = best[1]
    return count(peaks, 23), peaks


def _ranges(rate):
    import score_model as M
    return M.Tables(rate).range


def _comb(rate, floor, peak, seed, **kw):
    amps = flat(floor)
    for b in comb_bins(_ranges(rate), **kw):
        amps[b] = peak
    return pair(amps, seed)


# cap_search(48000.0)'s placement: 96 tonal maskers and 16 bands with a free bin, 112 candidates (make_score_edges_ref.py checks it)
THINNED_48K = (3, 8, 13, 18, 23, 28, 33, 38, 44, 50, 56, 62, 69, 76, 90, 106, 124, 135, 153, 171, 187, 203, 221, 240, 261) + \
    tuple(range(285, 2036, 25))


def _thinned():
    amps = flat(100)
    for b in THINNED_48K:
        amps[b] = 10000
    return pair(amps, 15)


def _tones(bins, seed):
    x = noise(seed)
    for b in bins:
        x = x + pair({b: 1 << 12}, 100 + seed, shift=24)
    return x


def _impulse(at_l, at_r):
    x = np.zeros((2, LEN))
    x[0, at_l] = x[1, at_r] = 2.0 ** -8
    return x


def _bump(ratio_num):
    """one bin at ratio_num / 2 times the power of its two neighbours, everything else 30 dB below those: amplitudes are integer
    square roots, so the power ratio is ratio_num / 2 to 1e-4 relative -- far from 6 on either side"""
    amps = flat(316)
    k = 700
    amps[k - 1] = amps[k + 1] = 10000
    amps[k] = int(round(10000 * (ratio_num / 2.0) ** 0.5))
    return pair(amps, 12)


def _loud_band():
    """a loud band (bins 600..699) next to bins that lie near the threshold in quiet (2^-28 of its power), three lines 36 dB over
    those, and silence above bin 1200"""
    amps = flat(1, 1, 1200)
    amps.update(flat(1 << 14, 600, 700))
    amps.update({350: 64, 400: 64, 450: 64})
    return pair(amps, 13, shift=26)


def _thr_some():
    t = np.zeros(BINS)
    t[50:250] = 2.0 ** -20             # dominates over the faint bins (2^-30) that carry the case's noise_power
    t[300:500] = 2.0 ** -14            # and over the three lines (2^-18)
    t[650:680] = 2.0 ** 4              # and inside the loud band (2^-2)
    return t


def _db_amp(db, base=10000):
    return int(round(base * 10.0 ** (db / 20.0)))


CASES = {
    "silence": (48000.0, lambda: np.zeros((2, LEN)), None, "every bin at kMinPower"),
    "left_silent": (48000.0, lambda: np.stack([np.zeros(LEN), noise(1)[1]]), None, "one channel silent"),
    "right_silent": (48000.0, lambda: np.stack([noise(2)[0], np.zeros(LEN)]), None, "one channel silent"),
    "dc": (48000.0, lambda: np.full((2, LEN), 2.0 ** -10), None, "bin 0 of the real-input split alone"),
    "nyquist": (48000.0, lambda: np.tile(np.array([2.0 ** -10, -2.0 ** -10]), (2, LEN // 2)), None, "bin 2048 alone: wr = -1; hf_penalty 1"),
    "impulse_0": (48000.0, lambda: _impulse(0, 0), None, "flat spectrum from the even samples alone"),
    "impulse_odd": (48000.0, lambda: _impulse(1001, 3), None, "flat spectrum from the odd samples alone"),
    "tone_1": (48000.0, lambda: _tones([1], 3), None, "a bin-centred tone at bin 1"),
    "tone_2": (48000.0, lambda: _tones([2], 4), None, "at bin 2"),
    "tone_2046": (48000.0, lambda: _tones([2046], 5), None, "at bin 2046"),
    "tone_2047": (48000.0, lambda: _tones([2047], 6), None, "at bin 2047"),
    "peak_4": (48000.0, lambda: pair({**flat(100), 4: 10000}, 7), None, "band 0 wholly consumed: 1 tonal, 23 noise maskers"),
    "peaks_3_2045": (48000.0, lambda: pair({**flat(100), 3: 10000, 2045: 10000}, 8), None, "the first and last bin the detection visits"),
    "peaks_2_2046": (48000.0, lambda: pair({**flat(100), 2: 10000, 2046: 10000}, 9), None, "one bin outside it on either side: no tonal masker"),
    "comb": (48000.0, lambda: _comb(48000.0, 100, 10000, 10), None, "the dense comb: 100 tonal maskers, 14 empty bands"),
    "comb_thinned": (48000.0, _thinned, None, "the most masker candidates a comb placement reaches (cap_search): 96 tonal, 16 bands"),
    "comb_7p5": (48000.0, lambda: _comb(48000.0, 10000, _db_amp(7.5), 11, gap=6), None, "peaks 7.5 dB over their neighbours: tonal"),
    "comb_7p1": (48000.0, lambda: _comb(48000.0, 10000, _db_amp(7.1), 11, gap=6), None, "at 7.1 dB: still tonal, a tenth of a dB over the test"),
    "comb_6p5": (48000.0, lambda: _comb(48000.0, 10000, _db_amp(6.5), 11, gap=6), None, "the same comb at 6.5 dB: none is"),
    "bump_6p5": (48000.0, lambda: _bump(13), None, "one bin at 6.5 localAvg: the peak test passes"),
    "bump_6p1": (48000.0, lambda: _bump(12.2), None, "at 6.1 localAvg: it still passes"),
    "bump_5p5": (48000.0, lambda: _bump(11), None, "at 5.5 localAvg: it does not"),
    "loud_band": (48000.0, _loud_band, None, "softplus: a loud band beside bins at the threshold in quiet"),
    "loud_band_thr": (48000.0, _loud_band, _thr_some, "the same with a thr array that dominates in some bins"),
    "silence_44k": (44100.0, lambda: np.zeros((2, LEN)), None, "other tables: the flatness penalty is exactly 0"),
    "comb_44k": (44100.0, lambda: _comb(44100.0, 100, 10000, 14), None, "the dense comb on the 44.1 kHz tables"),
}


def cases(rate=None):
    return [n for n, c in CASES.items() if rate is None or c[0] == rate]


_CACHE = {}


def rows(name):
    if name not in _CACHE:
        x = np.ascontiguousarray(CASES[name][1](), dtype=np.float64)
        assert x.shape == (2, LEN)
        x.setflags(write=False)
        _CACHE[name] = x
    return _CACHE[name]


def thr(name):
    f = CASES[name][2]
    return None if f is None else f()
