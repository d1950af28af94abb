"""numpy restatement of the dither stage (convopeq_amd/csrc/dither_design.cpp): FixedNoiseShaper (4 taps) and
Fixed15TapNoiseShaper (ORDER 16) of the reference, vectorised over channels, sample after sample, in the reference's operation
order.  Python floats and numpy's elementwise operations are IEEE fp64 without contraction, so the model is bit-exact.

Per sample and channel: x = in * headroom; fb = sum c[k] e[k] (e[0] the newest error; 4 taps: one expression left to right; 15
taps: fb = 0.0, fb += c[k] e[k]); y = x - fb; v = clamp(y, -1, 1 - scale) + (u1 + u2 - 1) * scale; yq = rint(v * invScale) * scale;
stored error = yq - y clamped to +-2 scale.  Non-finite values: the 4-tap shaper zeroes a non-finite y before the clamp and a
non-finite result, its error passes std::clamp (a NaN stays) and is zeroed when not finite; the 15-tap shaper guards nothing,
clamps the rounded code with std::clamp (a NaN stays), and its error passes max_sd / min_sd (a NaN becomes -2 scale).

Every stream is a DSPCore of its own: all L channels start from one generator state, all R channels from another."""
import math
import struct

import numpy as np

OFF, FIXED4, FIXED15 = 0, 1, 2
H = 0.8912509381337456
RATES = (44100.0, 48000.0, 88200.0, 96000.0, 176400.0, 192000.0, 352800.0, 384000.0, 705600.0, 768000.0)
PRESETS4 = ((0.394958, 0.319775, 0.145569, 0.139697), (0.460000, 0.280000, 0.170000, 0.090000),
            (0.727810, 0.189547, 0.125028, -0.042385), (0.742333, 0.185474, 0.106133, -0.033940),
            (0.775904, 0.126967, 0.043467, 0.053661), (0.774132, 0.117440, 0.047291, 0.061137),
            (0.724647, 0.094403, 0.113208, 0.067743), (0.714605, 0.097798, 0.124553, 0.063045),
            (0.635851, 0.161114, 0.194506, 0.008529), (0.624827, 0.174509, 0.201424, -0.000760))
PRESETS15 = (
    (2.157553, -2.356649, 2.179194, -1.802605, 1.429476, -1.073975, 0.775233, -0.535496, 0.360294, -0.229526, 0.143225, -0.081483, 0.045992, -0.021109, 0.009877, 0.0),
    (2.172009, -2.313034, 2.092949, -1.698718, 1.304487, -0.946581, 0.645299, -0.415598, 0.251068, -0.141026, 0.072650, -0.033120, 0.012821, -0.004274, 0.001068, 0.0),
    (1.458665, -1.271063, 1.372588, -1.257752, 1.186326, -1.042666, 0.931875, -0.787020, 0.671068, -0.541164, 0.438950, -0.333234, 0.250772, -0.174640, 0.097295, 0.0),
    (1.366976, -1.123204, 1.234291, -1.119397, 1.063887, -0.931030, 0.838107, -0.707665, 0.608977, -0.492384, 0.404256, -0.308827, 0.236248, -0.167088, 0.096853, 0.0),
    (0.892356, -0.425055, 0.645737, -0.531778, 0.565511, -0.483687, 0.474500, -0.404025, 0.379228, -0.317474, 0.286683, -0.233505, 0.199702, -0.166141, 0.117948, 0.0),
    (0.842437, -0.356337, 0.593464, -0.477529, 0.519248, -0.440863, 0.438827, -0.372969, 0.354221, -0.297057, 0.271334, -0.222591, 0.192842, -0.164283, 0.119255, 0.0),
    (0.576947, -0.000943, 0.355358, -0.225398, 0.306449, -0.241465, 0.271718, -0.228634, 0.237327, -0.205281, 0.201703, -0.179310, 0.166143, -0.176849, 0.142236, 0.0),
    (0.550200, 0.035746, 0.334748, -0.202925, 0.287573, -0.223403, 0.255932, -0.214959, 0.225551, -0.196308, 0.194281, -0.175339, 0.163224, -0.180050, 0.145728, 0.0),
    (0.403358, 0.274330, 0.229984, -0.085257, 0.190310, -0.131467, 0.169688, -0.142598, 0.154703, -0.144947, 0.142117, -0.148598, 0.132904, -0.195545, 0.151017, 0.0),
    (0.390229, 0.306061, 0.221612, -0.075413, 0.182734, -0.125438, 0.162912, -0.138648, 0.149015, -0.142960, 0.137870, -0.149116, 0.130580, -0.202133, 0.152692, 0.0))
SEEDS4 = ((0x123456789ABCDEF0, 0xFEDCBA9876543210, 0x0123456789ABCDEF, 0xEFCDAB8967452301),
          (0x89ABCDEF01234567, 0x76543210FEDCBA98, 0xABCDEF0123456789, 0x67452301EFCDAB89))
M64 = (1 << 64) - 1
U64 = np.uint64


def order_of(shaper):
    return {FIXED4: 4, FIXED15: 16}[shaper]


def design(rate, shaper, bits):
    """prepare(rate, bits) of a shaper fresh from its constructor: (coefficients [16], unused taps 0.0; scale)"""
    assert 1 <= bits <= 32
    order = order_of(shaper)
    table = PRESETS4 if order == 4 else PRESETS15
    lo = hi = 0
    t = 0.0
    if rate <= RATES[0]:
        pass
    elif rate >= RATES[-1]:
        lo = hi = len(RATES) - 1
    else:
        for i in range(len(RATES) - 1):
            if RATES[i] <= rate < RATES[i + 1]:
                lo, hi, t = i, i + 1, (rate - RATES[i]) / (RATES[i + 1] - RATES[i])
                break
    if t < 1e-12:
        c = list(table[lo])
    elif t > 1.0 - 1e-12:
        c = list(table[hi])
    else:
        c = [(1.0 - t) * a + t * b for a, b in zip(table[lo], table[hi])]
    if order == 4 and abs(c[0] + c[1] + c[2] + c[3] - 1.0) > 1.0e-12:
        c = list(PRESETS4[1])       # setCoefficients refuses the set and the constructor's values, the 48 kHz preset, stay
    return c + [0.0] * (16 - order), 1.0 / math.ldexp(1.0, bits - 1)


def _splitmix(state):
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def seed(shaper, rate, bits, ch):
    """the four xoshiro256++ words of channel ch (0 = L, 1 = R)"""
    if shaper == FIXED4:
        return list(SEEDS4[ch])
    safe = rate if (rate > 0.0 and math.isfinite(rate)) else 48000.0
    s = struct.unpack("<Q", struct.pack("<d", safe))[0]
    s ^= (bits << 32) & M64
    s ^= 0xD1B54A32D192ED03
    stream = s ^ ((0x9E3779B97F4A7C15 * (ch + 1)) & M64)
    words = []
    for _ in range(4):
        stream, w = _splitmix(stream)
        words.append(w)
    if not any(words):
        words[0] = 1
    return words


def _rotl(x, k):
    return (x << U64(k)) | (x >> U64(64 - k))


def _uniform(s):
    """s: uint64 [4, channels], advanced in place; returns float64 [channels]"""
    result = _rotl(s[0] + s[3], 23) + s[0]
    t = s[1] << U64(17)
    s[2] ^= s[0]
    s[3] ^= s[1]
    s[1] ^= s[2]
    s[0] ^= s[3]
    s[2] ^= t
    s[3] = _rotl(s[3], 45)
    return (result >> U64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _finite_or_zero(v):
    return np.where(np.isfinite(v), v, 0.0)


def scrub(v):
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(v) < 1.0e300, v, 0.0)


def encode16(rows):
    """the 16-bit pack: rint(x * 32768), ties to even, NaN -> 0, clipped to [-32768, 32767]"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.rint(np.asarray(rows, dtype=np.float64) * 32768.0)
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(v, -32768.0, 32767.0).astype(np.int64).astype(np.int16)


def recorded(fx, sh, bits, rate):
    """tests/golden/dither_ref.npz: the reference's output rows of one case: codes * scale, NaN where it delivered a non-finite value"""
    key = f"{sh}_{bits}_{int(rate)}"
    n = fx["input"].shape[1]
    y = fx["codes_" + key].astype(np.float64) / float(1 << (bits - 1))
    bad = np.unpackbits(fx["bad_" + key], axis=1)[:, :n].astype(bool)
    negzero = np.unpackbits(fx["negzero_" + key], axis=1)[:, :n].astype(bool)
    return np.where(bad, np.nan, np.where(negzero, -0.0, y))


class Dither:
    def __init__(self, rate, n_streams, shaper, bits):
        self.S, self.shaper, self.bits, self.order = n_streams, shaper, bits, order_of(shaper)
        self._design(rate)
        self._seed(rate)
        self.reset()

    def _design(self, rate):
        self.coeffs, self.scale = design(rate, self.shaper, self.bits)
        self.inv = math.ldexp(1.0, self.bits - 1)

    def _seed(self, rate):
        words = [seed(self.shaper, rate, self.bits, ch) for ch in (0, 1)]
        self.rng = np.array([[words[c % 2][k] for c in range(2 * self.S)] for k in range(4)], dtype=np.uint64)

    def prepare(self, rate):
        """prepare() again: coefficients, errors cleared, the 15-tap shaper reseeded"""
        self._design(rate)
        if self.shaper == FIXED15:
            self._seed(rate)
        self.reset()

    def reset(self):
        self.err = np.zeros((self.order, 2 * self.S))

    def process(self, x, headroom=H, scrubbed=False):
        """x [2 S, n] -> the shaper's output; state carried"""
        x = np.asarray(x, dtype=np.float64)
        y_out = np.empty_like(x)
        c, sc, inv, e, s = self.coeffs, self.scale, self.inv, self.err, self.rng
        max_v, lim = 1.0 - (1.0 / inv), 2.0 * sc
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(x.shape[1]):
                xi = x[:, i] * headroom
                if self.order == 4:
                    fb = c[0] * e[0] + c[1] * e[1] + c[2] * e[2] + c[3] * e[3]
                else:
                    fb = np.zeros(x.shape[0])
                    for k in range(16):
                        fb = fb + c[k] * e[k]
                y = xi - fb
                v = _finite_or_zero(y) if self.order == 4 else y
                v = np.where(v < -1.0, -1.0, np.where(v > max_v, max_v, v))
                u1 = _uniform(s)
                u2 = _uniform(s)
                v = v + (u1 + u2 - 1.0) * sc
                q = np.rint(v * inv)
                if self.order == 4:
                    yq = _finite_or_zero(q * sc)
                    error = yq - y
                    stored = np.where(error < -lim, -lim, np.where(lim < error, lim, error))
                else:
                    yq = np.where(q < -inv, -inv, np.where(inv - 1.0 < q, inv - 1.0, q)) * sc
                    error = yq - y
                    stored = np.where(error > -lim, error, -lim)
                    stored = np.where(stored < lim, stored, lim)
                stored = _finite_or_zero(stored)
                e[1:] = e[:-1].copy()
                e[0] = stored
                y_out[:, i] = yq
        return scrub(y_out) if scrubbed else y_out
