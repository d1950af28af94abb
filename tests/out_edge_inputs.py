"""Inputs of the output stage's edge tests and the restatement of k_out_pre (convopeq_amd/csrc/out_kernels.hip), shared by the
CPU checks (test_out_edges_cpu.py: on the models alone, each input does what its GPU test relies on) and the GPU tests
(test_gpu_out_edges.py).  numpy and tests/out_model.py only.

scan_tables, scan_section and scan_dc restate the kernel's fast path lane by lane (test_out_model_cpu.py holds them to the
long-double model).  kernel_dc adds the kernel's choice of path: per span of 2048 samples, counted from the call's first sample,
the fast path if every sample of the span is below 1e14 in magnitude, the carried state of section 0 is below 1e14 and that of
section 1 below 1e15; the reference's loop otherwise, with the state guards at the callback ends.  The build uses
-ffp-contract=off and every step is a single rounded fp64 operation in a fixed order, so the device is held to kernel_dc bit
for bit.

Lane 0 of wave 0 starts from the carried state itself (e = 0, a^0 = 1), so the first 8 samples of a span are the same bits on
both paths: a threshold value in a last span of 8 samples or fewer cannot tell the paths apart (THRESHOLD_POSITIONS["last"] is
such a place; "last of a long tail" is the one that can).

The constants restate the kernels' geometry: kOpSpan = kOpThreads * kOutChunk, kOqBatch = kOqThreads * kOqPer, the 64-sample
groups of the limiter, and the grid caps of k_out_headroom (1024 x 256 lanes) and k_out_post<false, true> (256 batches)."""
import numpy as np

import out_model as M

LD = np.longdouble
SPAN = 2048                 # samples of a DC span
BATCH = 2048                # samples of a limiter batch
GROUP = 64                  # samples of a limiter group
SLICE = 256                 # a lane's k-th sample of a batch is k * 256 + lane
HEADROOM_GRID = 1024 * 256  # samples of one trip of k_out_headroom's loop
CLAMP_GRID = 256 * BATCH    # samples of one trip of k_out_post<false, true>'s loop
FAST, GUARDED = "fast", "guarded"


# ------------------------------------------------------------------------------------------- the fast path, lane by lane
def scan_tables(alpha):
    """outSectionTable: a = 1 - alpha and its powers in long double, rounded once"""
    a = LD(1) - LD(alpha)
    ac = LD(1)
    for _ in range(8):
        ac = ac * a
    pow2, p = [], ac
    for _ in range(7):
        pow2.append(float(p))
        p = p * p
    lane, q = [], LD(1)
    for _ in range(64):
        lane.append(float(q))
        q = q * ac
    return pow2, np.array(lane)


def scan_section(u, alpha, carry, tab):
    """one section over a span: u [256, 8]; returns (u - lowpass, the state after every sample) as the lanes compute them"""
    pow2, lane_pow = tab
    z = np.zeros(256)
    for i in range(8):
        z = z + alpha * (u[:, i] - z)
    ln, wv = np.arange(256) & 63, np.arange(256) >> 6
    for k in range(6):
        d = 1 << k
        z = np.where(ln >= d, z + pow2[k] * np.roll(z, d), z)
    inc = [carry]
    for w in range(3):
        inc.append(pow2[6] * inc[-1] + z[64 * w + 63])
    e = np.where(ln == 0, 0.0, np.roll(z, 1))
    s = e + lane_pow[ln] * np.array([inc[w] for w in wv])
    y, states = np.empty_like(u), np.empty_like(u)
    for i in range(8):
        s = s + alpha * (u[:, i] - s)
        y[:, i] = u[:, i] - s
        states[:, i] = s
    return y, states


def scan_dc(x, alpha, state=(0.0, 0.0)):
    """k_out_pre's fast path on one channel: spans of 2048 samples (the last one padded with zeros), the states after a span's
    last sample carried to the next span and out of the call"""
    t0, t1 = scan_tables(alpha[0]), scan_tables(alpha[1])
    c0, c1 = state
    out = []
    for s0 in range(0, len(x), 2048):
        seg = x[s0:s0 + 2048]
        flat = np.zeros(2048)
        flat[:len(seg)] = seg
        y, st0 = scan_section(flat.reshape(256, 8), alpha[0], c0, t0)
        y, st1 = scan_section(y, alpha[1], c1, t1)
        out.append(y.reshape(-1)[:len(seg)])
        c0, c1 = st0.reshape(-1)[len(seg) - 1], st1.reshape(-1)[len(seg) - 1]
    return np.concatenate(out), (c0, c1)


# ------------------------------------------------------------------------------------------------ one call of k_out_pre
def span_is_fast(seg, c0, c1):
    """the kernel's own test: !(fabs(v) < limit) is true of a NaN"""
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.abs(seg) < 1.0e14)) and abs(c0) < 1.0e14 and abs(c1) < 1.0e15


def _keep(s):
    return s if abs(s) < 1.0e15 else 0.0


def kernel_dc(x, alpha, state, cb, force=None):
    """One k_out_pre call on one channel: x [n], callbacks of cb samples counted from the call's first sample.  force =
    {span index: FAST or GUARDED} overrides the kernel's test for those spans (the CPU tests use it to show that the two paths
    give different bits).  Returns (y, (state 0, state 1), [path of every span])."""
    n = len(x)
    a0, a1 = float(alpha[0]), float(alpha[1])
    t0, t1 = scan_tables(a0), scan_tables(a1)
    c0, c1 = float(state[0]), float(state[1])
    out, paths = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for k, s0 in enumerate(range(0, n, SPAN)):
            seg = x[s0:s0 + SPAN]
            path = FAST if span_is_fast(seg, c0, c1) else GUARDED
            path = (force or {}).get(k, path)
            paths.append(path)
            if path == FAST:
                flat = np.zeros(SPAN)
                flat[:len(seg)] = seg
                y, st0 = scan_section(flat.reshape(256, 8), a0, c0, t0)
                y, st1 = scan_section(y, a1, c1, t1)
                out.append(y.reshape(-1)[:len(seg)])
                c0, c1 = float(st0.reshape(-1)[len(seg) - 1]), float(st1.reshape(-1)[len(seg) - 1])
            else:
                y = np.empty(len(seg))
                for i, v in enumerate(seg.tolist()):
                    c0 = c0 + a0 * (v - c0)
                    v = v - c0
                    c1 = c1 + a1 * (v - c1)
                    v = v - c1
                    y[i] = v
                    g = s0 + i
                    if (g + 1) % cb == 0 or g == n - 1:
                        c0, c1 = _keep(c0), _keep(c1)
                out.append(y)
    return np.concatenate(out), (c0, c1), paths


class KernelStage:
    """cpq_out_process with DC_BLOCK (and HEADROOM) as the kernels compute it: kernel_dc per channel, states carried from call
    to call, then the multiply and the scrub"""

    def __init__(self, rate, n_ch):
        self.alpha = M.design(rate)[0]
        self.state = [(0.0, 0.0)] * n_ch

    def process(self, x, cb, flags=M.DC_BLOCK, force=None):
        """x [n_ch, n] -> (y, [paths of channel 0, paths of channel 1, ...]); force = {channel: {span: path}}"""
        y, paths = np.empty_like(x), []
        for ch in range(x.shape[0]):
            y[ch], self.state[ch], p = kernel_dc(x[ch], self.alpha, self.state[ch], cb, (force or {}).get(ch))
            paths.append(p)
        if flags & M.HEADROOM:
            y = M.scrub(y * M.H)
        return y, paths

    def run(self, x, calls, cb, flags=M.DC_BLOCK):
        out, paths, o = [], [], 0
        for n in calls:
            y, p = self.process(x[:, o:o + n], cb, flags)
            out.append(y)
            paths.append(p)
            o += n
        return np.concatenate(out, axis=1), paths


def model_runs(x, rate, calls, cb, flags=M.DC_BLOCK):
    """(long-double run, fp64 run) of the sequential model on x [2 S, n] cut into the given calls"""
    runs = []
    for dt in (LD, np.float64):
        st, parts, o = M.OutStage(rate, x.shape[0] // 2, dt), [], 0
        for n in calls:
            parts.append(st.process(x[:, o:o + n], cb, flags))
            o += n
        runs.append(np.concatenate(parts, axis=1))
    return runs


def bar_figures(y, ld, f64):
    """(largest |y - long double|, largest |fp64 model - long double|) of one channel or a segment of one"""
    return float(np.max(np.abs(y.astype(LD) - ld))), float(np.max(np.abs(f64.astype(LD) - ld)))


def quiet_rows(n, seed, rows=6, amp=0.25):
    return amp * np.random.default_rng(seed).standard_normal((rows, n))


# ---------------------------------------------------------------------------------------------------- DC blocker inputs
# Every DC input is a dict: x [6, n] (three streams), calls (their lengths), B (block size = callback length), T (blocks per
# call the engine is made for), any (CPQ_CALLS_ANY), rate, flags, rows (the rows that carry the event; the others are quiet and
# fast throughout) and want[call] = the paths the event rows must take.  An even and an odd row carry every event: with an odd
# n the odd rows are the ones on the kernel's unaligned loads and stores.
DC_SIZES = (1, 8, 9, 2047, 2048, 2049, 4096, 4097, 3 * 2048 + 5)
DC_RATES = (8000.0, 192000.0, 384000.0)
N3 = 3 * 2048 + 5

THRESHOLD_VALUES = {"+1e14": 1.0e14, "-1e14": -1.0e14, "just below 1e14": float(np.nextafter(1.0e14, 0.0))}
# name -> (n, index, span of the index)
THRESHOLD_POSITIONS = {"0": (N3, 0, 0), "2047": (N3, 2047, 0), "2048 + 5": (N3, 2048 + 5, 1), "last": (N3, N3 - 1, 3),
                       "last of a long tail": (N3 + 300, N3 + 299, 3)}
SAME_BITS_ON_BOTH_PATHS = ("last",)     # the event and everything after it lie in the first 8 samples of the span


def threshold_case(value, position, rate):
    """one sample at the sample test's threshold in 0.25 noise, one call, callbacks of 512: the span that holds it is guarded
    for +-1e14 and fast for the value below; every other span is fast (the state it leaves is alpha * 1e14 at the most)"""
    n, at, span = THRESHOLD_POSITIONS[position]
    x = quiet_rows(n, 101)
    x[0, at] = x[3, at] = THRESHOLD_VALUES[value]
    paths = [FAST] * ((n + SPAN - 1) // SPAN)
    if abs(THRESHOLD_VALUES[value]) >= 1.0e14:
        paths[span] = GUARDED
    return dict(x=x, calls=[n], B=512, T=16, any=True, rate=rate, flags=M.DC_BLOCK, rows=(0, 3), want=[paths], span=span)


CARRIED_RATES = {16000.0: [[GUARDED], [GUARDED, FAST]],         # 8.4e14 after the loud callback, 9.6e13 one span later
                 48000.0: [[GUARDED], [GUARDED, GUARDED]]}       # 3.3e14, 1.6e14 one span later and 7.8e13 after the call


def carried_case(rate, flags=M.DC_BLOCK):
    """a callback of 512 samples at 2e15 leaves section 0 in [1e14, 1e15): the reference keeps that state, and the kernel has
    to walk the quiet call of 8 x 512 that follows span by span until the state has decayed below 1e14.  (At 8 kHz the state
    passes 1e15 and is zeroed, at 192 kHz and above it stays below 1e14: the rates are the ones where the case exists.)"""
    x = quiet_rows(512 + 8 * 512, 103)
    x[0, :512] = 2.0e15
    x[3, :512] = -2.0e15
    return dict(x=x, calls=[512, 8 * 512], B=512, T=16, any=True, rate=rate, flags=flags, rows=(0, 3), want=CARRIED_RATES[rate])


def long_callback_case():
    """B = 4096, whole-block calls: 1e18 in the first 100 samples.  No callback ends at sample 2047, so span 0 ends without a
    guard and hands a state of 1.7e16 to span 1, which is quiet and guarded for its carried state alone; the guard at sample
    4095 zeroes the state (8.6e15) and the second call starts from 0.  (With 1e16 the state that reaches sample 2047 is below
    1e15 at every rate: (1 - e^-100a) e^-1948a <= 0.019.)"""
    x = quiet_rows(2 * 4096, 105)
    x[0, :100] = 1.0e18
    x[3, :100] = -1.0e18
    return dict(x=x, calls=[4096, 4096], B=4096, T=2, any=False, rate=48000.0, flags=M.DC_BLOCK, rows=(0, 3),
                want=[[GUARDED, GUARDED], [FAST, FAST]])


def section1_carry_case():
    """B = 4096 again, for the test of section 1's carried state alone: 5e15 up to sample 2046 and, on sample 2047, the value
    that brings section 0 back to zero (-s0 (1 - alpha0) / alpha0, about -7e18).  Span 0 ends without a guard; span 1 is quiet
    and inherits a section-0 state of rounding size and a section-1 state of 1.2e15, which alone sends it down the guarded
    path"""
    x = quiet_rows(2 * 4096, 117)
    a0 = M.design(48000.0)[0][0]
    for row, sign in ((0, 1.0), (3, -1.0)):
        x[row, :2047] = sign * 5.0e15
        s0 = 0.0
        for v in x[row, :2047].tolist():
            s0 = s0 + a0 * (v - s0)
        x[row, 2047] = -s0 * (1.0 - a0) / a0
    return dict(x=x, calls=[4096, 4096], B=4096, T=2, any=False, rate=48000.0, flags=M.DC_BLOCK, rows=(0, 3),
                want=[[GUARDED, GUARDED], [FAST, FAST]])


def part_callback_case():
    """B = 441, calls of any length: a call of 441 + 441 + 100 with a NaN in the part callback, whose guard is the one at
    g == n - 1; the call of 441 after it starts from the zeroed states and is fast"""
    x = quiet_rows(982 + 441, 107)
    x[0, 882 + 50] = x[3, 882 + 99] = np.nan
    return dict(x=x, calls=[982, 441], B=441, T=4, any=True, rate=44100.0, flags=M.DC_BLOCK, rows=(0, 3), want=[[GUARDED], [FAST]])


def nonfinite_headroom_case():
    """DC_BLOCK | HEADROOM, the guarded path of k_out_pre<true> and the scrub after it: +Inf in span 1 (the rest of its
    callback is NaN before the scrub), 1e300 in span 0 (a state of 3.5e296 until the callback's end) and -Inf on the call's
    last sample.  want is per row here."""
    x = quiet_rows(N3, 109)
    x[0, 2048 + 5], x[3, 7], x[4, N3 - 1] = np.inf, 1.0e300, -np.inf
    return dict(x=x, calls=[N3], B=512, T=16, any=True, rate=48000.0, flags=M.DC_BLOCK | M.HEADROOM, rows=(0, 3, 4),
                want={0: [[FAST, GUARDED, FAST, FAST]], 3: [[GUARDED, FAST, FAST, FAST]], 4: [[FAST, FAST, FAST, GUARDED]]})


def denormal_rows(n):
    """six rows of denormals: noise, an offset, and both at once, at 1e-310"""
    r = np.random.default_rng(111).standard_normal((6, n))
    x = 1.0e-310 * r
    x[1] = 1.0e-310
    x[2] = 1.0e-310 * (3.0 + r[2])
    x[4] = -1.0e-310 * (3.0 + r[4])
    return x


def loud_then_quiet_rows(cb=512):
    """three callbacks: one sample of 9.9e13 in noise at 1e-3 in the first, nothing but the noise in the other two.  All fast;
    the rounding of the loud callback's states (an ulp of 3e10 is 4e-6) is what the quiet ones inherit."""
    x = quiet_rows(3 * cb, 113, amp=1.0e-3)
    x[0, 100], x[3, cb - 1], x[4, 0] = 9.9e13, -9.9e13, 9.9e13
    return x


def long_dc_rows(n):
    """one stream: noise on an offset and a two-tone with a step in the middle of the call"""
    rng = np.random.default_rng(115)
    t = np.arange(n)
    x = np.empty((2, n))
    x[0] = 0.3 + 0.25 * rng.standard_normal(n)
    x[1] = 0.4 * np.sin(2 * np.pi * 0.0021 * t + 0.3) + 0.3 * np.sin(2 * np.pi * 0.0517 * t + 1.1) + np.where(t > n // 2, 0.5, -0.2)
    return x


# -------------------------------------------------------------------------------------------------------- limiter inputs
LONG_B, LONG_T = 4096, 129
LONG_N = LONG_B * LONG_T                # 528384 = 258 spans and batches, 2.02 trips of the headroom grid

ATTACK_N = 2 * BATCH + 130              # two batches and a last one of two groups and two samples
ATTACK_POSITIONS = (1791, 1792, 2047, 2048, 2049, 4095, 4096)
ATTACK_LAST_N = (2048 + 1, 2048 + 65, 4097)


def attack_rows(n, at, seed=None):
    """one stream of 0.05 noise with 3.0 at `at`, on the left channel for an even index and (negative) on the right for an odd"""
    x = quiet_rows(n, 200 + at if seed is None else seed, rows=2, amp=0.05)
    x[at % 2, at] = 3.0 if at % 2 == 0 else -3.0
    return x


STALL_CALLS = {48000.0: 18, 96000.0: 34}            # quiet calls of 8192 after which the envelope no longer moves
STALL_ATTACK_AT = 2048 + 64 * 5 + 17
STALL_NEAR_MISS_AT = 2048 + 64 * 2 + 3


def stall_rows(rate):
    """(x [2, (calls + 1) * 8192], calls): 2.5 on the first sample, then 0.01 noise until the envelope rests on its fixed point
    below 1.0, then one call with two planted peaks.  Inside the knee the desired gain is 1.0 or more (test_out_model_cpu.py),
    so a peak "just above CLIP_START" can never attack: the peaks sit just above the threshold instead.  The near miss gives
    1 - 1.1e-16, between the fixed point and 1.0 -- it must not move the envelope -- and the attack gives 1 - 1e-12, a few
    thousand ulps below the fixed point."""
    k = STALL_CALLS[rate]
    x = quiet_rows((k + 1) * 8192, 301, rows=2, amp=0.01)
    x[0, 0] = 2.5
    o = k * 8192
    x[1, o + STALL_NEAR_MISS_AT] = -float(np.nextafter(M.THRESHOLD, 1.0))
    x[0, o + STALL_ATTACK_AT] = M.THRESHOLD * (1.0 + 1.0e-12)
    return x, [8192] * (k + 1)


NONFINITE_KINDS = {"NaN left": (np.nan, None), "NaN right": (None, np.nan), "NaN both": (np.nan, np.nan),
                   "+Inf left": (np.inf, None), "-Inf right": (None, -np.inf)}
NONFINITE_AT = (5, 2048)


def nonfinite_limiter_rows(kind, at):
    """(x, calls): 0.05 noise with the value(s) at `at`, 300 quiet samples after it, and a second call of 500"""
    calls = [at + 1 + 300, 500]
    x = quiet_rows(sum(calls), 400 + at, rows=2, amp=0.05)
    for ch, v in enumerate(NONFINITE_KINDS[kind]):
        if v is not None:
            x[ch, at] = v
    return x, calls


def long_scrub_rows():
    """HEADROOM alone over more than two trips of k_out_headroom's grid: values on both sides of the scrub's bound and NaN and
    Inf, in every trip"""
    x = quiet_rows(LONG_N, 501, rows=2, amp=0.3)
    edge = 1.0e300 / M.H
    for q, at in enumerate((3, HEADROOM_GRID - 1, HEADROOM_GRID, HEADROOM_GRID + 1, 2 * HEADROOM_GRID - 1, 2 * HEADROOM_GRID,
                            2 * HEADROOM_GRID + 77, LONG_N - 1)):
        for ch in range(2):
            x[ch, at - ch] = (edge * 1.0001, np.nan, edge * 0.9999, -np.inf)[(q + ch) % 4]
    return x


def long_clamp_rows():
    """0.3 noise (a few hundred samples beyond +-H by themselves) with planted values beyond +-H in the 257th and 258th batch"""
    x = quiet_rows(LONG_N, 503, rows=2, amp=0.3)
    for q, at in enumerate((CLAMP_GRID - 1, CLAMP_GRID, CLAMP_GRID + 1, CLAMP_GRID + BATCH - 1, CLAMP_GRID + BATCH, LONG_N - 1)):
        x[q % 2, at] = (2.0, -2.0, np.inf)[q % 3]
        x[1 - q % 2, at] = (-1.5, 1.5)[q % 2]
    return x


def long_attack_rows():
    """0.05 noise and one attack in the 257th batch"""
    x = quiet_rows(LONG_N, 505, rows=2, amp=0.05)
    x[1, CLAMP_GRID + 1] = -3.0
    return x
