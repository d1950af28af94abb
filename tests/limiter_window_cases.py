"""The windows, call lengths and signals at which a rule of k_lim_apply or k_lim_keep (csrc/lim_kernels.hip) changes, shared by
tests/test_gpu_limiter_windows.py (the device object against the host object) and tests/test_limiter_window_cases_cpu.py (every
case limits, on the host object alone), with the numpy helpers tests/test_gpu_limiter.py uses as well.  No torch, no GPU.

The formulas are csrc/lim_plan.hpp's, restated; test_limiter_window_cases_cpu.py reads the constants out of the headers and holds
these to them.  M = W + taps (the minimum's window), D = W + taps - 1 (the latency), halo = 2 W + 2 taps - 3 (the history, and the
longest kept length), nR = tile + M + W - 2 (r values per tile, written in rounds of 256).  The sliding minimum doubles its window
1, 2, 4, ... while 2^k <= M and then takes one step of M - 2^k, swinging between two LDS stages: it starts on stage B, so an even
step count leaves the result on B and an odd one on A."""
import numpy as np

import convopeq_amd as amd

TILE = 1024             # kLimTile
ROUND = 256             # kLimThreads: r positions of one round
KEEP_CHUNK = 256        # kLimKeepBlock: samples of one chunk of the keep step, partials of one trip of the fold
PEAK_TAPS = 12          # kPeakTaps
MIN_WINDOW, MAX_WINDOW = 8, 1024
RATE = 48000
CEIL_DB = -1.0


def lim_m(W):
    return W + PEAK_TAPS


def lim_d(W):
    return W + PEAK_TAPS - 1


def lim_halo(W):
    return lim_m(W) + W - 2 + PEAK_TAPS - 1


def lim_r_count(W):
    return TILE + lim_m(W) + W - 2


def min_steps(W):
    """the steps of the sliding minimum, as k_lim_apply takes them"""
    M, have, steps = lim_m(W), 1, []
    while have < M:
        steps.append(have if 2 * have <= M else M - have)
        have += steps[-1]
    return steps


def remainder_step(W):
    """the last step where it is not a doubling: M - 2^k, or 0 where M is a power of two"""
    M = lim_m(W)
    return M - (1 << (M.bit_length() - 1))


def is_pow2(v):
    return v >= 1 and v & (v - 1) == 0


# class -> (windows, what every window of the class has)
CLASSES = {
    "M a power of two: no remainder step": ((20, 52, 116, 244, 500, 1012), lambda W: is_pow2(lim_m(W)) and remainder_step(W) == 0),
    "M = 2^k + 1: a remainder step of 1": ((21, 53, 245, 1013), lambda W: is_pow2(lim_m(W) - 1) and min_steps(W)[-1] == 1),
    "M = 2^k - 1: the largest remainder step": ((19, 115, 499, 1011), lambda W: is_pow2(lim_m(W) + 1) and min_steps(W)[-1] == sum(min_steps(W)[:-1])),
    "nR a whole number of rounds": ((123, 251), lambda W: lim_r_count(W) % ROUND == 0),
    "nR two past a whole number of rounds": ((124,), lambda W: lim_r_count(W) % ROUND == 2),
    "nR two short of a whole number of rounds": ((122,), lambda W: lim_r_count(W) % ROUND == ROUND - 2),
    "halo one short of 1 keep chunk": ((117,), lambda W: lim_halo(W) == KEEP_CHUNK - 1),
    "halo one past 1 keep chunk": ((118,), lambda W: lim_halo(W) == KEEP_CHUNK + 1),
    "halo one short of 2 keep chunks": ((245,), lambda W: lim_halo(W) == 2 * KEEP_CHUNK - 1),
    "halo one past 2 keep chunks": ((246,), lambda W: lim_halo(W) == 2 * KEEP_CHUNK + 1),
    "halo one short of 4 keep chunks": ((501,), lambda W: lim_halo(W) == 4 * KEEP_CHUNK - 1),
    "halo one past 4 keep chunks": ((502,), lambda W: lim_halo(W) == 4 * KEEP_CHUNK + 1),
    "D one short of a tile": ((1012,), lambda W: lim_d(W) == TILE - 1),
    "D a tile": ((1013,), lambda W: lim_d(W) == TILE),
    "D a tile and one: the flush's second tile has one output": ((1014,), lambda W: lim_d(W) == TILE + 1),
    "the limits": ((MIN_WINDOW, MAX_WINDOW), lambda W: W in (MIN_WINDOW, MAX_WINDOW)),
}
SWEEP_WINDOWS = tuple(sorted({W for ws, _ in CLASSES.values() for W in ws}))
OLD_WINDOWS = (8, 72, 1024)         # test_gpu_limiter.py's
MODEL_WINDOWS = (20, 21, 117, 1013)
IN_PLACE_WINDOWS = (116, 1013)
SWEEP_STREAMS = 2


# ------------------------------------------------------------------------------------------ what test_gpu_limiter.py uses too
def same(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


def noise(n_streams, n, seed, level=0.2):
    return level * np.random.default_rng(seed).standard_normal((2 * n_streams, n))


def plant(x, at, amp=2.5):
    """a peak well above the ceiling at sample `at`, on alternating channels of every stream"""
    for s in range(x.shape[0] // 2):
        x[2 * s + (s + at) % 2, at] = amp * (-1.0) ** s
    return x


def gains(n_streams):
    return 0.8 + 0.05 * (np.arange(n_streams) % 9)


def host_object(n_streams, W, rate=RATE):
    host = amd.TruePeakLimiter(n_streams, rate, CEIL_DB, W, host=True)
    host.set_gains(gains(n_streams))
    return host


def host_pieces(host, x, lengths):
    out, at = [], 0
    for k in lengths:
        out.append(host.process(x[:, at:at + k]))
        at += k
    assert at == x.shape[1]
    out.append(host.flush())
    return out


def plant_in(x, stream, at, amp):
    """a peak in one stream only"""
    x[2 * stream + at % 2, at] = amp * (-1.0) ** stream
    return x


# --------------------------------------------------------------------------------------------------------- the window sweep
def sweep_lengths(W):
    """5, then up to one short of the halo (the history grows across every keep chunk boundary below the halo in a call shorter
    than the halo), 1 (the history reaches the halo exactly; from here on it moves by keepShift = n), a tile and one, 2, two
    tiles and three"""
    return [5, lim_halo(W) - 6, 1, TILE + 1, 2, 2 * TILE + 3]


def sweep_peaks(W):
    """(stream or None for every stream, sample, amplitude).  Every stream: sample 0, the last sample of the second call, the
    last sample of the programme (the flush carries its dip).  Stream 0: three peaks M - 1 and then M samples apart (one window
    of the minimum holds the first two, none holds the last two).  Stream 1: three peaks W - 1 and then W samples apart.  In a
    chain the earlier peak is the higher one, so the minimum at the later peak's position tells whether its window still holds
    the earlier one.  The first gap of a chain straddles the seam between the first two tiles of the long call; at the largest
    windows, where 2 M - 1 samples do not fit behind that, the chain ends 5 samples before the programme does and starts in front
    of the long call."""
    lengths = sweep_lengths(W)
    n, start = sum(lengths), sum(lengths[:-1])
    peaks = [(None, 0, 2.5), (None, lengths[0] + lengths[1] - 1, 2.5), (None, n - 1, 2.5)]
    for stream, first, second in ((0, lim_m(W) - 1, lim_m(W)), (1, W - 1, W)):
        at = min(start + TILE - first // 2, n - 5 - first - second)
        peaks += [(stream, at, 3.0), (stream, at + first, 2.2), (stream, at + first + second, 1.6)]
    return peaks


def sweep_signal(W):
    """[4, n]: stream 0 is quiet noise, where only the planted peaks limit; stream 1 noise twice as loud, where about one sample in
    a hundred limits by an amount of its own, so that r, the minimum and the envelope differ from slot to slot"""
    n = sum(sweep_lengths(W))
    x = noise(SWEEP_STREAMS, n, 7000 + W)
    x[2:] *= 2.0
    positions = set()
    for stream, at, amp in sweep_peaks(W):
        assert 0 <= at < n and (stream, at) not in positions and (None, at) not in positions
        positions.add((stream, at))
        if stream is None:
            plant(x, at, amp)
        else:
            plant_in(x, stream, at, amp)
    return x


def wide(lengths, stride_pad):
    """per call: both row strides even, which is the kernels' 16-byte path (the test buffers are aligned)"""
    return [(k + stride_pad) % 2 == 0 for k in lengths]


# ------------------------------------------------------------------------------- more than 256 tiles, partials that grow
FOLD_W = 8
FOLD_LENGTHS = [3, KEEP_CHUNK * TILE, (KEEP_CHUNK + 1) * TILE + 1, 1500]
FOLD_DEEPEST_AMP = 6.0


def fold_call_starts():
    return [int(v) for v in np.cumsum([0] + FOLD_LENGTHS)]


def fold_peaks():
    """(sample, amplitude, call, tile of that call the dip begins in).  A peak at input sample p pulls down the outputs
    p ... p + halo, 38 of them at W = 8.  The third call has 258 tiles: one trip of the fold takes tiles 0 ... 255, the second 256
    and 257, and 257 has one output."""
    s = fold_call_starts()
    third = s[2]
    return [(0, 2.5, 0, 0),
            (s[1] + 100, 2.5, 1, 0), (s[1] + (KEEP_CHUNK - 1) * TILE + 500, 2.5, 1, KEEP_CHUNK - 1),
            (third + 200, 2.5, 2, 0), (third + (KEEP_CHUNK - 1) * TILE + 300, 2.5, 2, KEEP_CHUNK - 1),
            (third + KEEP_CHUNK * TILE + 400, FOLD_DEEPEST_AMP, 2, KEEP_CHUNK),
            (third + (KEEP_CHUNK + 1) * TILE - 10, 2.5, 2, KEEP_CHUNK),         # the last 10 outputs of tile 256 and the one of 257
            (s[3] + TILE + 76, 2.5, 3, 1)]


def fold_signal(n_streams, deepest=True):
    x = noise(n_streams, sum(FOLD_LENGTHS), 900 + n_streams)
    for at, amp, _, _ in fold_peaks():
        if deepest or amp != FOLD_DEEPEST_AMP:
            plant(x, at, amp)
    return x


def host_telemetry(n_streams, W, x, lengths):
    host = host_object(n_streams, W)
    host_pieces(host, x, lengths)
    return host.telemetry()
