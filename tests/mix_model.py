"""Plain models of what the kernels of convopeq_amd/csrc/mix_kernels.hip compute, written from the reference's description of
each operation (file and lines at every function), for tests/test_gpu_mix_kernels.py (bit equality with the device) and
tests/test_mix_model_cpu.py (the models against exact rational arithmetic and against the oracle).

fp64 numpy / Python floats for everything unfused: every step is one correctly rounded IEEE operation, as on the device (the
library is built with -ffp-contract=off).  The reference's two fused loops (the direct head's tap loop, the RMS accumulation)
use fma() below: exact rational product and sum, rounded once.  Ring positions and cursors are Python integers."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def fma(a, b, c):
    """a * b + c rounded once"""
    a, b, c = float(a), float(b), float(c)
    if hasattr(math, "fma"):
        try:
            return math.fma(a, b, c)
        except (OverflowError, ValueError):
            return a * b + c
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:                       # the sign of an exact zero: that of the unfused sum (round to nearest)
        return a * b + c
    try:
        return float(r)
    except OverflowError:
        return math.inf if r > 0 else -math.inf


# ---------------------------------------------------------------------------------------------------------------- direct head
def direct_head_sample(h, nt, win):
    """processDirectBlock (src/MKLNonUniformConvolver.cpp:1197-1222) for one output sample: win[k], k < nt, is the window
    [history | block] from this sample on; two 4-lane FMA accumulators over groups of 8 taps, summed lane-wise, then
    horizontally as (0 + 2) + (1 + 3); scalar tail with separate multiply and add; flush of a non-finite or sub-1e-20 result."""
    s0, s1 = [0.0] * 4, [0.0] * 4
    v8 = nt // 8 * 8
    for k in range(0, v8, 8):
        for j in range(4):
            s0[j] = fma(h[k + j], win[k + j], s0[j])
            s1[j] = fma(h[k + 4 + j], win[k + 4 + j], s1[j])
    v = [np.float64(s0[j]) + np.float64(s1[j]) for j in range(4)]
    with np.errstate(all="ignore"):
        y = (v[0] + v[2]) + (v[1] + v[3])
        for k in range(v8, nt):
            y = y + np.float64(h[k]) * np.float64(win[k])
    if not (np.isfinite(y) and abs(y) >= 1.0e-20):
        y = 0.0
    return float(y)


def direct_head(x, ir_rev, taps, ir_slot, hist_old, wet_on=None):
    """x: [n_ch][n] the block, hist_old: [n_ch][32] the 32 samples before it.  Returns (dout [n_ch][n], hist_new [n_ch][32]).
    A stream with wet_on == 0 rests: zero output, history kept.  nt == 0: zero output."""
    n_ch, n = x.shape
    dout = np.zeros((n_ch, n))
    hist_new = np.empty((n_ch, 32))
    for c in range(n_ch):
        if wet_on is not None and wet_on[c // 2] == 0:
            hist_new[c] = hist_old[c]
            continue
        full = np.concatenate([hist_old[c], x[c]])           # sample p of the block is full[32 + p]
        hist_new[c] = full[-32:]
        nt = int(taps[ir_slot[c]])
        h = ir_rev[ir_slot[c]]
        if nt == 0:
            continue
        for s in range(n):
            dout[c, s] = direct_head_sample(h, nt, full[32 + s - (nt - 1): 32 + s + 1])
    return dout, hist_new


def direct_head_exact(x, ir_rev, taps, ir_slot, hist_old):
    """the same for inputs whose every product and partial sum is an integer below 2^53 (fused or not, any order: the same
    bits), vectorised: only the placement of taps, history and samples is modelled.  No flush can occur (|y| >= 1 or y == 0)."""
    n_ch, n = x.shape
    dout = np.zeros((n_ch, n))
    for c in range(n_ch):
        nt = int(taps[ir_slot[c]])
        full = np.concatenate([hist_old[c], x[c]])
        for k in range(nt):
            dout[c] += ir_rev[ir_slot[c], k] * full[32 - (nt - 1) + k: 32 - (nt - 1) + k + n]
    return dout


# ---------------------------------------------------------------------------------------------------------------------- AGC
def block_mean_square(d):
    """calculateRMS (src/eqprocessor/EQProcessor.Processing.cpp:21-52) up to its divide: four FMA lanes over i % 4 for the whole
    groups of 4, summed left to right, the remainder by multiply and add, divided by the length"""
    B = len(d)
    v_end = B // 4 * 4
    lane = [0.0] * 4
    for i in range(v_end):
        lane[i % 4] = fma(d[i], d[i], lane[i % 4])
    s = np.float64(lane[0])
    with np.errstate(all="ignore"):
        s = ((s + np.float64(lane[1])) + np.float64(lane[2])) + np.float64(lane[3])
        for i in range(v_end, B):
            s = s + np.float64(d[i]) * np.float64(d[i])
        return float(s / np.float64(B))


def block_rms(d):
    """calculateRMS: the square root of block_mean_square"""
    return float(np.sqrt(np.float64(block_mean_square(d))))


def agc_gains(rms_in, rms_out, state, on, T, B, b_att, b_rel, b_sm):
    """processAGC (:405-442) and calculateAGCGain (:343-358) per stream over T callbacks.  rms_in / rms_out: [2 S][T] per channel
    (the stream's value is the largest channel value above 0: `if (rms > max) max = rms` from 0, so a NaN never wins);
    state: [S][3] = envIn, envOut, gain.  Returns (state, gains [S][T][2] = start gain, per-sample increment; NaN bits of
    the 0xFF prefill where the stream is off)."""
    S = len(on)
    state = np.array(state, dtype=np.float64).reshape(S, 3).copy()
    gains = np.full((S, T, 2), np.nan).view(np.uint64)
    gains[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    gains = gains.view(np.float64)
    f = np.float64
    with np.errstate(all="ignore"):
        for s in range(S):
            if not on[s]:
                continue
            env_in, env_out, cur = f(state[s, 0]), f(state[s, 1]), f(state[s, 2])
            for t in range(T):
                r = [f(0.0), f(0.0)]
                for k, src in enumerate((rms_in, rms_out)):
                    for ch in range(2):
                        v = f(src[2 * s + ch][t])
                        if v > r[k]:
                            r[k] = v
                    if not np.isfinite(r[k]) or r[k] > 1000.0:
                        r[k] = f(1000.0)
                in_a = f(b_att) if r[0] > env_in else f(b_rel)
                out_a = f(b_att) if r[1] > env_out else f(b_rel)
                env_in = env_in * (f(1.0) - in_a) + r[0] * in_a
                env_out = env_out * (f(1.0) - out_a) + r[1] * out_a
                if env_in < 1.0e-20:
                    env_in = f(0.0)
                if env_out < 1.0e-20:
                    env_out = f(0.0)
                target = f(1.0)
                if not env_out < 1.0e-6:
                    ratio = env_in / env_out
                    if not (ratio > f(1.0) / f(1.059) and ratio < 1.059):
                        lo, hi = f(np.float32(0.06)), f(16.0)           # AGC_MIN_GAIN / AGC_MAX_GAIN are floats
                        target = lo if ratio < lo else (hi if ratio > hi else ratio)
                nxt = cur * (f(1.0) - f(b_sm)) + target * f(b_sm)
                gains[s, t, 0] = cur
                gains[s, t, 1] = (nxt - cur) / f(B)
                cur = nxt
            state[s] = (env_in, env_out, cur)
    return state, gains


def ramp_gains(start, inc, B):
    """applyGainRamp_AVX2 (:279-337): the gain every sample of one callback is multiplied with.  Four lanes start at start +
    j * inc; inside a group of 16 the lanes advance by 4 * inc three times from the group's value, the group's value itself by
    16 * inc; the remaining groups of 4 advance by 4 * inc; the last B % 4 samples from start + i * inc by inc."""
    f = np.float64
    start, inc = f(start), f(inc)
    g = np.empty(B)
    with np.errstate(all="ignore"):
        v = np.array([start, start + inc, start + f(2.0) * inc, start + f(3.0) * inc])
        inc4, inc16 = f(4.0) * inc, f(16.0) * inc
        i = 0
        while i + 16 <= B:
            w = v.copy()
            for sub in range(4):
                g[i + 4 * sub: i + 4 * sub + 4] = w
                w = w + inc4
            v = v + inc16
            i += 16
        while i + 4 <= B:
            g[i: i + 4] = v
            v = v + inc4
            i += 4
        if i < B:
            gain = start + f(i) * inc
            while i < B:
                g[i] = gain
                gain = gain + inc
                i += 1
    return g


def gain_ramp(data, gains, on, B, T):
    """data: [2 S][>= B * T]; the streams flagged in `on` are multiplied callback by callback with ramp_gains"""
    out = data.copy()
    with np.errstate(all="ignore"):
        for s in range(len(on)):
            if on[s]:
                for t in range(T):
                    g = ramp_gains(gains[s, t, 0], gains[s, t, 1], B)
                    for c in (2 * s, 2 * s + 1):
                        out[c, t * B:(t + 1) * B] = data[c, t * B:(t + 1) * B] * g
    return out


def block_silence(data, S, B, T):
    """isAudioBlockSilent (:460-475): 1 when no sample of either channel of the callback is above 1e-8 in magnitude"""
    sil = np.empty((S, T), dtype=np.int32)
    for s in range(S):
        for t in range(T):
            blk = data[2 * s:2 * s + 2, t * B:(t + 1) * B]
            sil[s, t] = 0 if (np.abs(blk) > 1.0e-8).any() else 1
    return sil


# ------------------------------------------------------------------------------------------------------------- ring chunks
def _ring_read(ring_row, start, count):
    size = len(ring_row)
    return ring_row[(int(start) + np.arange(count)) % size]


def ring_get_chunks(out, ch_map, n, q, ring, pos, cnt):
    """Get() of layer 0 per chunk (ringRead, src/MKLNonUniformConvolver.cpp:1376-1402): cnt samples from the ring, zeros after"""
    out = out.copy()
    for c, row in enumerate(ch_map):
        if row < 0:
            continue
        for cb in range((n + q - 1) // q):
            m = min(q, n - cb * q)
            v = np.zeros(m)
            k = min(int(cnt[cb]), m)
            v[:k] = _ring_read(ring[c], pos[cb], k)
            out[row, cb * q: cb * q + m] = v
    return out


def ring_add_chunks(out, ch_map, n, q, ring, sched, gain):
    """delayLineReadAdd per chunk (:1653-1688): a negative entry adds nothing; a gain within 1e-12 of 1 adds the samples as they are"""
    out = out.copy()
    unity = abs(gain - 1.0) < 1.0e-12
    with np.errstate(all="ignore"):
        for c, row in enumerate(ch_map):
            if row < 0:
                continue
            for cb in range((n + q - 1) // q):
                if sched[cb] < 0:
                    continue
                m = min(q, n - cb * q)
                v = _ring_read(ring[c], sched[cb], m)
                seg = out[row, cb * q: cb * q + m]
                out[row, cb * q: cb * q + m] = seg + v if unity else seg + v * np.float64(gain)
    return out


def rows_gather(src, ch_map, n, strides, offs):
    """Add(): every layer accumulates the same input (:1431-1446).  Returns the destinations [n_ch][stride], 0xFF where nothing is stored"""
    dst = []
    for st, of in zip(strides, offs):
        d = np.empty((len(ch_map), st), dtype=np.uint64)
        d[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
        d = d.view(np.float64)
        for c, row in enumerate(ch_map):
            if row >= 0:
                d[c, of: of + n] = src[row, :n]
        dst.append(d)
    return dst


# ------------------------------------------------------------------------------------------------------------ convproc mix
def ring_put(ring, z, n, pos):
    ring = ring.copy()
    size = ring.shape[1]
    for i in range(n):
        ring[:, (pos + i) % size] = z[:, i]
    return ring


def ring_regrow(old, new_size, end):
    """a larger ring takes over absolute positions end - old_size .. end - 1; everything else stays zero"""
    n_ch, old_size = old.shape
    new = np.zeros((n_ch, new_size))
    for p in range(end - old_size, end):
        new[:, p % new_size] = old[:, p % old_size]
    return new


def convproc_mix(wet, n, gains, ring, pos0, d_new, d_old, x_len=None, x_gains=None, wet_valid=1, ramp_len=None, ramp_gains=None,
                 ramp_off=0, wet_on=None):
    """ConvolverProcessor::process, steady state (src/convolver/ConvolverProcessor.Runtime.cpp): the dry signal from the delay
    ring, delayed d_new (during a latency cross-fade new * g + old * (1 - g) for the first x_len samples, :394-540), the wet
    signal scrubbed (finite and |x| < 1e300, else 0, :50-60), mixed wet * wetGain + dry * dryGain (:635-657) with per-sample
    gains for the first ramp_len - ramp_off samples (:591-607); no wet: the delayed dry signal alone (:573-585).
    Returns out [n_ch][n]."""
    n_ch = wet.shape[0]
    size = ring.shape[1]
    out = np.empty((n_ch, n))
    i = np.arange(n)
    with np.errstate(all="ignore"):
        for c in range(n_ch):
            s = c // 2
            dry = ring[c, (pos0 + i - int(d_new[s])) % size]
            nx = 0 if x_len is None else int(x_len[s])
            if nx > 0:
                g = x_gains[s, :nx]
                old = ring[c, (pos0 + i[:nx] - int(d_old[s])) % size]
                dry = dry.copy()
                dry[:nx] = dry[:nx] * g + old * (1.0 - g)
            if not (wet_valid and (wet_on is None or wet_on[s])):
                out[c] = dry
                continue
            w = wet[c, :n]
            w = np.where(np.isfinite(w) & (np.abs(w) < 1.0e300), w, 0.0)
            wg, dg = np.full(n, gains[s, 0]), np.full(n, gains[s, 1])
            nr = 0 if ramp_len is None else min(max(int(ramp_len[s]) - ramp_off, 0), n)
            if nr > 0:
                wg[:nr], dg[:nr] = ramp_gains[s, ramp_off: ramp_off + nr, 0], ramp_gains[s, ramp_off: ramp_off + nr, 1]
            out[c] = w * wg + dry * dg
    return out


# ------------------------------------------------------------------------------------------------------------- tail reader
def tail_schedule(state, T, B, layers):
    """delayLineReadAdd's cursor logic (src/MKLNonUniformConvolver.cpp:1653-1688) for T callbacks.  state = [callbacks so far,
    read cursor layer 1, read cursor layer 2, first sample of the last call]; layers = [(PL, oL, D)]: partition size,
    outputDelaySamples, callbacks between a partition filling up and its block reaching the delay line.  After callback c
    (0-based) the writer stands at PL * floor((c + 1 - D) / (PL / B)) (0 before the first block).  The reader starts at
    max(read cursor, writer - oL) and skips the callback when fewer than B samples are there.
    Returns (state, sched [len(layers)][T], -1 = skip)."""
    cb0, R, sched = int(state[0]), [int(state[1]), int(state[2])], []
    for l, (PL, oL, D) in enumerate(layers):
        row = []
        for i in range(T):
            c = cb0 + i
            done = max(0, c + 1 - D) // (PL // B)
            W = done * PL
            start = max(R[l], max(W - oL, 0))
            if start + B > W:
                row.append(-1)
            else:
                row.append(start)
                R[l] = start + B
        sched.append(row)
    return [cb0 + T, R[0], R[1], cb0 * B], sched


def tail_append(ring, layer_out, state, n_ch):
    """what later calls may still read of this call's layer outputs: global samples from the layer's read cursor on, at most one
    ring's worth (the newest), at ring[(global index) % size].  ring: [n_tail][n_ch][size], layer_out: [n_tail][n_ch][n]"""
    ring = ring.copy()
    n_tail, _, size = ring.shape
    n = layer_out.shape[2]
    g0 = int(state[3])
    for l in range(n_tail):
        frm = max(int(state[1 + l]) - g0, n - size, 0)
        for i in range(frm, n):
            ring[l, :, (g0 + i) % size] = layer_out[l, :, i]
    return ring


# -------------------------------------------------------------------------------------------------------------------- rows
def bypass_blend(out, dry, n, on, length, g_end, gains):
    """EQ bypass cross-fade (src/eqprocessor/EQProcessor.Processing.cpp:977-1003): out * g + dry * (1 - g)"""
    res = out.copy()
    with np.errstate(all="ignore"):
        for c in range(out.shape[0]):
            s = c // 2
            if not on[s]:
                continue
            g = np.full(n, np.float64(g_end[s]))
            k = min(int(length[s]), n)
            g[:k] = gains[s, :k]
            res[c, :n] = out[c, :n] * g + dry[c, :n] * (1.0 - g)
    return res


def rows_scale(data, n, gain):
    """scaleBlockFallback (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:93-105): a gain of exactly 1 leaves the row alone"""
    res = data.copy()
    with np.errstate(all="ignore"):
        for c in range(data.shape[0]):
            if gain[c // 2] != 1.0:
                res[c, :n] = data[c, :n] * np.float64(gain[c // 2])
    return res
