"""Inputs of the meter edge tests, shared by the CPU checks (test_meter_edges_cpu.py: on the model alone, each input does
what its GPU test relies on) and the GPU tests (test_gpu_meter_edges.py).  numpy and tests/meter_model.py only.  It also holds
what test_gpu_metering.py and the edge tests share: signals(), and the two bars check_loudness() and check_true_peak().

True peak is one max per callback, so an error of k_meter_true_peak shows only where the model's maximum sits on the output
the kernel gets wrong.  planted() writes a short shape into noise at `floor`; peak_trace() says where the model's maximum of
every callback lies (output index 0 .. 4 cb - 1, 4 outputs per input sample).  On the model, (0.9,) at input p puts the
maximum at output 4 p + 61 (0.2806, the runner-up at 4 p + 58 is 0.15 % lower) and (0.9, 0.45) at 4 p + 58, an even index
(the runner-up 6e-5 lower: those inputs use a floor of 1e-6); an output beyond the callback's end is never formed, and the
last 16 input samples of a callback are interpolated against a zero future.

The constants restate the kernels' geometry (meter_kernels.hip): kMtTile, kMwSpan = kMwThreads * kMeterChunk, kMfChunk."""
import numpy as np

import meter_model as M

TILE = 512                  # base-rate samples of a true-peak workgroup
SPAN = 2048                 # samples of a K-weighting span
FINISH_CHUNK = 1024         # callbacks k_meter_finish walks at a time
IMP, PAIR = (0.9,), (0.9, 0.45)
LOBE = 0.2806               # the model's peak of IMP with its whole response inside the callback
BAD = (np.nan, np.inf, 1.0e300, -1.5e300)


# ------------------------------------------------- shared with test_gpu_metering.py: the signals, the references, the bars
def signals(n, seed=11):
    """four stereo streams: noise, a multi-sine, noise with silent stretches, noise at -120 dB"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.empty((8, n))
    x[0:2] = 0.25 * rng.standard_normal((2, n))
    for ch in range(2):
        x[2 + ch] = sum(a * np.sin(2 * np.pi * f * t + p + ch) for a, f, p in ((0.4, 0.0021, 0.3), (0.3, 0.0517, 1.1), (0.2, 0.2203, 2.0)))
    x[4:6] = 0.5 * rng.standard_normal((2, n))
    gate = (np.arange(n) // 700) % 3 == 1
    x[4:6, gate] = 0.0
    x[6:8] = 1.0e-6 * rng.standard_normal((2, n))
    return x


def loud_model(x, cb, rate, calls=None):
    """records of the model in long double and in fp64: (ms [K, S], pk [K, S]) each; calls = the call lengths (ragged ends)"""
    S = x.shape[0] // 2
    out = []
    for dt in (np.longdouble, np.float64):
        m = M.LoudnessMeter(rate, S, dt)
        recs, o = [], 0
        for n in (calls or [x.shape[1]]):
            recs += m.process(x[:, o:o + n], cb)
            o += n
        out.append((np.stack([r[0] for r in recs]), np.stack([r[1] for r in recs])))
        assert [r[2] for r in recs] == list(range(len(recs)))
    return out


def check_loudness(rec, x, cb, rate, calls=None, label="", tail=None):
    """rec against the model on x; tail: rec holds only the last `tail` records of the run.  Returns the distances the bars are
    made of: {field: [per stream] largest |fp64 model - long-double model|}."""
    (ms_l, pk_l), (ms_d, pk_d) = loud_model(x, cb, rate, calls)
    if tail is not None:
        ms_l, pk_l, ms_d, pk_d = ms_l[-tail:], pk_l[-tail:], ms_d[-tail:], pk_d[-tail:]
    K = ms_l.shape[0]
    assert rec.shape[1] == K, (rec.shape, K)
    dists = {"mean_square": [], "peak_linear": []}
    for s in range(rec.shape[0]):
        for name, ref, f64 in (("mean_square", ms_l[:, s], ms_d[:, s]), ("peak_linear", pk_l[:, s], pk_d[:, s])):
            dist = float(np.max(np.abs(f64.astype(np.longdouble) - ref)))
            err = float(np.max(np.abs(rec[name][s].astype(np.longdouble) - ref)))
            scale = float(np.max(np.abs(ref)))
            print(f"{label} stream {s} {name}: fp64 model vs long double {dist:.3e}, kernel vs long double {err:.3e} "
                  f"(bar {8 * dist:.3e}, largest value {scale:.3e})")
            assert err <= 8 * dist, (s, name, err, dist)
            dists[name].append(dist)
    assert np.array_equal(rec["block_index"][0], np.arange(K, dtype=np.uint64) + rec["block_index"][0][0])
    return dists


def check_true_peak(rec, x, cb, label=""):
    K = x.shape[1] // cb
    assert rec.shape[1] == K
    worst = 0.0
    for s in range(rec.shape[0]):
        det = M.TruePeakDetector()
        for k in range(K):
            tp, _, bound = det.process_block(x[2 * s:2 * s + 2, k * cb:(k + 1) * cb])
            err = abs(float(rec["true_peak"][s, k]) - tp)
            assert err <= bound, (s, k, err, bound, tp)
            worst = max(worst, err / bound if bound else 0.0)
        # the hold is the replay of the peaks the engine returned, to the bit
        assert np.array_equal(rec["true_peak_hold"][s], np.array(M.hold_replay(rec["true_peak"][s].tolist()))), s
    print(f"{label}: worst |true_peak - model| / bound = {worst:.3f}")


def planted(n, cb, positions, shape, floor=1e-4, seed=0):
    """one row [n]: noise at `floor`, `shape` written at sample k * cb + p for every (k, p) of positions"""
    x = floor * np.random.default_rng(seed).standard_normal(n)
    for k, p in positions:
        at = k * cb + p
        x[at:at + len(shape)] = shape
    return x


def peak_trace(x, cb):
    """x [2, n], one stereo stream -> per callback (peak, output index of the maximum, its channel): TruePeakDetector's
    processBlock in fp64, keeping where the maximum was (the margins relied on are many orders above fp64 rounding)"""
    st = M.tp_stages()
    x = M.scrub(x)
    hist = [[np.zeros(s["history_up_keep"]) for _ in range(2)] for s in st]
    out = []
    for k in range(x.shape[1] // cb):
        best = (0.0, 0, 0)
        for ch in range(2):
            o0, hist[0][ch], _, _ = M.interpolate(st[0], hist[0][ch], x[ch, k * cb:(k + 1) * cb], dtype=np.float64)
            o1, hist[1][ch], _, _ = M.interpolate(st[1], hist[1][ch], o0, dtype=np.float64)
            a = np.abs(o1)
            i = int(a.argmax())
            if a[i] > best[0]:
                best = (float(a[i]), i, ch)
        out.append(best)
    return out


def stereo(rows):
    """rows: list of (left, right) -> [2 S, n]"""
    return np.stack([r for pair in rows for r in pair])


# ------------------------------------------------------------------------------------------------------------ true peak
def seam_case(cb):
    """case 1: (x [2 S, 4 cb], what) -- two calls of two callbacks, the shape planted in the second callback of each; one
    stream per (seam, shape, p), p = t0 - 23 .. t0 - 8, on the left channel for even p and the right for odd p.
    what[s] = (t0, shape, p)."""
    rows, what = [], []
    for t0 in range(TILE, cb, TILE):
        for shape in (IMP, PAIR):
            for p in range(t0 - 23, t0 - 7):
                sig = planted(4 * cb, cb, [(1, p), (3, p)], shape, 1e-6, seed=1000 + len(rows))
                quiet = planted(4 * cb, cb, [], shape, 1e-6, seed=2000 + len(rows))
                rows.append((sig, quiet) if p % 2 == 0 else (quiet, sig))
                what.append((t0, shape, p))
    return stereo(rows), what


def short_tile_case(cb):
    """case 2 (cb = 516, 520, 1000: the last tile holds 4, 8, 488 samples): (x [6, 4 cb], want) -- IMP in the second callback
    of each call; want[s] = (lo, hi): the maximum of the planted callbacks lies at an output index in [lo, hi):
      stream 0 in the last tile, stream 1 in the callback's last 16 outputs, stream 2 in the 8 outputs before the last seam"""
    seam = TILE * ((cb - 1) // TILE)
    ps = (max(seam - 15 + (cb - seam) // 2, seam - 15), cb - 16, seam - 16)
    want = ((4 * seam, 4 * cb), (4 * cb - 16, 4 * cb), (4 * seam - 8, 4 * seam))
    rows = [(planted(4 * cb, cb, [(1, p), (3, p)], IMP, seed=3000 + i), planted(4 * cb, cb, [], IMP, seed=3100 + i))
            for i, p in enumerate(ps)]
    return stereo(rows), want


END_BACKS = tuple(range(1, 21))


def end_case(cb, T=3):
    """case 3: (x [2 * 20, 4 T cb], plants) -- stream i has IMP at cb - back, back = i + 1, in callbacks `plants`: callback 0
    (k = 0 of the first call), T + 1 (k = 1 of the second call) and 3 T - 1 (the last callback of the third call, so the
    fourth call finds it in its history); calls are T callbacks long"""
    plants = (0, T + 1, 3 * T - 1)
    rows = []
    for i, back in enumerate(END_BACKS):
        pos = [(k, cb - back) for k in plants]
        rows.append((planted(4 * T * cb, cb, pos if i % 2 == 0 else [], IMP, seed=4000 + i),
                     planted(4 * T * cb, cb, pos if i % 2 == 1 else [], IMP, seed=4100 + i)))
    return stereo(rows), plants


TINY_CBS = (8, 9, 12, 16, 23, 24, 25, 31, 32, 33)
TINY_T = 16


def tiny_case(cb, calls=4):
    """case 4: (x [4, calls * 16 * cb], plants) -- IMP every five callbacks at offsets that walk back from the callback's last
    sample; plants[s] = [(k, p)].  Stream 0 plants left, stream 1 right and two callbacks later."""
    K = calls * TINY_T
    plants = [[(k, (cb - 1 - 7 * i) % cb) for i, k in enumerate(range(2 + 2 * s, K - 3, 5))] for s in range(2)]
    n = K * cb
    rows = [(planted(n, cb, plants[0], IMP, seed=5000 + cb), planted(n, cb, [], IMP, seed=5100 + cb)),
            (planted(n, cb, [], IMP, seed=5200 + cb), planted(n, cb, plants[1], IMP, seed=5300 + cb))]
    return stereo(rows), plants


def sided_case(cb=1024):
    """case 5: (x [12, 4 cb], planted streams) -- IMP before the seam, in stream 1 on the left channel only and in stream 4
    on the right only; streams 0, 2, 3, 5 and the planted streams' other channel are at the floor"""
    pos = [(1, TILE - 16), (2, 100), (3, cb - 30)]
    rows = []
    for s in range(6):
        left = planted(4 * cb, cb, pos if s == 1 else [], IMP, seed=6000 + s)
        right = planted(4 * cb, cb, pos if s == 4 else [], IMP, seed=6100 + s)
        rows.append((left, right))
    return stereo(rows), (1, 4)


LONG_B, LONG_T = 8, 2056


def long_call_case():
    """case 6: x [4, 2 * 2056 * 8] -- two calls of 2056 callbacks of 8: 0.25-rms noise and a multi-sine (signals()' first two
    kinds, so the loudness bar has something to stand on) with a 3.0 impulse every 97 or 103 callbacks: the hold that enters
    callback 1024 of a call is an impulse's, well above the peaks that follow it"""
    n = 2 * LONG_T * LONG_B
    rng = np.random.default_rng(61)
    t = np.arange(n)
    x = np.empty((4, n))
    x[0:2] = 0.25 * rng.standard_normal((2, n))
    for ch in range(2):
        x[2 + ch] = sum(a * np.sin(2 * np.pi * f * t + p + ch) for a, f, p in ((0.4, 0.0021, 0.3), (0.3, 0.0517, 1.1), (0.2, 0.2203, 2.0)))
    for s, step in ((0, 97), (1, 103)):
        for k in range(5, 2 * LONG_T, step):
            x[2 * s + k % 2, k * LONG_B + k % LONG_B] = 3.0
    return x


# ----------------------------------------------------------------------------------------------------------- K-weighting
def span_counts(calls, cb):
    """spans of 2048 (counted from the call's first sample) that each callback of each call lies over, from the arithmetic
    alone: a call of n samples has callbacks [k cb, min((k + 1) cb, n))"""
    out = []
    for n in calls:
        for a in range(0, n, cb):
            b = min(a + cb, n)
            out.append((b - 1) // SPAN - a // SPAN + 1)
    return out


THREE_SPAN = {3000: ([9000, 9000], [9000, 3000, 7001, 5000, 8999, 1]),
              4095: ([12285, 12285], None)}                    # block size -> (calls of three callbacks, a ragged sequence)

MANY_BLOCKS = (1, 2, 7, 8, 9, 63, 64, 65)


def many_calls(B):
    """case 9: call lengths; a read follows every call, so the ring of 4096 never fills"""
    return [2500, 4090] if B == 1 else [2500, 4100, 3333]


CARRY_CALLS = [1, 2, 7, 8, 9, 15, 16, 17, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097]
CARRY_CALLS_ONES_LAST = [2049, 9, 2047, 17, 513, 7, 2048, 15, 511, 8, 16, 512, 2, 1, 1, 1]


def scrub_case():
    """case 11: (bad [4, n], calls) -- signals(n)[:4] with NaN, +Inf, 1e300 and -1.5e300 as the last and second-to-last sample
    of calls 0 and 2, and as samples 2046, 2047, 2048 of calls 1 and 2; every row gets every value somewhere"""
    calls = [1000, 3000, 2500, 600, 37, 512]
    x = signals(sum(calls), seed=71)[:4].copy()
    start = np.concatenate([[0], np.cumsum(calls)])
    spots = [start[1] - 1, start[1] - 2, start[1] + 2046, start[1] + 2047, start[1] + 2048,
             start[2] + 2046, start[2] + 2047, start[3] - 2, start[3] - 1]
    for q, at in enumerate(spots):
        for r in range(4):
            x[r, at] = BAD[(q + r) % 4]
    return x, calls, spots
