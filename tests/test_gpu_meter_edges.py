"""GPU tests of the meter kernels (convopeq_amd/csrc/meter_kernels.hip) at the places the kernels can go wrong and
test_gpu_metering.py does not reach, through set_metering / meter_process / meter_read_blocks, against
tests/meter_model.py in long double.  The inputs are those of tests/meter_edge_inputs.py; test_meter_edges_cpu.py shows on the
model alone that each of them puts the maximum, the carry or the span where this file needs it.

The bars are test_gpu_metering.py's, through the same two functions (meter_edge_inputs.check_loudness, check_true_peak):
loudness within 8 x the fp64 sequential model's own largest distance from the long-double run, every run at least 4096 samples
per stream; true peak within the model's per-callback bound, the hold the bit-exact replay of the returned peaks.  Where the
kernel is deterministic -- the same samples one callback per call and 16 per call -- the true-peak records are equal bits.

Measured on an MI355X over this file: over its 112 (run, stream, field) loudness comparisons the kernel lies 0.1 x to 6.2 x the
fp64 model's own distance from the long-double run (median 1.2 x).  The worst is mean_square of the -120 dB noise in callbacks of
65: fp64 model 5.7e-25, kernel 3.6e-24, bar 4.6e-24, largest value 6.4e-12; the same stream in callbacks of 64 has the same
kernel distance, 3.8e-24, against a model distance of 1.0e-24 (3.7 x) -- the figure moves with the model's own maximum, not with
the kernel.  Every other comparison is below 3 x (test_gpu_metering.py: 2.75 x).  Worst |true_peak - model| / bound 0.106
(callbacks of 8, 16 per call; test_gpu_metering.py: 0.059).

Mutations of meter_kernels.hip, one at a time, each run once against this file and test_gpu_metering.py (never committed):
  1. stage 0: `d < kMtTile + 4` -> `d < kMtTile + 3`
       here: test_true_peak_at_tile_seams[1024], [1536] fail
       test_gpu_metering.py: fails too (test_digital_silence_is_exactly_zero, test_true_peak_matches_model[2048-2])
  2. histNew: `j < 32 ? hOld[j]` -> `j < 32 ? 0.0`
       here: test_true_peak_tiny_callbacks_one_and_sixteen_per_call[8], [9], [12], [16] fail
       test_gpu_metering.py: passes
  3. k_meter_kweight: the read `pend[par ^ 1]` -> `pend[par]`
       here: test_loudness_of_a_callback_over_three_spans[3000], [4095] and
             test_loudness_of_many_callbacks_per_span[7], [9], [63], [65] fail
       test_gpu_metering.py: fails too (test_loudness_ragged_calls_and_split_invariance)
  4. k_meter_finish: `double hold` restarts from a.hold[s] at every chunk
       here: test_more_than_1024_callbacks_in_one_call fails
       test_gpu_metering.py: passes
(bench_shape_once was left out of the mutated runs of test_gpu_metering.py.)"""
import numpy as np
import pytest

import meter_edge_inputs as E
import meter_model as M
from meter_edge_inputs import check_loudness, check_true_peak, signals

pytestmark = pytest.mark.gpu

LOUD, PEAK = 1, 2
RATE = 48000.0


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def engine(amd, S, B, T, flags, factor=1):
    """CPQ_CALLS_ANY for the loudness cases (ragged calls), and where the block size is not a power of two of at least 64"""
    whole = flags != LOUD and B >= 64 and B & (B - 1) == 0
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=64, max_blocks_per_call=T, sample_rate=RATE * factor,
                            call_mode=amd.CPQ_CALLS_WHOLE_BLOCKS if whole else amd.CPQ_CALLS_ANY)
    if factor > 1:
        eng.set_oversampling(factor)
    eng.set_metering(flags)
    return eng


def feed(eng, x, calls):
    o = 0
    for n in calls:
        eng.meter_process(x[:, o:o + n])
        o += n
    assert o == x.shape[1]


def true_peak_run(amd, x, B, T, per_call=None, factor=1, eng=None):
    """x through a PEAK-only engine in calls of per_call (default T) callbacks of B / factor: the records"""
    cb = B // factor
    own = eng is None
    if own:
        eng = engine(amd, x.shape[0] // 2, B, T, PEAK, factor)
    else:
        eng.meter_reset()
    step = (per_call or T) * cb
    feed(eng, x, [step] * (x.shape[1] // step))
    rec, dropped = eng.meter_read_blocks()
    if own:
        eng.close()
    assert dropped == 0 and rec.shape == (x.shape[0] // 2, x.shape[1] // cb)
    assert not rec["mean_square"].any() and not rec["peak_linear"].any()
    return rec


# ------------------------------------------------------------------------------------------------------------ true peak
@pytest.mark.parametrize("cb", (1024, 1536))
def test_true_peak_at_tile_seams(amd, cb):
    """case 1: the callback's maximum on each of the 32 outputs before and after every seam between 512-sample tiles"""
    x, what = E.seam_case(cb)
    rec = true_peak_run(amd, x, cb, 2)
    check_true_peak(rec, x, cb, label=f"seams cb {cb}")
    assert rec["true_peak"][:, 1].min() > 0.25 and rec["true_peak"][:, 0].max() < 1e-4


@pytest.mark.parametrize("cb", (516, 520, 1000))
def test_true_peak_in_a_short_last_tile(amd, cb):
    """case 2: a last tile of 4, 8 and 488 samples; the maximum in it, in the callback's last 16 outputs, before the seam"""
    x, _ = E.short_tile_case(cb)
    rec = true_peak_run(amd, x, cb, 2)
    check_true_peak(rec, x, cb, label=f"short tile cb {cb}")
    assert rec["true_peak"][:, 1].min() > 0.25


@pytest.mark.parametrize("cb", (64, 512))
def test_true_peak_at_the_callback_end_and_after(amd, cb):
    """case 3: an impulse 1 .. 20 samples before the end of callback k = 0, of k = 1 and of a call's last callback: that
    callback (the zero future) and the ones after it (the history, from the call or from hOld)"""
    x, _ = E.end_case(cb)
    rec = true_peak_run(amd, x, cb, 3)
    check_true_peak(rec, x, cb, label=f"callback end cb {cb}")


@pytest.mark.parametrize("cb", E.TINY_CBS)
def test_true_peak_tiny_callbacks_one_and_sixteen_per_call(amd, cb):
    """case 4: callbacks of 8 .. 33 samples.  One per call (n < 32: histNew mixes the old history and the call) and 16 per
    call: both within the bound of the model, and equal to the bit."""
    x, _ = E.tiny_case(cb)
    eng = engine(amd, 2, cb, E.TINY_T, PEAK)
    one = true_peak_run(amd, x, cb, E.TINY_T, per_call=1, eng=eng)
    many = true_peak_run(amd, x, cb, E.TINY_T, eng=eng)
    eng.close()
    check_true_peak(one, x, cb, label=f"tiny cb {cb}, one per call")
    check_true_peak(many, x, cb, label=f"tiny cb {cb}, 16 per call")
    assert one.tobytes() == many.tobytes()
    assert one["true_peak"].max() > 0.25


def test_true_peak_one_sided_and_neighbouring_streams(amd):
    """case 5: the peak on the left channel only (stream 1) and the right only (stream 4); the streams beside them stay at
    the model's floor-level values"""
    cb = 1024
    x, hot = E.sided_case(cb)
    rec = true_peak_run(amd, x, cb, 2)
    check_true_peak(rec, x, cb, label="one-sided")
    for s in range(6):
        if s in hot:
            assert rec["true_peak"][s, 1:].min() > 0.25
        else:
            assert rec["true_peak"][s].max() < 1e-3


def test_more_than_1024_callbacks_in_one_call(amd):
    """case 6: 2056 callbacks of 8 per call, so k_meter_finish walks three chunks; two calls with a read of 100 records between
    them, so the ring's write position passes 4095 -> 0 inside the second"""
    B, T, S = E.LONG_B, E.LONG_T, 2
    x = E.long_call_case()
    eng = engine(amd, S, B, T, LOUD | PEAK)
    ring, recs = M.Ring(), []
    for call in range(2):
        eng.meter_process(x[:, call * T * B:(call + 1) * T * B])
        model_dropped = sum(0 if ring.push(call * T + k) else 1 for k in range(T))
        rec, dropped = eng.meter_read_blocks(100 if call == 0 else M.RING)
        want = [ring.pop() for _ in range(min(100 if call == 0 else M.RING, ring.w - ring.r))]
        assert dropped == model_dropped == 0
        for s in range(S):
            assert np.array_equal(rec["block_index"][s], np.array(want, dtype=np.uint64)), (call, s)
        recs.append(rec)
    eng.close()
    assert recs[0].shape == (S, 100) and recs[1].shape == (S, 2 * T - 100)
    assert (ring.r - recs[1].shape[1]) % M.RING + recs[1].shape[1] > M.RING          # the slots read were 100 .. 4095, 0 .. 15
    rec = np.concatenate(recs, axis=1)
    assert np.array_equal(rec["block_index"], np.broadcast_to(np.arange(2 * T, dtype=np.uint64), (S, 2 * T)))
    check_true_peak(rec, x, B, label="2056 callbacks per call")                      # and the hold, to the bit, over it all
    check_loudness(rec, x, B, RATE, [T * B, T * B], label="2056 callbacks per call")


@pytest.mark.parametrize("B,factor", ((64, 8), (512, 4)))
def test_true_peak_of_base_rate_callbacks_under_oversampling(amd, B, factor):
    """case 7: the meters see base-rate rows in callbacks of block_size / factor: 8 (the tiny input) and 128 (the
    callback-end input)"""
    cb = B // factor
    if cb == 8:
        x, _ = E.tiny_case(cb)
        T = E.TINY_T
    else:
        x, _ = E.end_case(cb)
        T = 3
    rec = true_peak_run(amd, x, B, T, factor=factor)
    check_true_peak(rec, x, cb, label=f"B {B} factor {factor}")
    assert rec["true_peak"].max() > 0.25


# ----------------------------------------------------------------------------------------------------------- K-weighting
def loudness_run(amd, x, B, T, calls, read_every_call=False, eng=None):
    own = eng is None
    if own:
        eng = engine(amd, x.shape[0] // 2, B, T, LOUD)
    else:
        eng.meter_reset()
    if read_every_call:
        recs, o = [], 0
        for n in calls:
            eng.meter_process(x[:, o:o + n])
            rec, dropped = eng.meter_read_blocks()
            assert dropped == 0
            recs.append(rec)
            o += n
        rec = np.concatenate(recs, axis=1)
    else:
        feed(eng, x, calls)
        rec, dropped = eng.meter_read_blocks()
        assert dropped == 0
    if own:
        eng.close()
    assert not rec["true_peak"].any() and not rec["true_peak_hold"].any()
    return rec


@pytest.mark.parametrize("B", sorted(E.THREE_SPAN))
def test_loudness_of_a_callback_over_three_spans(amd, B):
    """case 8: callbacks of 3000 and 4095 samples in calls of three; the middle span of a callback reads the pending sum of
    the span before it and writes its own"""
    whole, ragged = E.THREE_SPAN[B]
    eng = engine(amd, 4, B, 3, LOUD)
    for calls in (whole, ragged):
        if calls:
            x = signals(sum(calls), seed=81 + len(calls))
            rec = loudness_run(amd, x, B, 3, calls, eng=eng)
            check_loudness(rec, x, B, RATE, calls, label=f"three spans B {B}, {len(calls)} calls")
    eng.close()


@pytest.mark.parametrize("B", E.MANY_BLOCKS)
def test_loudness_of_many_callbacks_per_span(amd, B):
    """case 9: up to 2048 callbacks in one span, dealt to the four waves; callbacks shorter than a wave, than a lane's chunk"""
    calls = E.many_calls(B)
    x = signals(sum(calls), seed=91)
    rec = loudness_run(amd, x, B, (max(calls) + B - 1) // B, calls, read_every_call=True)
    check_loudness(rec, x, B, RATE, calls, label=f"many callbacks B {B}")


def test_loudness_call_lengths_at_the_carry_edges(amd):
    """case 10: calls of 1 .. 4097 samples: the span's last sample on lane 0 element 0, element 7, a wave's last lane, the
    span's last lane; then an order that ends on three calls of one sample"""
    B, T = 512, 16
    eng = engine(amd, 4, B, T, LOUD)
    for i, calls in enumerate((E.CARRY_CALLS, E.CARRY_CALLS_ONES_LAST)):
        x = signals(sum(calls), seed=101 + i)
        rec = loudness_run(amd, x, B, T, calls, eng=eng)
        check_loudness(rec, x, B, RATE, calls, label=f"carry edges, order {i}")
    eng.close()


def test_loudness_scrubbed_samples_on_the_carries(amd):
    """case 11: NaN, +Inf, 1e300, -1.5e300 as the last two samples of a call and as samples 2046 .. 2048 of a longer one: the
    carried x1, x2 are the scrubbed 0"""
    B, T = 512, 16
    bad, calls, _ = E.scrub_case()
    rec = loudness_run(amd, bad, B, T, calls)
    for f in ("mean_square", "peak_linear"):
        assert np.isfinite(rec[f]).all(), f
    check_loudness(rec, M.scrub(bad), B, RATE, calls, label="scrubbed carries")
