"""GPU tests of the output stage (cpq_engine_set_output_stage, cpq_out_*; kernels in convopeq_amd/csrc/out_kernels.hip) through
the C ABI, against tests/out_model.py.

Exact parts.  Headroom, scrub, limiter and clamp are compared bit for bit: every one of their operations is a single rounded
fp64 operation in the reference's order.

DC blocker bar.  The kernel's scan reassociates the two one-pole recurrences, so it is compared with the model run in
np.longdouble; the bar of a channel is 8 x the largest distance, over the run, between the model's own sequential fp64 form and
that long-double run on the same input (tests/test_out_model_cpu.py derives the factor: the emulated scan lies 0.16 - 1.00 x that
distance away).  Both figures are printed by every test.  A callback that holds a value of 1e14 or more (or a NaN) is walked
sequentially in the reference's order and is compared bit for bit.

Release.  The reference's envelope does not return to 1.0 after an attack: in fp64 it stalls at a fixed point just below it
(0.9999999999999556 at 8 kHz) -- see tests/test_out_model_cpu.py.  The release test therefore asks for that value, bit for bit."""
import numpy as np
import pytest

import out_model as M

pytestmark = pytest.mark.gpu

LD = np.longdouble
EXACT = M.HEADROOM | M.LIMITER | M.CLAMP
DC_BAR = 8.0


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def stage_engine(amd, S, flags, B=512, T=16, rate=48000.0, any_calls=True, factor=1):
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=1024, max_blocks_per_call=T, sample_rate=rate,
                            call_mode=amd.CPQ_CALLS_ANY if any_calls else amd.CPQ_CALLS_WHOLE_BLOCKS)
    if factor > 1:
        eng.set_oversampling(factor)
    eng.set_output_stage(flags)
    return eng


def run_calls(eng, x, calls):
    out, o = [], 0
    for n in calls:
        out.append(eng.out_process(np.ascontiguousarray(x[:, o:o + n])))
        o += n
    assert o == x.shape[1]
    return np.concatenate(out, axis=1)


def model_calls(st, x, calls, cb, flags):
    out, o = [], 0
    for n in calls:
        out.append(st.process(x[:, o:o + n], cb, flags))
        o += n
    return np.concatenate(out, axis=1)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def same_bits_or_nan(a, b):
    """same_bits, except that a NaN matches any NaN: IEEE 754 leaves the sign and payload a NaN takes through an operation to
    the implementation, so they are no property of the reference's arithmetic"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and same_bits(np.where(na, 0.0, a), np.where(nb, 0.0, b))


def mixed_streams(S, n, seed=7):
    """stream 0 limits most of the time, stream 1 never, the others now and then"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2 * S, n))
    amp = [1.5, 0.1, 0.45, 0.6, 1.0]
    for s in range(S):
        x[2 * s:2 * s + 2] *= amp[s % 5]
    return x


# ------------------------------------------------------------------------------------------------------- the exact parts
@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 127, 128, 4097))
def test_exact_parts_every_size(amd, S, n):
    x = mixed_streams(S, n)
    eng = stage_engine(amd, S, EXACT)
    y = eng.out_process(x)
    env = [eng.out_read_envelope(s) for s in range(S)]
    eng.close()
    st = M.OutStage(48000.0, S)
    ref = st.process(x, 512, EXACT)
    assert same_bits(y, ref) and env == st.env
    assert np.abs(y).max() <= M.H


def test_exact_parts_five_streams_two_batches(amd):
    S, n = 5, 2048 + 2048 + 77
    x = mixed_streams(S, n, seed=9)
    x[2:4, :2048] *= 0.0                                  # a batch of stream 1 that is digital silence
    eng = stage_engine(amd, S, EXACT)
    y = eng.out_process(x)
    env = [eng.out_read_envelope(s) for s in range(S)]
    eng.close()
    st = M.OutStage(48000.0, S)
    assert same_bits(y, st.process(x, 512, EXACT)) and env == st.env and st.env[1] == 1.0 and st.env[0] < 1.0


@pytest.mark.parametrize("channel", (0, 1))
@pytest.mark.parametrize("pos", (0, 63, 64, 129))
def test_attack_positions_and_one_sided_peaks(amd, pos, channel):
    n = 130
    x = 0.05 * np.random.default_rng(pos).standard_normal((2, n))
    x[channel, pos] = 3.0 if channel == 0 else -3.0
    eng = stage_engine(amd, 1, EXACT)
    y = eng.out_process(x)
    env = eng.out_read_envelope(0)
    eng.close()
    st = M.OutStage(48000.0, 1)
    ref = st.process(x, 512, EXACT)
    assert same_bits(y, ref) and env == st.env[0] < 1.0
    assert same_bits(y[:, :pos], x[:, :pos] * M.H)        # nothing before the attack is touched


@pytest.mark.parametrize("level", (M.CLIP_START, float(np.nextafter(M.CLIP_START, 1.0)), M.THRESHOLD, float(np.nextafter(M.THRESHOLD, 1.0))))
def test_signals_at_clip_start_and_threshold(amd, level):
    n = 300
    x = np.full((2, n), level)
    x[1] = -0.5 * level
    eng = stage_engine(amd, 1, M.LIMITER | M.CLAMP)
    y = eng.out_process(x)
    env = eng.out_read_envelope(0)
    eng.close()
    st = M.OutStage(48000.0, 1)
    assert same_bits(y, st.process(x, 512, M.LIMITER | M.CLAMP)) and env == st.env[0]
    assert (env < 1.0) == (level > M.THRESHOLD)           # at and below the threshold the envelope is never taken down


def test_limiting_stream_between_quiet_ones(amd):
    S, n = 3, 3000
    rng = np.random.default_rng(3)
    x = 0.15 * rng.standard_normal((6, n))
    x[2:4] *= 10.0
    eng = stage_engine(amd, S, EXACT)
    y = eng.out_process(x)
    env = [eng.out_read_envelope(s) for s in range(S)]
    eng.close()
    st = M.OutStage(48000.0, S)
    assert same_bits(y, st.process(x, 512, EXACT)) and env == st.env and env[0] == 1.0 == env[2] and env[1] < 1.0
    for rows in (slice(0, 2), slice(4, 6)):
        assert same_bits(y[rows], x[rows] * M.H)          # the quiet streams: the headroom multiply alone


def test_envelope_carried_across_calls(amd):
    S, calls = 3, [700, 1, 900]
    x = mixed_streams(S, sum(calls), seed=21)
    x[:, 700] = 0.0                                       # the one-sample call releases
    eng = stage_engine(amd, S, EXACT)
    st = M.OutStage(48000.0, S)
    o = 0
    for n in calls:
        y = eng.out_process(np.ascontiguousarray(x[:, o:o + n]))
        assert same_bits(y, st.process(x[:, o:o + n], 512, EXACT))
        assert [eng.out_read_envelope(s) for s in range(S)] == st.env
        o += n
    eng.out_reset()
    assert [eng.out_read_envelope(s) for s in range(S)] == [1.0] * S
    eng.close()


def test_release_at_8_khz_stalls_where_the_reference_does(amd):
    """An attack, then 32768 quiet samples: the envelope ends on the fixed point below 1.0, and a further quiet call (the
    kernel's streaming pass with a gain that is not 1.0) is still the model's, bit for bit."""
    rng = np.random.default_rng(4)
    n = 4 * 8192
    x = 0.01 * rng.standard_normal((2, n + 8192))
    x[0, 0] = 2.5
    eng = stage_engine(amd, 1, EXACT, rate=8000.0)
    st = M.OutStage(8000.0, 1)
    y = run_calls(eng, x, [8192] * 5)
    env = eng.out_read_envelope(0)
    eng.close()
    ref = model_calls(st, x, [8192] * 5, 512, EXACT)
    assert same_bits(y, ref) and env == st.env[0]
    print(f"envelope after {n + 8192} samples at 8 kHz: {env!r}")
    assert env < 1.0 and 1.0 - env < 1e-12 and 1.0 + (env - 1.0) * st.release == env


def test_scrub_writes_what_the_model_writes(amd):
    n = 200
    x = 0.3 * np.random.default_rng(6).standard_normal((2, n))
    x[0, 3], x[1, 10], x[0, 64], x[1, 65] = np.nan, np.inf, -np.inf, 1.0e300
    x[0, 100], x[1, 130], x[0, 131] = 0.99e300, 1.0e300 / M.H * 1.0001, -0.0
    for flags in (M.HEADROOM, EXACT):
        eng = stage_engine(amd, 1, flags)
        y = eng.out_process(x)
        eng.close()
        ref = M.OutStage(48000.0, 1).process(x, 512, flags)
        assert same_bits(y, ref) and np.isfinite(y).all()
        if flags == M.HEADROOM:
            assert y[0, 3] == 0.0 and y[1, 10] == 0.0 and y[0, 64] == 0.0 and y[1, 130] == 0.0 and y[1, 65] == 1.0e300 * M.H
            assert np.signbit(y[0, 131])


@pytest.mark.parametrize("flags", (M.CLAMP, M.HEADROOM | M.CLAMP))
def test_clamp_with_the_limiter_off(amd, flags):
    S, n = 3, 2 * 2048 + 5
    x = mixed_streams(S, n, seed=12)
    x[0, 7] = np.inf
    eng = stage_engine(amd, S, flags)
    y = eng.out_process(x)
    eng.close()
    assert same_bits(y, M.OutStage(48000.0, S).process(x, 512, flags))
    assert np.abs(y).max() == M.H and (np.abs(y) == M.H).sum() > 10


# -------------------------------------------------------------------------------------------------------- the DC blocker
def dc_signals(n, seed=3):
    """three streams: noise / noise on a large offset, sines / a quiet signal, an offset alone / noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.empty((6, n))
    x[0] = 0.25 * rng.standard_normal(n)
    x[1] = 0.9 + 0.05 * rng.standard_normal(n)
    x[2] = 0.4 * np.sin(2 * np.pi * 0.0021 * t + 0.3) + 0.3 * np.sin(2 * np.pi * 0.0517 * t + 1.1) - 0.2
    x[3] = 1.0e-6 * rng.standard_normal(n) + 1.0e-3
    x[4] = -0.75
    x[5] = 0.5 * rng.standard_normal(n)
    return x


def check_dc(y, x, calls, cb, rate, flags=M.DC_BLOCK, label=""):
    """y against the long-double model on x, per channel within DC_BAR x the fp64 model's own distance from it"""
    S = x.shape[0] // 2
    ref = model_calls(M.OutStage(rate, S, LD), x, calls, cb, flags)
    f64 = model_calls(M.OutStage(rate, S), x, calls, cb, flags)
    for ch in range(x.shape[0]):
        dist = float(np.max(np.abs(f64[ch].astype(LD) - ref[ch])))
        err = float(np.max(np.abs(y[ch].astype(LD) - ref[ch])))
        print(f"{label} channel {ch}: fp64 model vs long double {dist:.3e}, kernel vs long double {err:.3e} (bar {DC_BAR * dist:.3e})")
        assert err <= DC_BAR * dist, (ch, err, dist)


@pytest.mark.parametrize("n", (1, 7, 8, 9, 2047, 2049, 3 * 2048 + 5))
def test_dc_blocker_parity_sizes(amd, n):
    x = dc_signals(n)
    eng = stage_engine(amd, 3, M.DC_BLOCK)
    y = eng.out_process(x)
    eng.close()
    check_dc(y, x, [n], 512, 48000.0, label=f"n {n}")


@pytest.mark.parametrize("B,call,rate", ((64, 64 * 40, 44100.0), (512, 441, 44100.0), (512, 512 * 5, 96000.0)))
def test_dc_blocker_parity_callbacks(amd, B, call, rate):
    n = 2560
    calls = [call] * (n // call) + ([n % call] if n % call else [])
    x = dc_signals(n, seed=8)
    eng = stage_engine(amd, 3, M.DC_BLOCK, B=B, T=64, rate=rate)
    y = run_calls(eng, x, calls)
    eng.close()
    check_dc(y, x, calls, B, rate, label=f"callbacks of {min(B, call)}")


def test_dc_blocker_one_call_against_four(amd):
    n = 3 * 2048 + 5
    x = dc_signals(n, seed=5)
    calls = [2047, 1, 2049, n - 4097]
    eng = stage_engine(amd, 3, M.DC_BLOCK | M.HEADROOM)
    one = eng.out_process(x)
    eng.out_reset()
    four = run_calls(eng, x, calls)
    eng.close()
    check_dc(one, x, [n], 512, 48000.0, M.DC_BLOCK | M.HEADROOM, "one call")
    check_dc(four, x, [n], 512, 48000.0, M.DC_BLOCK | M.HEADROOM, "four calls")


@pytest.mark.parametrize("bad", (1.0e16, float("nan")))
def test_dc_guarded_callbacks_reset_the_states_as_the_model_does(amd, bad):
    """A callback of 512 samples at 1e16 drives section 0 past 1e15; one that holds a NaN poisons both sections: the reference
    zeroes such a state at the end of the callback.  Those calls run the guarded path and are the model's bit for bit; the quiet
    callbacks after them start from the model's (reset) states and are back within the bar."""
    B = 512
    x = dc_signals(4 * B, seed=13)
    x[0:2, 0:B] = 1.0e16
    x[4, 0:B] = 1.0e16
    if bad != bad:
        x[:, 0:B] = dc_signals(B, seed=14)
        x[0, 17], x[3, B - 1], x[4, 300] = bad, bad, bad
    calls = [B, B, 2 * B]
    eng = stage_engine(amd, 3, M.DC_BLOCK)
    y = run_calls(eng, x, calls)
    eng.close()
    st = M.OutStage(48000.0, 3)
    ref = model_calls(st, x, calls, B, M.DC_BLOCK)
    touched = [0, 1, 4] if bad == bad else [0, 3, 4]
    assert same_bits_or_nan(y[:, :B][touched], ref[:, :B][touched])
    assert (bad == bad) or np.isnan(y[0, 17:B]).all()
    rest = np.ascontiguousarray(x[:, B:])
    st2, stl = M.OutStage(48000.0, 3), M.OutStage(48000.0, 3, LD)
    for m in (st2, stl):
        m.process(x[:, :B], B, M.DC_BLOCK)             # the states the guards leave
    assert all(st2.dc[ch][0] == 0.0 for ch in touched)
    f64, ld = st2.process(rest, B, M.DC_BLOCK), stl.process(rest, B, M.DC_BLOCK)
    for ch in range(6):
        dist = float(np.max(np.abs(f64[ch].astype(LD) - ld[ch])))
        err = float(np.max(np.abs(y[ch, B:].astype(LD) - ld[ch])))
        print(f"after the guarded callback, channel {ch}: fp64 model {dist:.3e}, kernel {err:.3e} (bar {DC_BAR * dist:.3e})")
        assert err <= DC_BAR * dist


def test_zeros_in_exact_zeros_out(amd):
    eng = stage_engine(amd, 3, M.ALL)
    y = eng.out_process(np.zeros((6, 5000)))
    env = [eng.out_read_envelope(s) for s in range(3)]
    eng.close()
    assert same_bits(y, np.zeros((6, 5000))) and env == [1.0] * 3


# ------------------------------------------------------------------------------------------------------- the whole chain
def _copy_params(po, pa):
    for i in range(20):
        b, o = pa.bands[i], po.bands[i]
        b.frequency, b.gain, b.q, b.enabled, b.type, b.channel_mode = o.frequency, o.gain, o.q, o.enabled, o.type, o.channelMode
    pa.nonlinear_saturation = po.nonlinearSaturation
    return pa


def chain_engine(amd, O, S, F, irs, B, T):
    rate = 48000.0 * F
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=len(irs[0]), max_blocks_per_call=T, sample_rate=rate)
    eng.prepare_to_play(rate, B * T)
    for s in range(S):
        eng.set_impulse(s, irs[2 * s], irs[2 * s + 1])
    eng.set_eq_params(amd.CPQ_ALL_STREAMS, _copy_params(O.eq_params_bench(0.2), amd.eq_params_default()))
    if F > 1:
        eng.set_oversampling(F)
    return eng


@pytest.fixture(scope="module")
def chain(amd, oracle):
    """short IR + EQ + 2x oversampling, three streams: the input, and the rows of an engine that never heard of the stage"""
    O = oracle
    S, F, B, T = 3, 2, 512, 8
    nb = B * T // F
    irs = [O.gen_ir(2000, stream=c // 2, channel=c % 2) for c in range(2 * S)]
    x = 0.25 * np.stack([O.gen_pcm(2 * nb, stream=c // 2, channel=c % 2) for c in range(2 * S)])
    cfg = dict(S=S, F=F, B=B, T=T, nb=nb, irs=irs, x=x)
    eng = chain_engine(amd, O, S, F, irs, B, T)
    cfg["plain"] = np.concatenate([eng.process(np.ascontiguousarray(x[:, o:o + nb])) for o in range(0, x.shape[1], nb)], axis=1)
    eng.close()
    return cfg


def run_chain(amd, oracle, c, flags, metering=0, toggle=False):
    eng = chain_engine(amd, oracle, c["S"], c["F"], c["irs"], c["B"], c["T"])
    if toggle:
        eng.set_output_stage(M.ALL)
    eng.set_output_stage(flags)
    if metering:
        eng.set_metering(metering)
    y = np.concatenate([eng.process(np.ascontiguousarray(c["x"][:, o:o + c["nb"]])) for o in range(0, c["x"].shape[1], c["nb"])], axis=1)
    rec = eng.meter_read_blocks()[0] if metering else None
    eng.close()
    return y, rec


def test_flags_zero_change_nothing(amd, oracle, chain):
    y, _ = run_chain(amd, oracle, chain, 0, toggle=True)
    assert same_bits(y, chain["plain"]) and np.abs(y).max() > 1e-3


def test_whole_chain_is_the_stage_on_the_plain_rows(amd, oracle, chain):
    """CPQ_OUT_ALL at the end of the chain == the stage alone on the rows of the same chain without it: the kernel's own
    cpq_out_process bit for bit, and the model within the DC bar (the limiter does not act on this signal: the bar is the DC
    blocker's, scaled by the headroom multiply the model carries)."""
    c = chain
    cb = c["B"] // c["F"]
    y, _ = run_chain(amd, oracle, c, M.ALL)
    eng = stage_engine(amd, c["S"], M.ALL, B=c["B"], T=c["T"], rate=48000.0 * c["F"], any_calls=False, factor=c["F"])
    alone = run_calls(eng, c["plain"], [c["nb"]] * 2)
    env = [eng.out_read_envelope(s) for s in range(c["S"])]
    eng.close()
    assert same_bits(y, alone)
    assert env == [1.0] * c["S"] and np.abs(c["plain"]).max() * M.H < M.CLIP_START
    check_dc(y, c["plain"], [c["nb"]] * 2, cb, 48000.0, M.ALL, "whole chain")


def test_meters_read_between_scrub_and_limiter(amd, oracle, chain):
    c = chain
    loud_and_peak = 3
    _, rec = run_chain(amd, oracle, c, M.ALL, metering=loud_and_peak)
    rows, _ = run_chain(amd, oracle, c, M.DC_BLOCK | M.HEADROOM)
    eng = stage_engine(amd, c["S"], 0, B=c["B"], T=c["T"], rate=48000.0 * c["F"], any_calls=False, factor=c["F"])
    eng.set_metering(loud_and_peak)
    for o in range(0, rows.shape[1], c["nb"]):
        eng.meter_process(np.ascontiguousarray(rows[:, o:o + c["nb"]]))
    ref, _ = eng.meter_read_blocks()
    eng.close()
    assert rec.shape == ref.shape and rec.shape[1] == rows.shape[1] // (c["B"] // c["F"])
    assert rec.tobytes() == ref.tobytes() and rec["mean_square"].max() > 0.0


def test_pcm_s24_never_exceeds_the_headroom(amd, oracle, chain):
    c = chain
    eng = chain_engine(amd, oracle, c["S"], c["F"], c["irs"], c["B"], c["T"])
    eng.set_gains(amd.CPQ_ALL_STREAMS, 1.0, 200.0)         # loud enough to need the limiter and the clamp
    eng.set_output_stage(M.ALL)
    from convopeq_amd import _capi as K
    raw = eng.process_pcm(np.ascontiguousarray(c["x"][:, :c["nb"]]), K.CPQ_PCM_F64, K.CPQ_PCM_S24, c["nb"])
    env = [eng.out_read_envelope(s) for s in range(c["S"])]
    eng.close()
    b = raw.reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    v = np.where(v >= 1 << 23, v - (1 << 24), v)
    limit = int(round(M.H * 2 ** 23))
    print(f"S24 peak {np.abs(v).max()} of {limit}; envelopes {env}")
    assert np.abs(v).max() <= limit and np.abs(v).max() > limit // 2 and min(env) < 1.0


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_move_no_state(amd):
    """"Calls before prepare", as read here: an engine is usable from cpq_engine_create on (its descriptor carries the rate;
    cpq_engine_prepare only changes it), so there is no un-prepared engine to refuse.  What is not ready is a stage that was
    never set: its own calls give CPQ_ERR_NOT_READY until cpq_engine_set_output_stage has run with flags other than 0."""
    eng = amd.BatchedEngine(1, block_size=512, max_ir_len=1024, max_blocks_per_call=4)
    x = np.full((2, 512), 2.0)
    for call in (lambda: eng.out_process(x), eng.out_reset, lambda: eng.out_read_envelope(0), lambda: eng.out_process_device(0, 0, 512)):
        with pytest.raises(amd.CpqError) as ei:         # before the stage is set
            call()
        assert ei.value.status == -6
    for flags in (16, -1, M.ALL | 32):
        with pytest.raises(amd.CpqError) as ei:
            eng.set_output_stage(flags)
        assert ei.value.status == -1
    eng.set_output_stage(EXACT)
    y = eng.out_process(x)
    env = eng.out_read_envelope(0)
    assert env < 1.0
    for bad in (np.zeros((2, 100)), np.zeros((2, 4 * 512 + 512))):     # not whole callbacks / longer than a call
        with pytest.raises(amd.CpqError) as ei:
            eng.out_process(bad)
        assert ei.value.status == -1
    with pytest.raises(amd.CpqError):
        eng.out_read_envelope(1)
    with pytest.raises(amd.CpqError):
        eng.set_output_stage(64)
    assert eng.out_read_envelope(0) == env                # none of the refusals moved it
    eng.set_output_stage(EXACT)                           # the same flags: no reset
    assert eng.out_read_envelope(0) == env
    eng.set_output_stage(EXACT | M.DC_BLOCK)              # a change of the flags resets
    assert eng.out_read_envelope(0) == 1.0
    eng.out_process(x)
    eng.prepare_to_play(44100.0, 512)                     # and so does prepare
    assert eng.out_read_envelope(0) == 1.0
    eng.out_process(x)
    eng.set_oversampling(2)                               # and a new base rate
    assert eng.out_read_envelope(0) == 1.0
    eng.close()
    assert np.abs(y).max() <= M.H


def test_profiler_lists_k_out_only_when_it_ran(amd):
    eng = amd.BatchedEngine(1, block_size=512, max_ir_len=1024, max_blocks_per_call=4)
    eng.profile_enable(True)
    assert "k_out" not in eng.profile_read()
    eng.set_output_stage(M.ALL)
    eng.out_process(np.zeros((2, 1024)))
    n, ms = eng.profile_read()["k_out"]
    eng.close()
    assert n == 2 and ms > 0.0
