"""GPU tests of the half-band oversampler (CustomInputOversampler around the routing): the stage kernels against
tests/os_model.py, ragged calls, the round trip, the guards and per-stream state machine, the silence path, and the whole
DSPCore chain at the oversampled rate against the oracle's restatements."""
import numpy as np
import pytest

import os_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def signals(n_streams, n, seed=5):
    """different signals per stream, |x| <= 1: noise, multi-sine, noise with silent stretches"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.empty((2 * n_streams, n))
    for c in range(2 * n_streams):
        kind = (c // 2) % 3
        if kind == 0:
            x[c] = rng.uniform(-1.0, 1.0, n)
        elif kind == 1:
            x[c] = 0.3 * np.sin(2 * np.pi * 0.013 * (c + 1) * t) + 0.25 * np.sin(2 * np.pi * 0.31 * t + c)
        else:
            x[c] = rng.uniform(-0.5, 0.5, n) * (np.sin(2 * np.pi * t / 1500.0) > 0)
    return x


def any_engine(amd, S, F, os_type, max_base=4096, rate=48000.0):
    eng = amd.BatchedEngine(S, block_size=480, max_ir_len=1024, max_blocks_per_call=(max_base * F + 479) // 480,
                            call_mode=amd.CPQ_CALLS_ANY, sample_rate=rate * F)
    eng.set_oversampling(F, os_type)
    return eng


RAGGED = [1, 7, 441, 480, 4096, 480, 7]


@pytest.mark.parametrize("F", [2, 4, 8])
@pytest.mark.parametrize("os_type", [M.IIR, M.LINEAR_PHASE])
def test_up_down_match_model_ragged(amd, F, os_type):
    S = 3
    n = sum(RAGGED)
    x = signals(S, n)
    eng = any_engine(amd, S, F, os_type)
    models = [M.Oversampler(F, os_type) for _ in range(S)]
    # split == whole holds bit for bit when the silence path discards nothing: here it is taken only on all-zero input
    # and history, where it equals the computed path.  (At 8x the up output does hold samples in (0, 1e-19): the far
    # taps' response to the first samples; no down call of them takes the silence path.)
    assert np.all((x == 0.0) | (np.abs(x) >= 1e-19))
    ups, downs, o = [], [], 0
    for m in RAGGED:
        u = eng.os_up(x[:, o:o + m])
        ref_u = np.concatenate([models[s].up(x[2 * s:2 * s + 2, o:o + m]) for s in range(S)])
        assert np.abs(u - ref_u).max() <= 1e-13, (m, np.abs(u - ref_u).max())
        d = eng.os_down(ref_u)
        ref_d = np.concatenate([models[s].down(ref_u[2 * s:2 * s + 2]) for s in range(S)])
        assert np.abs(d - ref_d).max() <= 1e-13, (m, np.abs(d - ref_d).max())
        ups.append(u)
        downs.append(d)
        o += m
    for s in range(S):
        t = eng.os_telemetry(s)
        assert t["corruption_events"] == 0 and t["auto_clears"] == 0 and t["hard_fallback"] == 0
        assert models[s].silent_discards == 0
    u_all = np.concatenate(ups, axis=1)
    # the same samples in one call: each output is one fixed-order FMA chain over the same operands
    one = any_engine(amd, S, F, os_type, max_base=n)
    u1 = one.os_up(x)
    assert np.array_equal(u1, u_all)
    d1 = one.os_down(np.concatenate(ups, axis=1))
    eng2 = any_engine(amd, S, F, os_type)
    d2 = []
    for u in ups:
        d2.append(eng2.os_down(u))
    assert np.array_equal(d1, np.concatenate(d2, axis=1))
    for e in (eng, one, eng2):
        e.close()


@pytest.mark.parametrize("F,os_type", [(8, M.IIR), (2, M.LINEAR_PHASE), (4, M.LINEAR_PHASE)])
def test_round_trip_is_a_delay(amd, F, os_type):
    """No model: up then down of a multi-sine below 0.4 fs is the input delayed by cpq_os_latency (a fractional delay,
    built analytically), times the reference's passband gain of 0.75 per stage (interpolateStage writes the centre
    phase as 0.5 x instead of 2 x 0.5 x, so each up / down pair passes 1/2 + 1/4 of the signal)."""
    S, n = 2, 16384
    rng = np.random.default_rng(11)
    f = rng.uniform(0.002, 0.4, (2 * S, 6))
    ph = rng.uniform(0, 2 * np.pi, (2 * S, 6))
    t = np.arange(n, dtype=np.float64)
    x = np.stack([(0.15 * np.sin(2 * np.pi * f[c][:, None] * t + ph[c][:, None])).sum(0) for c in range(2 * S)])
    L = amd.os_latency(F, os_type)
    assert L == M.latency(F, os_type) and (F < 8 or L != int(L))
    ref = np.stack([(0.15 * np.sin(2 * np.pi * f[c][:, None] * (t - L) + ph[c][:, None])).sum(0) for c in range(2 * S)])
    gain = 0.75 ** {2: 1, 4: 2, 8: 3}[F]
    eng = any_engine(amd, S, F, os_type)
    y = np.concatenate([eng.os_down(eng.os_up(x[:, o:o + 4096])) for o in range(0, n, 4096)], axis=1)
    skip = 4 * int(L) + 64
    for c in range(2 * S):
        assert rms(y[c, skip:] - gain * ref[c, skip:]) <= 1e-4 * rms(gain * ref[c, skip:])
    eng.close()


def test_guards_and_state_machine(amd):
    F, T, S, m = 8, M.IIR, 3, 480
    calls = [m] * 12
    n = m * len(calls)
    clean = signals(S, n, seed=3)
    x = clean.copy()
    # stream 1: NaN, Inf and 1e300, one at the last sample of a call (its centre tap reaches it in the NEXT call)
    x[2, 100] = np.nan
    x[3, m + 300] = np.inf
    x[2, 3 * m - 1] = np.nan
    x[3, 5 * m + 17] = 1e300
    eng = any_engine(amd, S, F, T)
    models = [M.Oversampler(F, T) for _ in range(S)]
    out, ref, tel = [], [], []
    o = 0
    for k, mm in enumerate(calls):
        xb = x[:, o:o + mm]
        out.append(eng.os_down(eng.os_up(xb)))
        ref.append(np.concatenate([models[s].down(models[s].up(xb[2 * s:2 * s + 2])) for s in range(S)]))
        t = eng.os_telemetry(1)
        assert (t["corruption_events"], t["auto_clears"], t["hard_fallback"], t["consecutive_auto_clears"]) == \
            (models[1].events, models[1].auto_clears, int(models[1].hard), models[1].consecutive), (k, t)
        assert np.abs(out[-1] - ref[-1]).max() <= 1e-13, k
        o += mm
    assert models[1].auto_clears >= 4 and models[1].events >= 4
    # the NaN at the end of call 2 is flagged in call 3 and silences call 3 (auto-clear in processDown of call 3)
    assert np.all(out[3][2:4] == 0.0) and not np.all(out[2][2:4] == 0.0)
    # the other streams are bit-identical to a clean run
    ec = any_engine(amd, S, F, T)
    oc = np.concatenate([ec.os_down(ec.os_up(clean[:, i * m:(i + 1) * m])) for i in range(len(calls))], axis=1)
    got = np.concatenate(out, axis=1)
    for c in (0, 1, 4, 5):
        assert np.array_equal(got[c], oc[c])
    for s in (0, 2):
        assert eng.os_telemetry(s)["corruption_events"] == 0
    eng.close()
    ec.close()


def test_hard_fallback_latches_and_reset_clears(amd):
    F, T, S, m = 4, M.LINEAR_PHASE, 2, 480
    x = signals(S, 10 * m, seed=9)
    for k in range(4):                          # four consecutive corrupted blocks of stream 0
        x[0, k * m + 10] = np.nan
    eng = any_engine(amd, S, F, T)
    models = [M.Oversampler(F, T) for _ in range(S)]
    for k in range(7):
        xb = x[:, k * m:(k + 1) * m]
        y = eng.os_down(eng.os_up(xb))
        r = np.concatenate([models[s].down(models[s].up(xb[2 * s:2 * s + 2])) for s in range(S)])
        assert np.abs(y - r).max() <= 1e-13, k
        t = eng.os_telemetry(0)
        assert t["hard_fallback"] == int(models[0].hard) and t["auto_clears"] == models[0].auto_clears, (k, t)
        if k >= 3:
            assert t["hard_fallback"] == 1 and np.all(y[0:2] == 0.0)   # the documented silence
        assert not np.all(y[2:4] == 0.0)
    assert eng.os_telemetry(0)["consecutive_auto_clears"] == 4
    eng.os_reset()
    for s in range(S):
        models[s].reset()
    t = eng.os_telemetry(0)
    assert t["hard_fallback"] == 0 and t["consecutive_auto_clears"] == 0 and t["auto_clears"] == 4   # counters stay
    for k in range(7, 10):
        xb = x[:, k * m:(k + 1) * m]
        y = eng.os_down(eng.os_up(xb))
        r = np.concatenate([models[s].down(models[s].up(xb[2 * s:2 * s + 2])) for s in range(S)])
        assert np.abs(y - r).max() <= 1e-13 and not np.all(y[0:2] == 0.0)
    eng.set_oversampling(F, T)                  # set_oversampling also clears the counters
    assert eng.os_telemetry(0)["auto_clears"] == 0 and eng.os_telemetry(0)["corruption_events"] == 0
    eng.close()


@pytest.mark.parametrize("F,os_type", [(2, M.IIR), (8, M.LINEAR_PHASE)])
def test_silence_path(amd, F, os_type):
    S, m = 2, 480
    x = signals(S, 16 * m, seed=21)
    x[:, 3 * m:] = 0.0
    eng = any_engine(amd, S, F, os_type)
    models = [M.Oversampler(F, os_type) for _ in range(S)]
    first_gpu = first_ref = None
    for k in range(16):
        xb = x[:, k * m:(k + 1) * m]
        y = eng.os_down(eng.os_up(xb))
        r = np.concatenate([models[s].down(models[s].up(xb[2 * s:2 * s + 2])) for s in range(S)])
        assert np.abs(y - r).max() <= 1e-13
        if first_gpu is None and np.all(y == 0.0):
            first_gpu = k
        if first_ref is None and np.all(r == 0.0):
            first_ref = k
        if first_ref is not None:
            assert np.all(y == 0.0), k          # exactly zero from then on
    assert first_ref is not None and first_gpu == first_ref and first_ref > 3
    eng.close()


def _copy_params(po, pa):
    for i in range(20):
        b, o = pa.bands[i], po.bands[i]
        b.frequency, b.gain, b.q, b.enabled, b.type, b.channel_mode = o.frequency, o.gain, o.q, o.enabled, o.type, o.channelMode
    pa.nonlinear_saturation = po.nonlinearSaturation
    pa.total_gain_db = po.totalGainDb
    pa.filter_structure = po.filterStructure
    pa.agc_enabled = po.agcEnabled
    return pa


def chain_engine(amd, O, S, F, os_type, order, irs, B, T):
    rate = 48000.0 * F
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=len(irs[0]), max_blocks_per_call=T, sample_rate=rate)
    eng.prepare_to_play(rate, B * T)
    for s in range(S):
        eng.set_impulse(s, irs[2 * s], irs[2 * s + 1])
    eng.set_eq_params(amd.CPQ_ALL_STREAMS, _copy_params(O.eq_params_bench(0.2), amd.eq_params_default()))
    eng.set_convproc_params(amd.CPQ_ALL_STREAMS, mix=1.0)
    eng.set_conv_level(amd.CPQ_LEVEL_PROCESSOR)
    eng.set_order(order)
    # the sequential cascade kernels reproduce the reference recurrences operation for operation: at 384 kHz the output
    # filter's 20 Hz high-pass (poles at |z| = 0.9997) would amplify the time-parallel kernels' last-bit differences
    eng.set_eq_mode(amd.CPQ_EQ_MODE_SEQUENTIAL)
    eng.set_outfilter_params(amd.CPQ_ALL_STREAMS, int(order == amd.CPQ_ORDER_EQ_THEN_CONV), 1, 0, 1)
    eng.enable_output_filter(True)
    if F > 1:
        eng.set_oversampling(F, os_type)
    return eng


@pytest.mark.parametrize("F,os_type,eq_first", [(8, M.IIR, False), (2, M.LINEAR_PHASE, True)])
def test_whole_chain_at_the_oversampled_rate(amd, oracle, F, os_type, eq_first):
    """DSPCore::processDouble: processUp, processor-level conv + EQ + OutputFilter at F x 48 kHz on blocks of 4096,
    processDown -- against os_model around the oracle's restatements of the chain at that rate."""
    O = oracle
    S, B, T = 2, 4096, 2
    rate = 48000.0 * F
    order = amd.CPQ_ORDER_EQ_THEN_CONV if eq_first else amd.CPQ_ORDER_CONV_THEN_EQ
    irs = [O.gen_ir(3000, stream=c // 2, channel=c % 2) for c in range(2 * S)]
    nb = B * T // F
    x = np.stack([O.gen_pcm(6 * nb, stream=c // 2, channel=c % 2) for c in range(2 * S)])
    eng = chain_engine(amd, O, S, F, os_type, order, irs, B, T)
    y = np.concatenate([eng.process(x[:, o:o + nb]) for o in range(0, x.shape[1], nb)], axis=1)
    prof = eng.profile_read()
    assert "k_os_halfband" not in prof          # profiling is off: nothing recorded
    po = O.eq_params_bench(0.2)
    q = O.outfilter_design(int(eq_first), 1, 0, 1, rate)
    for s in range(S):
        model = M.Oversampler(F, os_type)
        u = model.up(x[2 * s:2 * s + 2])
        if eq_first:
            el, er, _ = O.eq_process_stereo(u[0], u[1], po, sr=rate, block=B)
            w = [O.convproc_steady(irs[2 * s + ch], v, B) for ch, v in enumerate((el, er))]
        else:
            w = [O.convproc_steady(irs[2 * s + ch], u[ch], B) for ch in range(2)]
            w = list(O.eq_process_stereo(w[0], w[1], po, sr=rate, block=B)[:2])
        fl, fr, _ = O.outfilter_process_stereo(w[0], w[1], q)
        ref = model.down(np.stack([fl, fr]))
        assert rms(y[2 * s] - ref[0]) <= 1e-12 and rms(y[2 * s + 1] - ref[1]) <= 1e-12, (rms(y[2 * s] - ref[0]),)
        assert rms(ref[0]) > 1e-3
    eng.close()


def test_factor_one_is_the_plain_path(amd, oracle):
    O = oracle
    S, B, T = 2, 512, 4
    irs = [O.gen_ir(2000, stream=c // 2, channel=c % 2) for c in range(2 * S)]
    x = np.stack([O.gen_pcm(4 * B * T, stream=c // 2, channel=c % 2) for c in range(2 * S)])
    a = chain_engine(amd, O, S, 1, 0, amd.CPQ_ORDER_CONV_THEN_EQ, irs, B, T)
    b = chain_engine(amd, O, S, 1, 0, amd.CPQ_ORDER_CONV_THEN_EQ, irs, B, T)
    b.set_oversampling(8, M.IIR)
    b.set_oversampling(1, M.IIR)
    b.profile_enable(True)
    ya = np.concatenate([a.process(x[:, o:o + B * T]) for o in range(0, x.shape[1], B * T)], axis=1)
    yb = np.concatenate([b.process(x[:, o:o + B * T]) for o in range(0, x.shape[1], B * T)], axis=1)
    assert np.array_equal(ya, yb)
    assert "k_os_halfband" not in b.profile_read()
    a.close()
    b.close()


def test_abi_errors(amd):
    from convopeq_amd import _capi
    S = 1
    eng = amd.BatchedEngine(S, block_size=480, max_ir_len=1024, max_blocks_per_call=8, call_mode=amd.CPQ_CALLS_ANY,
                            sample_rate=384000.0)
    for factor, t in ((3, 0), (16, 0), (0, 0), (2, 5), (2, -1)):
        with pytest.raises(amd.CpqError) as ei:
            eng.set_oversampling(factor, t)
        assert ei.value.status == _capi.CPQ_ERR_INVALID_ARG
    x = np.zeros((2, 4))
    with pytest.raises(amd.CpqError) as ei:
        eng.os_up(x)                            # factor 1: nothing to run
    assert ei.value.status == _capi.CPQ_ERR_NOT_READY
    eng.set_oversampling(2, M.IIR)
    limit = 480 * 8 // 2
    eng.os_up(np.zeros((2, limit)))
    with pytest.raises(amd.CpqError) as ei:     # n_base * F beyond the call limit
        eng.os_up(np.zeros((2, limit + 1)))
    assert ei.value.status == _capi.CPQ_ERR_INVALID_ARG
    with pytest.raises(amd.CpqError):
        eng.process(np.zeros((2, limit + 1)))
    with pytest.raises(amd.CpqError):
        eng.os_telemetry(1)
    eng.close()
    hi = amd.BatchedEngine(S, block_size=512, max_ir_len=1024, max_blocks_per_call=4, sample_rate=800000.0)
    with pytest.raises(amd.CpqError) as ei:     # processing rate above 768 kHz
        hi.set_oversampling(2, M.IIR)
    assert ei.value.status == _capi.CPQ_ERR_INVALID_ARG
    hi.set_oversampling(1, M.IIR)
    hi.close()
    odd = amd.BatchedEngine(S, block_size=441, max_ir_len=1024, max_blocks_per_call=4, call_mode=amd.CPQ_CALLS_ANY)
    with pytest.raises(amd.CpqError) as ei:     # 441 is not a multiple of 2
        odd.set_oversampling(2, M.IIR)
    assert ei.value.status == _capi.CPQ_ERR_INVALID_ARG
    odd.close()
    wb = amd.BatchedEngine(S, block_size=512, max_ir_len=1024, max_blocks_per_call=4, sample_rate=192000.0)
    wb.set_oversampling(4, M.LINEAR_PHASE)
    with pytest.raises(amd.CpqError):           # 100 * 4 is not whole partitions of 512
        wb.process(np.zeros((2, 100)))
    wb.close()
