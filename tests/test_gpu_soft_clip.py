"""GPU tests of the soft clipper (cpq_engine_set_soft_clip, cpq_soft_clip_*; kernel in convopeq_amd/csrc/softclip_kernels.hip).

The kernel alone is held to tests/softclip_model.py bit for bit (a NaN matching a NaN: x86 and the GPU give the default NaN
opposite signs), and so is the stage inside the oversampled chain: there it sits between pieces that are bit-exact entry points
of their own (cpq_os_up, cpq_eq_process, a multiply, cpq_os_down), so a second engine with the clipper off runs those pieces
around the model and the two outputs must be the same bits.  At factor 1 the local 2x pair is compared with os_model's one
31-tap stage around the model under the oversampler tests' own bar, 1e-13 absolute on signals of order 1.

Every engine runs the same chain: convolver bypassed, the EQ's default (flat) parameters."""
import ctypes as C

import numpy as np
import pytest

import os_model as OS
import out_model as OM
import dither_model as DM
import pcm_model as PM
import softclip_model as M

pytestmark = pytest.mark.gpu

OS_BAR = 1.0e-13            # tests/test_gpu_oversampling.py: |kernel - os_model| on signals of order 1
AMOUNTS = (0.2, 1.0)        # stream 0, stream 1


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def K():
    from convopeq_amd import _capi
    return _capi


def engine(amd, S=2, B=64, T=64, F=1, any_calls=True, clip=AMOUNTS, makeup=1.0, rate=48000.0):
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=1024, max_blocks_per_call=T, sample_rate=rate * F,
                            call_mode=amd.CPQ_CALLS_ANY if any_calls else amd.CPQ_CALLS_WHOLE_BLOCKS)
    eng.set_conv_bypass(True)
    eng.set_eq_params(amd.CPQ_ALL_STREAMS, amd.eq_params_default())
    if F > 1:
        eng.set_oversampling(F)
    if makeup != 1.0:
        eng.set_gains(amd.CPQ_ALL_STREAMS, 1.0, makeup)
    if clip is not None:
        for s in range(S):
            eng.set_soft_clip(s, True, clip[s % len(clip)])
    return eng


def planted(amount):
    """both signs of the three corners and their neighbours one ulp either side, the doubles around a tanh argument of 4.5 and
    values far beyond it, zeros, denormals, infinities, and a NaN"""
    thr, knee, _ = M.params(amount)
    pos = []
    for v in (thr - knee, thr, thr + knee):
        pos += [np.nextafter(v, 0.0), v, np.nextafter(v, 4.0)]
    edge = thr + 4.5 * knee
    pos += [np.nextafter(edge, 0.0), edge, np.nextafter(edge, 4.0), thr + 5.0 * knee, 100.0, 1.0e300, 0.0, 5.0e-324, 1.0e-310, np.inf]
    return np.array([s * v for v in pos for s in (1.0, -1.0)] + [np.nan])


def rows_with_planted(S, n, cb, seed, amounts=AMOUNTS):
    """noise at +-2; where the row is long enough the planted values sit from sample 0 (body samples of the first callback, over
    16-byte seams at every offset), then again ending at the row's last sample (the tail of the last callback) and at the end of
    the first callback"""
    x = np.random.default_rng(seed).uniform(-2.0, 2.0, (2 * S, n))
    for c in range(2 * S):
        p = planted(amounts[(c // 2) % len(amounts)])
        p = np.roll(p, c)                               # another value on every seam in every row
        m = min(n, p.size)
        x[c, :m] = p[:m]
        x[c, n - m:] = p[p.size - m:]
        if cb < n and cb >= m:
            x[c, cb - m:cb] = p[p.size - m:]
    return x


def device_clip(torch, eng, x, cb, in_place=False):
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = d_in if in_place else torch.full_like(d_in, 7.0)
    eng.soft_clip_process_device(d_in.data_ptr(), d_out.data_ptr(), x.shape[1], cb)
    eng.synchronize()
    return d_out.cpu().numpy()


# -------------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("cb", (1, 2, 3, 5, 64, 441, 2049))
def test_kernel_alone_against_the_model(amd, torch, cb):
    eng = engine(amd, T=64)
    for n in sorted({cb, 2 * cb + 3, 2049, 4096}):      # odd n: every second row starts on an odd double; 2 cb + 3: a ragged last callback
        if n > 64 * 64:
            continue
        x = rows_with_planted(2, n, cb, 1000 + cb + n)
        want = M.clip_rows(x, cb, AMOUNTS)
        y = device_clip(torch, eng, x, cb, in_place=(n % 2 == 0))
        assert M.same(y, want), (cb, n, int(np.sum(~(np.isnan(y) & np.isnan(want)) & (y != want))))
        if n == 2049:
            assert M.same(eng.soft_clip_process(x, cb), want)                            # the host-pointer entry
            assert np.isnan(y[0][np.isnan(x[0])]).all() and np.isnan(y[0][np.isinf(x[0])]).all()   # NaN passes, Inf becomes NaN, as the model says
            assert np.isnan(want).sum() == np.isnan(x).sum() + np.isinf(x).sum()
    # the two streams really clip differently, and a stream that rests is left alone bit for bit
    x = rows_with_planted(2, 333, cb, 7)
    eng.set_soft_clip(1, False, 1.0)
    y = device_clip(torch, eng, x, cb)
    assert M.same(y[:2], M.clip_rows(x, cb, AMOUNTS)[:2])
    assert np.array_equal(y[2:].view(np.uint64), x[2:].view(np.uint64))
    assert not M.same(M.clip(x[2], cb, AMOUNTS[0]), M.clip(x[2], cb, AMOUNTS[1]))
    eng.close()


def test_planted_values_take_both_paths_in_the_kernel(amd, torch):
    """the same planted values as body samples (callback 64: the first 64) and as tail samples (callback 3: every one), over a
    16-byte seam (neighbours 2k, 2k + 1 share an access; 2k + 1, 2k + 2 do not) and in rows that start on an odd double (n odd)"""
    eng = engine(amd)
    n = 63
    x = rows_with_planted(2, n, 64, 3)
    body, tail = device_clip(torch, eng, x, 64), device_clip(torch, eng, x, 3)
    for c in range(4):
        a = AMOUNTS[c // 2]
        mask = M.tail_mask(n, 64)
        assert mask.tolist() == [False] * 60 + [True] * 3
        assert M.same(body[c], np.where(mask, M.tail(x[c], a), M.body(x[c], a))) and M.same(tail[c], M.tail(x[c], a))
        ok = ~np.isnan(body[c]) & ~np.isnan(tail[c])
        assert np.any(body[c][ok] != tail[c][ok])                    # the two paths differ in bits on these inputs
    eng.close()


# ------------------------------------------------------------------------------------------------- inside the oversampled chain
@pytest.mark.parametrize("F", (2, 8))
def test_oversampled_chain_bit_for_bit(amd, F):
    """make-up gain 1.7, clipper on: three calls, the last one ragged.  The reference engine has the clipper off and no make-up
    gain and runs the chain's own pieces by their entry points: up, EQ, x 1.7 (one rounding, as the kernel's multiply), the model,
    down."""
    S, B = 2, 64 * F
    calls = (128, 64, 100)                               # base-rate samples; 100 = one callback of 64 and a ragged one of 36
    rng = np.random.default_rng(40 + F)
    x = rng.uniform(-1.0, 1.0, (2 * S, sum(calls)))
    on = engine(amd, S, B=B, T=4, F=F, makeup=1.7)
    ref = engine(amd, S, B=B, T=4, F=F, clip=None)
    on.profile_enable(True)
    o, worst, clipped = 0, 0.0, 0
    for n in calls:
        xb = np.ascontiguousarray(x[:, o:o + n])
        y = on.process(xb)
        block = 1.7 * ref.eq_process(ref.os_up(xb))
        after = M.clip_rows(block, B, AMOUNTS)
        clipped += int(np.sum(after != block))
        want = ref.os_down(after)
        worst = max(worst, float(np.abs(y - want).max()))
        print(f"factor {F}, call of {n}: max |engine - pieces| = {np.abs(y - want).max():.3e}")
        assert np.array_equal(y.view(np.uint64), want.view(np.uint64)), (F, n, worst)
        o += n
    assert clipped > 0.2 * 2 * S * sum(calls) * F        # the block really is clipped: noise at +-1.7 against clip starts of 0.74 and 0.1
    prof = on.profile_read()
    assert prof["k_soft_clip"][0] == len(calls) and "k_soft_clip" not in ref.profile_read()
    for s in range(S):
        assert on.soft_clip_telemetry(s)["corruption_events"] == 0          # the local stage never ran
    on.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------- factor 1
def local_model():
    m = OS.Oversampler(2, OS.IIR)
    m.stages = [OS.design_stage(2, OS.IIR)]             # prepareSingleStage(31, 90.0): the design of the third IIR-like stage
    assert m.stages[0]["taps"] == 31 and len(m.stages[0]["conv"]) == 16
    m.reset()
    return m


def test_factor_one_local_pair_against_the_models(amd):
    S, B = 2, 64
    calls = (1, 7, 512, 441)
    x = np.random.default_rng(9).uniform(-1.0, 1.0, (2 * S, sum(calls)))
    on = engine(amd, S, B=B, T=8, makeup=1.7)
    ref = engine(amd, S, B=B, T=8, makeup=1.7, clip=None)
    on.profile_enable(True)
    models = [local_model() for _ in range(S)]
    o, clipped = 0, 0
    for n in calls:
        xb = np.ascontiguousarray(x[:, o:o + n])
        y, chain = on.process(xb), ref.process(xb)      # chain: what enters the clipper's local pair
        for s in range(S):
            u = models[s].up(chain[2 * s:2 * s + 2])
            v = M.clip_rows(u, 2 * B, [AMOUNTS[s]])
            clipped += int(np.sum(u != v))
            want = models[s].down(v)
            err = float(np.abs(y[2 * s:2 * s + 2] - want).max())
            print(f"call of {n}, stream {s}: max |engine - models| = {err:.3e}")
            assert err <= OS_BAR, (n, s, err)
        o += n
    assert clipped > 500
    prof = on.profile_read()
    assert prof["k_soft_clip"][0] == len(calls) and prof["k_os_halfband"][0] == 2 * len(calls)
    for s in range(S):
        t = on.soft_clip_telemetry(s)
        assert t["corruption_events"] == 0 and t["auto_clears"] == 0 and models[s].events == 0
    on.close()
    ref.close()


def test_factor_one_gain_and_latency_on_a_quiet_sine(amd):
    """below the clip start the clipper is the identity, so what is left is the local pair: 3/4 of the signal, 15 samples late"""
    S, B, n = 2, 64, 2048
    t = np.arange(n, dtype=np.float64)
    x = np.stack([0.05 * np.sin(2 * np.pi * f * t + c) for c, f in enumerate((0.011, 0.023, 0.037, 0.051))])
    assert np.abs(x).max() < M.params(1.0)[0] - M.params(1.0)[1]
    on, ref = engine(amd, S, B=B, T=32), engine(amd, S, B=B, T=32, clip=None)
    y, plain = on.process(x), ref.process(x)
    L = int(amd.soft_clip_latency(1))
    assert L == 15 and amd.soft_clip_latency(2) == 0.0
    for c in range(2 * S):
        want = 0.75 * plain[c, 64:n - L]
        got = y[c, 64 + L:]
        rel = float(np.sqrt(np.mean((got - want) ** 2)) / np.sqrt(np.mean(want ** 2)))
        off = [float(np.sqrt(np.mean((y[c, 64 + d:n - 30 + d] - 0.75 * plain[c, 64:n - 30]) ** 2))) for d in range(30)]
        print(f"channel {c}: rms(engine - 0.75 x delayed by 15) / rms = {rel:.3e}; best delay {int(np.argmin(off))}")
        assert rel <= 1.0e-4 and int(np.argmin(off)) == L
    on.close()
    ref.close()


def test_factor_one_state_rules(amd):
    """cpq_soft_clip_reset, cpq_engine_prepare, cpq_engine_set_oversampling and a change of `enabled` clear the local stage; a
    change of the amount alone does not"""
    S, B, n = 2, 64, 256
    x = np.random.default_rng(21).uniform(-1.0, 1.0, (2 * S, n))
    fresh = engine(amd, S, B=B, T=8)
    first = fresh.process(x)
    second = fresh.process(x)
    assert not np.array_equal(first, second)             # the histories carry
    fresh.close()
    warm = engine(amd, S, B=B, T=8, clip=None)           # the chain has run once, the local stage never: what a cleared stage must give
    warm.process(x)
    for s in range(S):
        warm.set_soft_clip(s, True, AMOUNTS[s])
    cleared = warm.process(x)
    warm.close()
    actions = {"reset": lambda e: e.soft_clip_reset(),
               "prepare": lambda e: e.prepare_to_play(48000.0, B * 8),
               "oversampling": lambda e: (e.set_oversampling(2), e.set_oversampling(1)),
               "enabled": lambda e: (e.set_soft_clip(1, False, AMOUNTS[1]), e.set_soft_clip(1, True, AMOUNTS[1]))}
    for name, act in actions.items():
        eng = engine(amd, S, B=B, T=8)
        eng.process(x)
        act(eng)
        again = eng.process(x)
        assert np.array_equal(again, first if name == "prepare" else cleared), name      # prepare starts the chain over as well
        assert not np.array_equal(again, second)
        eng.close()
    eng = engine(amd, S, B=B, T=8)
    eng.process(x)
    eng.set_soft_clip(0, True, 0.9)                      # the amount alone: the histories stay
    eng.set_soft_clip(0, True, AMOUNTS[0])
    assert np.array_equal(eng.process(x), second)
    eng.close()


def test_a_resting_stream_at_factor_one_is_not_touched(amd):
    S, B, n = 3, 64, 300
    x = np.random.default_rng(22).uniform(-1.0, 1.0, (2 * S, n))
    plain = engine(amd, S, B=B, T=8, clip=None)
    every = engine(amd, S, B=B, T=8, clip=(0.5,))
    some = engine(amd, S, B=B, T=8, clip=None)
    some.set_soft_clip(0, True, 0.5)
    some.set_soft_clip(2, True, 0.5)                     # two runs of one stream each around a resting one
    for _ in range(2):
        p, a, b = plain.process(x), every.process(x), some.process(x)
        assert np.array_equal(b[2:4], p[2:4]) and np.array_equal(b[0:2], a[0:2]) and np.array_equal(b[4:6], a[4:6])
        assert not np.array_equal(a[2:4], p[2:4])
    for e in (plain, every, some):
        e.close()


# -------------------------------------------------------------------------------------------------------------- off is off
@pytest.mark.parametrize("F", (1, 2))
def test_off_is_an_engine_that_never_heard_of_it(amd, F):
    S, B = 2, 64 * F
    x = np.random.default_rng(30 + F).uniform(-1.5, 1.5, (2 * S, 8 * 64))      # 8 calls: past the 255 samples the 2x pair delays by
    never = engine(amd, S, B=B, T=4, F=F, clip=None, makeup=1.7)
    told_off = engine(amd, S, B=B, T=4, F=F, clip=None, makeup=1.7)
    told_off.set_soft_clip(amd.CPQ_ALL_STREAMS, False, 0.5)
    toggled = engine(amd, S, B=B, T=4, F=F, clip=None, makeup=1.7)
    toggled.set_soft_clip(amd.CPQ_ALL_STREAMS, True, 0.5)
    toggled.set_soft_clip(amd.CPQ_ALL_STREAMS, False, 0.5)
    outs = []
    for e in (never, told_off, toggled):
        e.profile_enable(True)
        outs.append(np.concatenate([e.process(np.ascontiguousarray(x[:, o:o + 64])) for o in range(0, x.shape[1], 64)], axis=1))
        prof = e.profile_read()
        assert "k_soft_clip" not in prof and (F > 1) == ("k_os_halfband" in prof)
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
    assert np.array_equal(outs[0].view(np.uint64), outs[2].view(np.uint64))
    on = engine(amd, S, B=B, T=4, F=F, makeup=1.7)
    clipped = np.concatenate([on.process(np.ascontiguousarray(x[:, o:o + 64])) for o in range(0, x.shape[1], 64)], axis=1)
    assert not np.array_equal(clipped, outs[0]) and np.abs(outs[0]).max() > 1.0
    for e in (never, told_off, toggled, on):
        e.close()


# ------------------------------------------------------------------------------------------------------------------- guards
def test_non_finite_input_raises_the_local_stages_own_counters(amd):
    """The EQ ahead of the stage turns a non-finite sample into 0 (sanitizeFiniteInRangeV), so the infinity is made behind it: one
    sample of stream 1 at 1.5 under a make-up gain of 1.7e308 overflows to +Inf on its way into the local pair (and the stream's
    other samples, finite, lie above the stage's 2^53 guard)."""
    S, B, n = 2, 64, 128
    x = np.random.default_rng(31).uniform(-0.5, 0.5, (2 * S, n))
    eng = engine(amd, S, B=B, T=8)
    clean = engine(amd, S, B=B, T=8)
    eng.process(x)
    clean.process(x)
    eng.set_gains(1, 1.0, 1.7e308)
    bad = x.copy()
    bad[2, 40] = 1.5                                     # 1.5 * 1.7e308 overflows
    y = eng.process(bad)
    yc = clean.process(x)
    t0, t1 = eng.soft_clip_telemetry(0), eng.soft_clip_telemetry(1)
    assert t1["corruption_events"] > 0 and t1["auto_clears"] >= 1 and t0["corruption_events"] == 0 and t0["auto_clears"] == 0
    assert np.array_equal(y[:2], yc[:2])                 # the other stream does not notice
    assert np.all(y[2:4] == 0.0)                         # the call's processDown auto-clears and delivers silence
    for s in range(S):                                   # the main oversampler's counters are another instance's
        t = eng.os_telemetry(s)
        assert t["corruption_events"] == 0 and t["auto_clears"] == 0 and t["hard_fallback"] == 0
    eng.close()
    clean.close()


# ------------------------------------------------------------------------------------------------------------- composition
def test_composes_with_output_stage_and_dithered_pcm(amd, K):
    """one whole-chain call, F64 rows in, 16-bit PCM out: clipper, DC blocker, 4-tap shaper at 16 bits (headroom, scrub), limiter,
    clamp, pack -- equal to running the pieces one after the other by their own entry points"""
    S, B, n = 2, 512, 512
    x = np.random.default_rng(33).uniform(-1.0, 1.0, (2 * S, n))

    def whole(clip):
        e = engine(amd, S, B=B, T=2, any_calls=False, clip=clip, makeup=1.7)
        e.set_output_stage(OM.ALL)
        e.set_dither(DM.FIXED4, 16)
        raw = e.process_pcm(PM.to_bytes(x, PM.F64, PM.PLANAR), K.CPQ_PCM_F64, K.CPQ_PCM_S16, n, PM.PLANAR)
        e.close()
        return PM.from_bytes(raw, PM.S16, PM.PLANAR, 2 * S, n)

    got = whole(AMOUNTS)
    first = engine(amd, S, B=B, T=2, any_calls=False, makeup=1.7)
    rows = first.process(x)                              # routing, make-up gain, the clipper's local pair
    first.close()
    dc = engine(amd, S, B=B, T=2, any_calls=False, clip=None)
    dc.set_output_stage(OM.DC_BLOCK)
    rows = dc.out_process(rows)
    dc.close()
    sh = engine(amd, S, B=B, T=2, any_calls=False, clip=None)
    sh.set_output_stage(OM.HEADROOM)
    sh.set_dither(DM.FIXED4, 16)
    rows = sh.dither_process(rows)
    post = engine(amd, S, B=B, T=2, any_calls=False, clip=None)
    post.set_output_stage(OM.LIMITER | OM.CLAMP)
    rows = post.out_process(rows)
    post.close()
    want = PM.from_bytes(sh.pcm_pack(rows, K.CPQ_PCM_S16, PM.PLANAR), PM.S16, PM.PLANAR, 2 * S, n)
    sh.close()
    assert np.array_equal(got, want) and np.abs(got).max() > 10000
    assert not np.array_equal(got, whole(None))          # the clipper is in the call


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_state_moves(amd, torch, K):
    S, B, n = 2, 64, 96
    x = np.random.default_rng(34).uniform(-2.0, 2.0, (2 * S, n))
    eng = engine(amd, S, B=B, T=8, clip=None)
    lib = K.load()
    h = eng._h
    buf = np.zeros((2 * S, n))
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    # off: the row calls and the reset are refused, telemetry reads zeros
    assert lib.cpq_soft_clip_process(h, p, p, n, B) == K.CPQ_ERR_NOT_READY and lib.cpq_soft_clip_reset(h) == K.CPQ_ERR_NOT_READY
    assert lib.cpq_soft_clip_process_device(h, buf.ctypes.data, buf.ctypes.data, n, B) == K.CPQ_ERR_NOT_READY
    assert eng.soft_clip_telemetry(0)["corruption_events"] == 0
    eng.process(x)
    for stream, amount in ((S, 0.5), (-2, 0.5), (0, -0.01), (0, 1.01), (0, float("nan")), (0, float("inf")), (amd.CPQ_ALL_STREAMS, 2.0)):
        assert lib.cpq_engine_set_soft_clip(h, stream, 1, amount) == K.CPQ_ERR_INVALID_ARG, (stream, amount)
    assert lib.cpq_soft_clip_reset(h) == K.CPQ_ERR_NOT_READY              # still off: no refused call switched it on
    ref = engine(amd, S, B=B, T=8, clip=None)
    ref.process(x)
    assert np.array_equal(eng.process(x), ref.process(x))
    eng.set_soft_clip(amd.CPQ_ALL_STREAMS, True, 0.5)
    assert lib.cpq_engine_set_soft_clip(h, 0, 1, 1.5) == K.CPQ_ERR_INVALID_ARG and lib.cpq_engine_set_soft_clip(h, 5, 0, 0.5) == K.CPQ_ERR_INVALID_ARG
    want = M.clip_rows(x, B, (0.5, 0.5))
    assert M.same(eng.soft_clip_process(x, B), want)     # the refused amount and stream changed nothing
    buf[:] = x
    for args in ((None, p, n, B), (p, None, n, B), (p, p, 0, B), (p, p, -1, B), (p, p, 8 * B + 1, B), (p, p, n, 0), (p, p, n, -3)):
        assert lib.cpq_soft_clip_process(h, *args) == K.CPQ_ERR_INVALID_ARG, args[2:]
    odd = C.cast(buf.ctypes.data + 8, C.POINTER(C.c_double))
    assert lib.cpq_soft_clip_process(h, odd, odd, 8, B) == K.CPQ_ERR_INVALID_ARG
    assert np.array_equal(buf, x)
    tel = K.OsTelemetry()
    assert lib.cpq_soft_clip_read_telemetry(h, S, C.byref(tel)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_soft_clip_read_telemetry(h, 0, None) == K.CPQ_ERR_INVALID_ARG
    eng.close()
    ref.close()
