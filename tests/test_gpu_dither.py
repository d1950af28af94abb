"""GPU tests of the dither stage (cpq_engine_set_dither, cpq_dither_*; kernel in convopeq_amd/csrc/dither_kernels.hip) and of
16-bit PCM output through the C ABI, against tests/dither_model.py and the reference's recorded codes
(tests/golden/dither_ref.npz).  Every comparison is bit for bit; a NaN (which only the 15-tap shaper without the scrub delivers)
matches a NaN.

Whole chain.  The rows that enter the shaper are taken from an engine with the same chain and CPQ_OUT_DC_BLOCK alone: the DC
kernel's scan is held to its own bar elsewhere (tests/test_gpu_output_stage.py) and is not bit-equal to a sequential model, so the
composition starts behind it: dither_model (headroom, shaper, scrub), out_model (limiter, clamp), the 16-bit encode."""
import ctypes as C
import os

import numpy as np
import pytest

import dither_model as M
import out_model as OM
import pcm_model as PM

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPERS, BITS = (M.FIXED4, M.FIXED15), (8, 16, 24)


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


@pytest.fixture(scope="module")
def tile(K):
    """CPQ_DITHER_TILE as the header states it"""
    import re
    text = open(os.path.join(os.path.dirname(HERE), "include", "convopeq_mi355x.h")).read()
    t = int(re.search(r"#define\s+CPQ_DITHER_TILE\s+(\d+)", text).group(1))
    assert t == K.CPQ_DITHER_TILE
    return t


def same_bits_or_nan(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    a0, b0 = np.ascontiguousarray(np.where(na, 0.0, a)), np.ascontiguousarray(np.where(nb, 0.0, b))
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a0.view(np.uint64), b0.view(np.uint64))


def stage_engine(amd, S, B=64, T=64, rate=48000.0, any_calls=True, flags=0):
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=1024, max_blocks_per_call=T, sample_rate=rate,
                            call_mode=amd.CPQ_CALLS_ANY if any_calls else amd.CPQ_CALLS_WHOLE_BLOCKS)
    if flags:
        eng.set_output_stage(flags)
    return eng


def device_run(torch, eng, x, in_place=False):
    """cpq_dither_process_device on contiguous rows [2 S][n]: with n odd every second row starts on an odd double"""
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = d_in if in_place else torch.full_like(d_in, 7.0)
    eng.dither_process_device(d_in.data_ptr(), d_out.data_ptr(), x.shape[1])
    eng.synchronize()
    return d_out.cpu().numpy()


def signal(S, n, seed):
    rng = np.random.default_rng(seed)
    x = 0.4 * rng.standard_normal((2 * S, n))
    x[:, ::7] *= 4.0                                    # some samples beyond the clamp
    return x


# ------------------------------------------------------------------------------------------------------- the stage alone
@pytest.mark.parametrize("S", (1, 32, 33))
@pytest.mark.parametrize("which", range(5))
def test_stage_alone_every_size(amd, torch, tile, S, which):
    n = (1, tile - 1, tile, tile + 1, 3 * tile + 5)[which]
    x = signal(S, n, 100 * S + which)
    eng = stage_engine(amd, S)
    for rate in (48000.0, 64000.0):
        eng.prepare_to_play(rate, 64 * 64)
        for sh in SHAPERS:
            for bits in BITS:
                headroom = bits == 16                   # with and without CPQ_OUT_HEADROOM (headroom 0.891 and scrub / 1.0)
                eng.set_output_stage(OM.HEADROOM if headroom else 0)
                eng.set_dither(sh, bits)
                y = device_run(torch, eng, x, in_place=(bits == 24))
                ref = M.Dither(rate, S, sh, bits).process(x, M.H if headroom else 1.0, scrubbed=headroom)
                assert same_bits_or_nan(y, ref), (rate, sh, bits)
                assert np.array_equal(y * 2.0 ** (bits - 1), np.rint(y * 2.0 ** (bits - 1)))
    eng.close()


def test_host_entry_and_nan_without_scrub(amd):
    """cpq_dither_process (host pointers); without CPQ_OUT_HEADROOM nothing scrubs: the 15-tap shaper hands a NaN on, the 4-tap
    shaper writes 0 -- and both carry on as the model does"""
    x = signal(2, 150, 5)
    x[0, 10], x[1, 20], x[2, 30], x[3, 149] = np.nan, np.inf, -np.inf, np.nan
    eng = stage_engine(amd, 2)
    for sh in SHAPERS:
        eng.set_dither(sh, 16)
        y = eng.dither_process(x)
        ref = M.Dither(48000.0, 2, sh, 16).process(x, 1.0)
        assert same_bits_or_nan(y, ref)
        assert np.isnan(y[0, 10]) == (sh == M.FIXED15) and np.isfinite(y[1]).all() and np.isfinite(y[2]).all()
    eng.close()


@pytest.mark.parametrize("rate", (44100.0, 48000.0, 64000.0, 1.0e6))
def test_fixture_inputs_give_the_reference_codes(amd, rate):
    """the recorded input, NaN / Inf stretch included, in the recorded two calls, with the reference's headroom; the scrub that
    follows the shaper in the reference's chain turns the 15-tap shaper's NaN outputs into 0"""
    fx = np.load(os.path.join(HERE, "golden", "dither_ref.npz"))
    x, (n1, n2) = fx["input"], fx["calls"]
    eng = stage_engine(amd, 1, rate=rate, flags=OM.HEADROOM)
    for sh in SHAPERS:
        for bits in BITS:
            eng.set_dither(sh, bits)
            y = np.concatenate([eng.dither_process(x[:, :n1]), eng.dither_process(x[:, n1:])], axis=1)
            want = M.scrub(M.recorded(fx, sh, bits, rate))
            assert same_bits_or_nan(y, want), (sh, bits)
    eng.close()


def test_zero_input_is_the_pure_dither_pattern(amd, torch):
    S, n = 40, 200
    eng = stage_engine(amd, S)
    for sh in SHAPERS:
        eng.set_dither(sh, 16)
        y = device_run(torch, eng, np.zeros((2 * S, n)))
        assert y.any() and same_bits_or_nan(y, M.Dither(48000.0, S, sh, 16).process(np.zeros((2 * S, n)), 1.0))
        for s in range(1, S):
            assert np.array_equal(y[2 * s], y[0]) and np.array_equal(y[2 * s + 1], y[1])       # every stream draws the same two sequences
        assert not np.array_equal(y[0], y[1])
    eng.close()


@pytest.mark.parametrize("sh", SHAPERS)
def test_split_invariance(amd, sh):
    S, B = 3, 64
    x = signal(S, 4 * B, 9)
    eng = stage_engine(amd, S, B=B, any_calls=False)           # whole callbacks: one call of 4 == 4 calls
    eng.set_dither(sh, 16)
    one = eng.dither_process(x)
    eng.set_dither(M.OFF)
    eng.set_dither(sh, 16)
    four = np.concatenate([eng.dither_process(np.ascontiguousarray(x[:, o:o + B])) for o in range(0, 4 * B, B)], axis=1)
    eng.close()
    assert same_bits_or_nan(one, four) and same_bits_or_nan(one, M.Dither(48000.0, S, sh, 16).process(x, 1.0))
    eng = stage_engine(amd, S, B=B)                            # CPQ_CALLS_ANY: cuts at 1 and 65
    eng.set_dither(sh, 16)
    parts = [eng.dither_process(np.ascontiguousarray(x[:, a:b])) for a, b in ((0, 1), (1, 65), (65, 4 * B))]
    eng.close()
    assert same_bits_or_nan(np.concatenate(parts, axis=1), one)


def test_state_rules(amd, K):
    S, n = 2, 96
    x = signal(S, 2 * n, 13)
    a, b = np.ascontiguousarray(x[:, :n]), np.ascontiguousarray(x[:, n:])
    for sh in SHAPERS:
        eng = stage_engine(amd, S)
        st = M.Dither(48000.0, S, sh, 16)
        eng.set_dither(sh, 16)
        assert same_bits_or_nan(eng.dither_process(a), st.process(a, 1.0))
        eng.set_dither(sh, 16)                                                     # the same arguments: nothing moves
        for bad in ((3, 16), (-1, 16), (sh, 0), (sh, 33)):                         # refusals move no state
            assert eng._lib.cpq_engine_set_dither(eng._h, bad[0], bad[1]) == K.CPQ_ERR_INVALID_ARG
        assert eng._lib.cpq_dither_process(eng._h, None, None, n) == K.CPQ_ERR_INVALID_ARG
        assert same_bits_or_nan(eng.dither_process(b), st.process(b, 1.0))
        eng.dither_reset()                                                         # errors cleared, the generators run on
        st.reset()
        assert same_bits_or_nan(eng.dither_process(a), st.process(a, 1.0))
        eng.prepare_to_play(64000.0, 64 * 64)                                      # redesigns; reseeds the 15-tap shaper, not the 4-tap one
        st.prepare(64000.0)
        y = eng.dither_process(a)
        assert same_bits_or_nan(y, st.process(a, 1.0))
        fresh = M.Dither(64000.0, S, sh, 16).process(a, 1.0)
        assert same_bits_or_nan(y, fresh) == (sh == M.FIXED15)
        eng.set_dither(sh, 24)                                                     # any change reseeds, for either shaper
        assert same_bits_or_nan(eng.dither_process(a), M.Dither(64000.0, S, sh, 24).process(a, 1.0))
        other = M.FIXED15 if sh == M.FIXED4 else M.FIXED4
        eng.set_dither(other, 24)
        assert same_bits_or_nan(eng.dither_process(a), M.Dither(64000.0, S, other, 24).process(a, 1.0))
        eng.set_dither(M.OFF)
        assert eng._lib.cpq_dither_process(eng._h, a.ctypes.data_as(K.c_double_p), a.ctypes.data_as(K.c_double_p), n) == K.CPQ_ERR_NOT_READY
        assert eng._lib.cpq_dither_reset(eng._h) == K.CPQ_ERR_NOT_READY
        eng.close()


def test_oversampling_sets_the_base_rate(amd):
    """the rate is sample_rate / factor: 128 kHz at 2x designs and seeds for 64 kHz"""
    x = signal(1, 100, 17)
    eng = amd.BatchedEngine(1, block_size=64, max_ir_len=1024, max_blocks_per_call=64, sample_rate=128000.0, call_mode=amd.CPQ_CALLS_ANY)
    eng.set_dither(M.FIXED15, 16)
    eng.set_oversampling(2)
    y = eng.dither_process(x)
    eng.close()
    assert same_bits_or_nan(y, M.Dither(64000.0, 1, M.FIXED15, 16).process(x, 1.0))


# ------------------------------------------------------------------------------------------------------------ 16-bit pack
def test_s16_pack_only_with_dither_at_16_bits_or_fewer(amd, torch, K):
    S, n = 3, 301
    rows = np.random.default_rng(2).uniform(-1.2, 1.2, (2 * S, n))
    rows[0, :4] = [np.nan, 0.5 / 32768.0, 1.5 / 32768.0, -1.0]
    eng = stage_engine(amd, S)
    d_rows = torch.from_numpy(rows).cuda()
    for shaper, bits in ((M.OFF, 0), (M.FIXED4, 24), (M.FIXED15, 17)):
        eng.set_dither(shaper, bits)
        dst = torch.full((2 * S * n,), 0x5A5A, dtype=torch.int16, device="cuda")
        assert eng._lib.cpq_pcm_pack_device(eng._h, C.c_void_p(d_rows.data_ptr()), C.c_void_p(dst.data_ptr()), K.CPQ_PCM_S16, 0, n) == K.CPQ_ERR_UNSUPPORTED
        eng.synchronize()
        assert (dst.cpu().numpy() == 0x5A5A).all()                                 # the destination is untouched
        host = np.full(2 * S * n, 0x5A5A, dtype=np.int16)
        assert eng._lib.cpq_pcm_pack(eng._h, C.c_void_p(rows.ctypes.data), C.c_void_p(host.ctypes.data), K.CPQ_PCM_S16, 0, n) == K.CPQ_ERR_UNSUPPORTED
        assert (host == 0x5A5A).all()
    for bits in (16, 8):
        eng.set_dither(M.FIXED4, bits)
        for layout in (PM.PLANAR, PM.INTERLEAVED):
            got = PM.from_bytes(eng.pcm_pack(rows, K.CPQ_PCM_S16, layout), PM.S16, layout, 2 * S, n)
            assert np.array_equal(got, M.encode16(rows))
    assert list(M.encode16(rows[0, :4])) == [0, 0, 2, -32768]
    eng.close()


# ------------------------------------------------------------------------------------------------------------ whole chain
def _copy_params(po, pa):
    for i in range(20):
        b, o = pa.bands[i], po.bands[i]
        b.frequency, b.gain, b.q, b.enabled, b.type, b.channel_mode = o.frequency, o.gain, o.q, o.enabled, o.type, o.channelMode
    pa.nonlinear_saturation = po.nonlinearSaturation
    return pa


def chain_engine(amd, O, c):
    rate = 48000.0 * c["F"]
    eng = amd.BatchedEngine(c["S"], block_size=c["B"], max_ir_len=len(c["irs"][0]), max_blocks_per_call=c["T"], sample_rate=rate)
    eng.prepare_to_play(rate, c["B"] * c["T"])
    for s in range(c["S"]):
        eng.set_impulse(s, c["irs"][2 * s], c["irs"][2 * s + 1])
    eng.set_eq_params(amd.CPQ_ALL_STREAMS, _copy_params(O.eq_params_bench(0.2), amd.eq_params_default()))
    eng.set_oversampling(c["F"])
    return eng


def calls(c):
    return range(0, c["x"].shape[1], c["nb"])


@pytest.fixture(scope="module")
def chain(amd, oracle):
    """short IR + EQ + 2x oversampling, three streams, F32 input: the rows of an engine that never heard of the stage, and the
    rows behind the DC blocker alone"""
    O = oracle
    S, F, B, T = 3, 2, 512, 8
    nb = B * T // F
    irs = [O.gen_ir(2000, stream=c // 2, channel=c % 2) for c in range(2 * S)]
    x = (0.25 * np.stack([O.gen_pcm(2 * nb, stream=c // 2, channel=c % 2) for c in range(2 * S)])).astype(np.float32)
    c = dict(S=S, F=F, B=B, T=T, nb=nb, irs=irs, x=x)
    x64 = x.astype(np.float64)
    for key, flags in (("plain", 0), ("dc", OM.DC_BLOCK)):
        eng = chain_engine(amd, O, c)
        eng.set_output_stage(flags)
        c[key] = np.concatenate([eng.process(np.ascontiguousarray(x64[:, o:o + nb])) for o in calls(c)], axis=1)
        eng.close()
    return c


def run_pcm_chain(amd, oracle, K, c, shaper, bits, out_fmt, layout, metering=0, gain=1.0):
    eng = chain_engine(amd, oracle, c)
    eng.set_output_stage(OM.ALL)
    if gain != 1.0:
        eng.set_gains(amd.CPQ_ALL_STREAMS, 1.0, gain)
    eng.set_dither(shaper, bits)
    if metering:
        eng.set_metering(metering)
    out = []
    for o in calls(c):
        src = PM.to_bytes(c["x"][:, o:o + c["nb"]], PM.F32, layout)
        raw = eng.process_pcm(src, K.CPQ_PCM_F32, out_fmt, c["nb"], layout)
        out.append(PM.from_bytes(raw, out_fmt, layout, 2 * c["S"], c["nb"]))
    rec = eng.meter_read_blocks()[0] if metering else None
    env = [eng.out_read_envelope(s) for s in range(c["S"])]
    eng.close()
    return np.concatenate(out, axis=1), rec, env


@pytest.mark.parametrize("sh", SHAPERS)
@pytest.mark.parametrize("layout", (PM.PLANAR, PM.INTERLEAVED))
def test_whole_chain_f32_in_s16_out(amd, oracle, K, chain, sh, layout):
    c = chain
    got, rec, env = run_pcm_chain(amd, oracle, K, c, sh, 16, K.CPQ_PCM_S16, layout, metering=3)
    post = M.Dither(48000.0, c["S"], sh, 16).process(c["dc"], M.H, scrubbed=True)        # the shaper's state runs across the calls
    lim = OM.OutStage(48000.0, c["S"])
    rows = lim.process(post, c["B"] // c["F"], OM.LIMITER | OM.CLAMP)
    assert np.array_equal(got, M.encode16(rows)) and np.abs(got).max() > 30
    # a quiet input: the limiter stays idle, so every code is the fp64 row exactly
    assert env == [1.0] * c["S"] == lim.env and np.array_equal(rows, post)
    assert np.array_equal(got.astype(np.float64) * 2.0 ** -15, rows)
    # the meters read the post-dither rows
    eng = stage_engine(amd, c["S"], B=c["B"], T=c["T"], rate=48000.0 * c["F"], any_calls=False)
    eng.set_oversampling(c["F"])
    eng.set_metering(3)
    for o in calls(c):
        eng.meter_process(np.ascontiguousarray(post[:, o:o + c["nb"]]))
    ref, _ = eng.meter_read_blocks()
    eng.close()
    assert rec.shape == ref.shape and rec.tobytes() == ref.tobytes() and rec["mean_square"].max() > 0.0


def test_whole_chain_limited_samples_leave_the_grid(amd, oracle, K, chain):
    """the limiter acts after quantisation: loud enough to limit, the F64 rows are the model's and no longer multiples of 2^-15"""
    c = chain
    gain = 200.0
    got, _, env = run_pcm_chain(amd, oracle, K, c, M.FIXED15, 16, K.CPQ_PCM_F64, PM.PLANAR, gain=gain)
    eng = chain_engine(amd, oracle, c)                                                   # the rows behind makeup gain and DC blocker
    eng.set_gains(amd.CPQ_ALL_STREAMS, 1.0, gain)
    eng.set_output_stage(OM.DC_BLOCK)
    x64 = c["x"].astype(np.float64)
    dc = np.concatenate([eng.process(np.ascontiguousarray(x64[:, o:o + c["nb"]])) for o in calls(c)], axis=1)
    eng.close()
    post = M.Dither(48000.0, c["S"], M.FIXED15, 16).process(dc, M.H, scrubbed=True)
    lim = OM.OutStage(48000.0, c["S"])
    rows = lim.process(post, c["B"] // c["F"], OM.LIMITER | OM.CLAMP)
    assert same_bits_or_nan(got, rows) and env == lim.env and min(env) < 1.0
    assert not np.array_equal(rows * 32768.0, np.rint(rows * 32768.0)) and np.abs(rows).max() <= OM.H


def test_s16_output_still_refused_without_16_bit_dither(amd, oracle, K, chain):
    c = chain
    for shaper, bits in ((M.OFF, 0), (M.FIXED15, 24)):
        eng = chain_engine(amd, oracle, c)
        eng.set_output_stage(OM.ALL)
        eng.set_dither(shaper, bits)
        src = PM.to_bytes(c["x"][:, :c["nb"]], PM.F32, PM.PLANAR)
        dst = np.full(2 * c["S"] * c["nb"], 0x5A5A, dtype=np.int16)
        rc = eng._lib.cpq_engine_process_block_pcm(eng._h, C.c_void_p(src.ctypes.data), K.CPQ_PCM_F32, C.c_void_p(dst.ctypes.data),
                                                   K.CPQ_PCM_S16, PM.PLANAR, 0, c["nb"])
        assert rc == K.CPQ_ERR_UNSUPPORTED and (dst == 0x5A5A).all()
        y = eng.process(np.ascontiguousarray(c["x"][:, :c["nb"]].astype(np.float64)))    # and no state moved: the first call's rows
        eng.close()
        if shaper == M.OFF:
            ref = chain_engine(amd, oracle, c)
            ref.set_output_stage(OM.ALL)
            want = ref.process(np.ascontiguousarray(c["x"][:, :c["nb"]].astype(np.float64)))
            ref.close()
            assert same_bits_or_nan(y, want)


def test_dither_off_is_an_engine_that_never_heard_of_it(amd, oracle, chain):
    c = chain
    x64 = c["x"].astype(np.float64)
    eng = chain_engine(amd, oracle, c)
    eng.set_dither(M.FIXED15, 16)                                                        # on, then off again, before the first call
    eng.set_dither(M.OFF)
    eng.profile_enable()
    y = np.concatenate([eng.process(np.ascontiguousarray(x64[:, o:o + c["nb"]])) for o in calls(c)], axis=1)
    assert "k_dither" not in eng.profile_read()                                          # nothing is launched
    eng.close()
    assert same_bits_or_nan(y, c["plain"]) and np.abs(y).max() > 1e-3
