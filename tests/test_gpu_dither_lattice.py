"""GPU tests of the adaptive 9th-order lattice shaper of the dither stage (CPQ_DITHER_ADAPTIVE9, cpq_dither_set_adaptive_coeffs /
cpq_dither_get_adaptive_coeffs; kernel k_dither_lattice in convopeq_amd/csrc/dither_kernels.hip) through the C ABI, against
tests/lattice_model.py and the reference's recorded codes (tests/golden/lattice_ref.npz).  Every comparison is bit for bit; a NaN
(which the shaper hands on for the sample that carried it, unless the scrub follows) matches a NaN.

Whole chain: composed as in tests/test_gpu_dither.py -- the rows that enter the shaper are taken behind the DC blocker from a twin
engine, then lattice_model (headroom, shaper, scrub), out_model (limiter, clamp), the 16-bit encode."""
import os

import numpy as np
import pytest

import dither_model as M
import lattice_model as L
import out_model as OM
import pcm_model as PM

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
A9 = L.ADAPTIVE9
BITS = (8, 16, 24)
STRONG = [0.82, -0.68, 0.55, -0.43, 0.33, -0.25, 0.18, -0.12, 0.07]


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


def same_bits_or_nan(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    a0, b0 = np.ascontiguousarray(np.where(na, 0.0, a)), np.ascontiguousarray(np.where(nb, 0.0, b))
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a0.view(np.uint64), b0.view(np.uint64))


def stage_engine(amd, S, B=64, T=64, rate=48000.0, flags=0):
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=1024, max_blocks_per_call=T, sample_rate=rate, call_mode=amd.CPQ_CALLS_ANY)
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


def stream_sets(S, seed):
    """a set of its own for every stream: stream 0 the strong set, then random ones of every length 0 .. 9, some beyond +-0.85"""
    rng = np.random.default_rng(seed)
    return [STRONG if s == 0 else list(rng.uniform(-1.0, 1.0, (s * 7) % 10)) for s in range(S)]


def load(eng, model, sets):
    for s, k in enumerate(sets):
        eng.dither_set_adaptive_coeffs(s, k)
        model.set_coeffs(s, k)


# ------------------------------------------------------------------------------------------------------- the stage alone
@pytest.mark.parametrize("S", (1, 32, 33))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 197))
def test_stage_alone_every_size(amd, torch, K, S, n):
    """one channel pair, one full wave, a second workgroup with two live rows; n around the 64-sample tile, odd n included"""
    assert K.CPQ_DITHER_TILE == 64
    x = signal(S, n, 100 * S + n)
    sets = stream_sets(S, S)
    eng = stage_engine(amd, S)
    for bits in BITS:
        headroom = bits == 16                           # with and without CPQ_OUT_HEADROOM (headroom 0.891 and scrub / 1.0)
        eng.set_output_stage(OM.HEADROOM if headroom else 0)
        eng.set_dither(A9, bits)
        ref = L.Lattice(S, bits)
        load(eng, ref, sets)
        y = device_run(torch, eng, x, in_place=(bits == 24))
        want = ref.process(x, L.H if headroom else 1.0, scrubbed=headroom)
        assert same_bits_or_nan(y, want), bits
        assert np.array_equal(y * 2.0 ** (bits - 1), np.rint(y * 2.0 ** (bits - 1)))
        if S > 1 and n > 1:
            assert not np.array_equal(y[0], y[2])
    eng.close()


def test_host_entry_and_non_finite_input(amd):
    """cpq_dither_process (host pointers) without the scrub: a NaN in is a NaN out for that sample only, +-inf goes to the rails"""
    x = signal(2, 150, 5)
    x[0, 10], x[1, 20], x[2, 30], x[3, 149] = np.nan, np.inf, -np.inf, np.nan
    eng = stage_engine(amd, 2)
    eng.set_dither(A9, 16)
    ref = L.Lattice(2, 16)
    load(eng, ref, [STRONG, [0.3, -0.2]])
    y = eng.dither_process(x)
    eng.close()
    assert same_bits_or_nan(y, ref.process(x, 1.0))
    assert np.array_equal(np.isnan(y), np.isnan(x)) and y[1, 20] == 1.0 - 2.0 ** -15 and y[2, 30] == -1.0


@pytest.mark.parametrize("case", "abcde")
def test_fixture_inputs_give_the_reference_codes(amd, case):
    """the recorded input, NaN / Inf stretch included, in the recorded two calls, with the reference's headroom; the scrub that
    follows the shaper in the reference's chain turns its NaN outputs into 0.  Case e swaps the set between the two calls"""
    fx = np.load(os.path.join(HERE, "golden", "lattice_ref.npz"))
    x, (n1, n2) = fx["input"], fx["calls"]
    eng = stage_engine(amd, 1, flags=OM.HEADROOM)
    for bits in BITS:
        eng.set_dither(M.OFF)
        eng.set_dither(A9, bits)
        eng.dither_set_adaptive_coeffs(amd.CPQ_ALL_STREAMS, fx["set1_" + case])
        first = eng.dither_process(x[:, :n1])
        if bool(fx["swap_" + case]):
            eng.dither_set_adaptive_coeffs(0, fx["set2_" + case])
        y = np.concatenate([first, eng.dither_process(x[:, n1:])], axis=1)
        assert same_bits_or_nan(y, M.scrub(L.recorded(fx, case, bits))), bits
    eng.close()


# ------------------------------------------------------------------------------------------------------------ state rules
def test_state_rules(amd, K):
    S, n = 3, 96
    x = signal(S, 8 * n, 13)
    part = [np.ascontiguousarray(x[:, i * n:(i + 1) * n]) for i in range(8)]
    sets = [STRONG, [0.5, -0.4, 0.3], [1.5, -3.0, np.nan, np.inf, 0.25, -0.125]]
    eng = stage_engine(amd, S)
    lib, h = eng._lib, eng._h
    kp = lambda a: a.ctypes.data_as(K.c_double_p)
    nine = np.full(9, 0.11)
    eng.set_dither(A9, 16)
    st = L.Lattice(S, 16)
    for s in range(S):
        assert list(eng.dither_get_adaptive_coeffs(s)) == list(L.DEFAULT)
    load(eng, st, sets)
    for s in range(S):
        assert list(eng.dither_get_adaptive_coeffs(s)) == L.clamp_coeffs(sets[s]) == list(st.coeffs(s))       # the clamped values
    assert same_bits_or_nan(eng.dither_process(part[0]), st.process(part[0], 1.0))
    eng.set_dither(A9, 16)                                                         # the same arguments: nothing moves
    # every refusal, then a call that proves no state moved
    for bad in ((3, 16), (-1, 16), (5, 16), (A9, 0), (A9, 33)):
        assert lib.cpq_engine_set_dither(h, bad[0], bad[1]) == K.CPQ_ERR_INVALID_ARG
    for stream, k, cnt in ((S, nine, 9), (-2, nine, 9), (0, nine, 10), (0, nine, -1), (K.CPQ_ALL_STREAMS, nine, 10)):
        assert lib.cpq_dither_set_adaptive_coeffs(h, stream, kp(k), cnt) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_dither_set_adaptive_coeffs(h, 0, None, 1) == K.CPQ_ERR_INVALID_ARG
    got = np.full(9, 7.0)
    for stream in (S, -2, K.CPQ_ALL_STREAMS):
        assert lib.cpq_dither_get_adaptive_coeffs(h, stream, kp(got)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_dither_get_adaptive_coeffs(h, 0, None) == K.CPQ_ERR_INVALID_ARG and (got == 7.0).all()
    assert lib.cpq_dither_process(h, None, None, n) == K.CPQ_ERR_INVALID_ARG
    for s in range(S):
        assert list(eng.dither_get_adaptive_coeffs(s)) == L.clamp_coeffs(sets[s])
    assert same_bits_or_nan(eng.dither_process(part[1]), st.process(part[1], 1.0))
    # a new set for stream 1 of 3: that stream's states cleared, the others' kept, every generator runs on
    eng.dither_set_adaptive_coeffs(1, [-0.6, 0.2])
    st.set_coeffs(1, [-0.6, 0.2])
    y = eng.dither_process(part[2])
    assert same_bits_or_nan(y, st.process(part[2], 1.0))
    eng.dither_set_adaptive_coeffs(2, [])                                          # n = 0 with a null pointer: all zeros
    st.set_coeffs(2, [])
    assert list(eng.dither_get_adaptive_coeffs(2)) == [0.0] * 9
    assert same_bits_or_nan(eng.dither_process(part[3]), st.process(part[3], 1.0))
    eng.dither_reset()                                                             # states only
    st.reset()
    assert same_bits_or_nan(eng.dither_process(part[4]), st.process(part[4], 1.0))
    eng.prepare_to_play(64000.0, 64 * 64)                                          # keeps the coefficients, clears the states, no reseed
    st.prepare()
    y = eng.dither_process(part[5])
    assert same_bits_or_nan(y, st.process(part[5], 1.0))
    fresh = L.Lattice(S, 16)
    for s in range(S):
        assert list(eng.dither_get_adaptive_coeffs(s)) == list(st.coeffs(s))
        fresh.set_coeffs(s, st.coeffs(s))
    assert not same_bits_or_nan(y, fresh.process(part[5], 1.0))                    # a reseeded shaper would have given these
    eng.set_dither(A9, 24)                                                         # any change: reseeded, default set everywhere
    assert same_bits_or_nan(eng.dither_process(part[0]), L.Lattice(S, 24).process(part[0], 1.0))
    for other in (M.FIXED4, M.FIXED15):
        eng.set_dither(other, 24)
        assert lib.cpq_dither_set_adaptive_coeffs(h, 0, kp(nine), 9) == K.CPQ_ERR_NOT_READY
        assert lib.cpq_dither_get_adaptive_coeffs(h, 0, kp(got)) == K.CPQ_ERR_NOT_READY and (got == 7.0).all()
        fixed = M.Dither(64000.0, S, other, 24)
        assert same_bits_or_nan(eng.dither_process(part[0]), fixed.process(part[0], 1.0))
        assert same_bits_or_nan(eng.dither_process(part[1]), fixed.process(part[1], 1.0))      # the refusals moved nothing
        eng.set_dither(A9, 24)
        eng.dither_set_adaptive_coeffs(amd.CPQ_ALL_STREAMS, STRONG)
        eng.set_dither(other, 24)
        eng.set_dither(A9, 24)                                                     # and back: defaults again, reseeded
        assert list(eng.dither_get_adaptive_coeffs(S - 1)) == list(L.DEFAULT)
        assert same_bits_or_nan(eng.dither_process(part[1]), L.Lattice(S, 24).process(part[1], 1.0))
    eng.set_dither(M.OFF)
    assert lib.cpq_dither_set_adaptive_coeffs(h, 0, kp(nine), 9) == K.CPQ_ERR_NOT_READY
    assert lib.cpq_dither_get_adaptive_coeffs(h, 0, kp(got)) == K.CPQ_ERR_NOT_READY
    assert lib.cpq_dither_reset(h) == K.CPQ_ERR_NOT_READY
    eng.close()


def test_all_streams_and_oversampling_keep_the_coefficients(amd):
    """CPQ_ALL_STREAMS loads every stream; cpq_engine_set_oversampling clears the states, keeps the sets and does not reseed"""
    S = 2
    x = signal(S, 200, 17)
    a, b = np.ascontiguousarray(x[:, :100]), np.ascontiguousarray(x[:, 100:])
    eng = stage_engine(amd, S, rate=128000.0)
    eng.set_dither(A9, 16)
    st = L.Lattice(S, 16)
    eng.dither_set_adaptive_coeffs(amd.CPQ_ALL_STREAMS, STRONG)
    st.set_coeffs(None, STRONG)
    eng.dither_set_adaptive_coeffs(1, [0.2, 0.1])
    st.set_coeffs(1, [0.2, 0.1])
    assert same_bits_or_nan(eng.dither_process(a), st.process(a, 1.0))
    eng.set_oversampling(2)
    st.prepare()
    assert list(eng.dither_get_adaptive_coeffs(0)) == STRONG and list(eng.dither_get_adaptive_coeffs(1))[:3] == [0.2, 0.1, 0.0]
    assert same_bits_or_nan(eng.dither_process(b), st.process(b, 1.0))
    eng.close()


def test_split_invariance_and_profile_name(amd):
    """cuts at 1 and 65 change nothing; the launches are counted under k_dither"""
    S = 3
    x = signal(S, 256, 9)
    sets = stream_sets(S, 4)
    out = []
    for cuts in (((0, 256),), ((0, 1), (1, 65), (65, 256))):
        eng = stage_engine(amd, S)
        eng.set_dither(A9, 16)
        ref = L.Lattice(S, 16)
        load(eng, ref, sets)
        eng.profile_enable()
        out.append(np.concatenate([eng.dither_process(np.ascontiguousarray(x[:, a:b])) for a, b in cuts], axis=1))
        prof = eng.profile_read()
        assert prof["k_dither"][0] == len(cuts) and prof["k_dither"][1] > 0.0
        eng.close()
    assert same_bits_or_nan(out[0], out[1]) and same_bits_or_nan(out[0], ref.process(x, 1.0))


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


def test_whole_chain_f32_in_s16_interleaved_out(amd, oracle, K):
    """short IR + EQ + 2x oversampling, three streams with their own sets, CPQ_OUT_ALL, 16 bits, S16 interleaved PCM out"""
    O = oracle
    S, F, B, T = 3, 2, 512, 4
    nb = B * T // F
    irs = [O.gen_ir(2000, stream=c // 2, channel=c % 2) for c in range(2 * S)]
    x = (0.25 * np.stack([O.gen_pcm(2 * nb, stream=c // 2, channel=c % 2) for c in range(2 * S)])).astype(np.float32)
    c = dict(S=S, F=F, B=B, T=T, nb=nb, irs=irs, x=x)
    sets = [STRONG, [0.4, -0.3, 0.2, -0.1], list(L.DEFAULT)]
    twin = chain_engine(amd, O, c)                                                 # the rows behind the DC blocker
    twin.set_output_stage(OM.DC_BLOCK)
    x64 = x.astype(np.float64)
    dc = np.concatenate([twin.process(np.ascontiguousarray(x64[:, o:o + nb])) for o in range(0, 2 * nb, nb)], axis=1)
    twin.close()
    eng = chain_engine(amd, O, c)
    eng.set_output_stage(OM.ALL)
    eng.set_dither(A9, 16)
    ref = L.Lattice(S, 16)
    load(eng, ref, sets)
    eng.profile_enable()
    out = []
    for o in range(0, 2 * nb, nb):
        src = PM.to_bytes(x[:, o:o + nb], PM.F32, PM.INTERLEAVED)
        raw = eng.process_pcm(src, K.CPQ_PCM_F32, K.CPQ_PCM_S16, nb, PM.INTERLEAVED)
        out.append(PM.from_bytes(raw, K.CPQ_PCM_S16, PM.INTERLEAVED, 2 * S, nb))
    assert eng.profile_read()["k_dither"][0] == 2
    env = [eng.out_read_envelope(s) for s in range(S)]
    eng.close()
    got = np.concatenate(out, axis=1)
    post = ref.process(dc, L.H, scrubbed=True)                                     # the shaper's state runs across the calls
    lim = OM.OutStage(48000.0, S)
    rows = lim.process(post, B // F, OM.LIMITER | OM.CLAMP)
    assert np.array_equal(got, L.encode16(rows)) and np.abs(got).max() > 30
    assert env == lim.env
