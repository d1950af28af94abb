"""GPU tests of the packed PCM entry points (cpq_pcm_unpack / cpq_pcm_pack / cpq_engine_process_block_pcm and their _device
variants; kernels in convopeq_amd/csrc/pcm_kernels.hip) against tests/pcm_model.py.  Every comparison is bit for bit (NaNs as
NaN, not by payload); there is no tolerance in this file.

The converter tests drive the kernels on device buffers (torch tensors) that carry guard regions of a sentinel on both sides
of the destination: a store outside the destination changes a guard.  Sizes: the ends of a row (1, 2, 3, 5), the 16-byte slot
(15, 16, 17), and the kernel's tile -- kPcmTile (kernels.hpp) = 4096 samples of a planar row or 2048 stereo frames of an
interleaved stream per workgroup -- from both sides: 2047 / 2049 and 4095 / 4096 / 4097.  With S = 3 and odd n the rows start
on odd bytes (S24), off 16-byte slots (S16, F32, S32) and on odd doubles.

cpq_engine_process_block_pcm has ONE layout argument for both buffers, so "same pointer, different layouts" cannot be said
through the ABI; the same pointer with different formats is what test_aliasing refuses."""
import ctypes as C

import numpy as np
import pytest

import pcm_model as M

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 5, 15, 16, 17, 2047, 2049, 4095, 4096, 4097]
SEAMS = [0, 1, 2047, 2048, 2049, 4095, 4096]          # first samples, both tile seams; mirrored from the end of the row as well
GUARD = 64


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def converters(amd):
    """engines that only convert, per stream count; callbacks of 64 (the sanitise tests make their own)"""
    engs = {S: amd.BatchedEngine(S, block_size=64, max_ir_len=256, max_blocks_per_call=128, call_mode=amd.CPQ_CALLS_ANY) for S in (1, 3)}
    yield engs
    for e in engs.values():
        e.close()


def same_bits(a, b):
    """equal bit for bit, NaNs as NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def edge_positions(n):
    pos = sorted({p for p in SEAMS if p < n} | {n - 1 - p for p in SEAMS if p < n})
    return pos


def input_samples(fmt, channels, n, seed):
    """[channels][n] of the format's dtype (S24: codes): random, with the format's edge values at row ends and tile seams"""
    rng = np.random.default_rng(seed)
    if fmt in (M.F32, M.F64):
        dt = M.DTYPE[fmt]
        a = rng.uniform(-1.5, 1.5, (channels, n)).astype(dt)
        tiny = np.array([1, 0x007FFFFF, 0x80000001], dtype=np.uint32).view(np.float32).astype(dt)       # float denormals
        edge = np.concatenate([np.array([np.nan, np.inf, -np.inf, 1e-25, -0.0, 2.0, -2.0, 1.0, -1.0, 0.0], dtype=dt), tiny])
    else:
        bits = {M.S16: 16, M.S24: 24, M.S32: 32}[fmt]
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        a = rng.integers(lo, hi + 1, (channels, n)).astype(np.int64)
        edge = np.array([lo, hi, lo + 1, hi - 1, 1, -1, 0] + ([(1 << 24) + 1, (1 << 24) + 3, 0x7FFFFFBF, 0x7FFFFFC0] if bits == 32 else []), dtype=np.int64)
    for c in range(channels):
        for j, p in enumerate(edge_positions(n)):
            a[c, p] = edge[(j + 3 * c) % len(edge)]
    return a if fmt in (M.F32, M.F64) else a.astype(np.int32)


def device_bytes(torch, payload, lead):
    """the bytes on the device behind `lead` bytes of padding (lead = 1: an odd base address); (tensor, address)"""
    t = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), np.ascontiguousarray(payload).view(np.uint8).reshape(-1)])).cuda()
    return t, t.data_ptr() + lead


def run_unpack(torch, eng, samples, fmt, layout, flags=0):
    """cpq_pcm_unpack_device into a guarded destination; returns rows [channels][n]"""
    channels, n = samples.shape
    lead = 1 if fmt == M.S24 and n % 2 else 0
    src, src_ptr = device_bytes(torch, M.to_bytes(samples, fmt, layout), lead)
    sentinel = -7.25e77
    dst = torch.full((GUARD + channels * n + GUARD,), sentinel, dtype=torch.float64, device="cuda")
    eng.pcm_unpack_device(src_ptr, fmt, dst.data_ptr() + 8 * GUARD, n, layout, flags)
    eng.synchronize()
    out = dst.cpu().numpy()
    assert np.all(out[:GUARD] == sentinel) and np.all(out[-GUARD:] == sentinel), "store outside the destination rows"
    del src
    return out[GUARD:-GUARD].reshape(channels, n)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("layout", [M.PLANAR, M.INTERLEAVED])
@pytest.mark.parametrize("fmt", [M.F64, M.F32, M.S16, M.S24, M.S32])
def test_unpack_equals_model(torch, converters, fmt, layout, S):
    eng = converters[S]
    for n in NS:
        samples = input_samples(fmt, 2 * S, n, seed=100 * fmt + n)
        got = run_unpack(torch, eng, samples, fmt, layout)
        assert same_bits(got, M.decode(samples, fmt)), (fmt, layout, S, n)


@pytest.mark.parametrize("layout", [M.PLANAR, M.INTERLEAVED])
@pytest.mark.parametrize("cb,n", [(64, 229), (441, 4300), (7, 37)])
def test_unpack_sanitize(amd, torch, cb, n, layout):
    """callbacks of cb samples and a ragged last one (37, 331 and 2 samples): an infinity in the 4-wide body of a callback reads
    +-1, in the scalar tail (the last len % 4 samples of the callback) 0; NaN and 1e-25 read +0.0, 2.0 reads 1.0"""
    S = 2
    eng = amd.BatchedEngine(S, block_size=cb, max_ir_len=256, max_blocks_per_call=16, call_mode=amd.CPQ_CALLS_ANY)
    try:
        rng = np.random.default_rng(cb)
        x = rng.uniform(-1.5, 1.5, (2 * S, n)).astype(np.float32)
        last = n // cb * cb                       # start of the ragged callback ...
        if n - last < 4:
            last = 2 * cb                         # ... which is all scalar tail when shorter than 4: the start of callback 2 instead
        tail_full = cb + cb // 4 * 4              # first scalar-tail sample of callback 1 (none when cb % 4 == 0)
        x[0, 0], x[1, cb + 1], x[2, last], x[3, 3] = np.inf, -np.inf, np.inf, -np.inf                     # bodies
        x[0, n - 1], x[1, n - 1] = np.inf, -np.inf                                                        # tail of the ragged callback
        if cb % 4:
            x[2, tail_full], x[3, 2 * cb - 1] = -np.inf, np.inf                                           # tail of a whole callback
        x[0, 5], x[1, 6], x[2, 9], x[3, 10], x[0, 11] = np.nan, 1e-25, 2.0, -2.0, -0.0
        got = run_unpack(torch, eng, x, M.F32, layout, flags=amd._capi.CPQ_PCM_SANITIZE)
        assert same_bits(got, M.sanitize(M.decode(x, M.F32), cb))
        assert (got[0, 0], got[1, cb + 1], got[2, last], got[3, 3]) == (1.0, -1.0, 1.0, -1.0)
        assert got[0, n - 1] == 0.0 and got[1, n - 1] == 0.0 and not np.signbit(got[:2, n - 1]).any()
        if cb % 4:
            assert got[2, tail_full] == 0.0 and got[3, 2 * cb - 1] == 0.0
        assert [got[0, 5], got[1, 6], got[2, 9], got[3, 10], got[0, 11]] == [0.0, 0.0, 1.0, -1.0, 0.0]
        assert not np.signbit(got[[0, 1, 0], [5, 6, 11]]).any() and np.abs(got).max() <= 1.0
        # integers through the same option: bit-equal to the model (only exact zeros and in-range codes exist)
        codes = input_samples(M.S24, 2 * S, n, seed=cb)
        assert same_bits(run_unpack(torch, eng, codes, M.S24, layout, flags=1), M.sanitize(M.decode(codes, M.S24), cb))
    finally:
        eng.close()


def output_rows(fmt, channels, n, seed):
    """fp64 rows with the pack edge cases at row ends and tile seams: ties, saturation on both sides, NaN, +-Inf, 1e300"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.2, 1.2, (channels, n))
    s = float(1 << ({M.S24: 24, M.S32: 32}.get(fmt, 24) - 1))
    edge = np.array([0.5 / s, 1.5 / s, 2.5 / s, -0.5 / s, -1.5 / s, -2.5 / s, 1.0, -1.0, (s - 1.0) / s, (s - 0.5) / s, (s - 1.5) / s,
                     -(s + 0.5) / s, -(s + 1.5) / s, np.nan, np.inf, -np.inf, 1e300, -1e300, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1e-45,
                     np.nextafter(1.0, 0.0), -0.0])
    for c in range(channels):
        for j, p in enumerate(edge_positions(n)):
            a[c, p] = edge[(j + 5 * c) % len(edge)]
    return a


def run_pack(torch, eng, rows, fmt, layout):
    """cpq_pcm_pack_device into a guarded destination; returns the packed bytes"""
    channels, n = rows.shape
    nbytes = channels * n * M.BYTES[fmt]
    lead = GUARD + (1 if fmt == M.S24 and n % 2 else 0)
    src = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    dst = torch.full((lead + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    eng.pcm_pack_device(src.data_ptr(), dst.data_ptr() + lead, fmt, n, layout)
    eng.synchronize()
    out = dst.cpu().numpy()
    assert np.all(out[:lead] == 0xA5) and np.all(out[lead + nbytes:] == 0xA5), "store outside the destination bytes"
    return out[lead:lead + nbytes]


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("layout", [M.PLANAR, M.INTERLEAVED])
@pytest.mark.parametrize("fmt", [M.F64, M.F32, M.S24, M.S32])
def test_pack_equals_model(torch, converters, fmt, layout, S):
    eng = converters[S]
    for n in NS:
        rows = output_rows(fmt, 2 * S, n, seed=7 * fmt + n)
        got = M.from_bytes(run_pack(torch, eng, rows, fmt, layout), fmt, layout, 2 * S, n)
        assert same_bits(got, M.encode(rows, fmt)), (fmt, layout, S, n)
    if fmt == M.F32:
        probe = np.zeros((2 * S, 16))
        probe[0, :2] = [1e300, -1e300]
        got = M.from_bytes(run_pack(torch, eng, probe, fmt, layout), fmt, layout, 2 * S, 16)
        assert got[0, 0] == np.inf and got[0, 1] == -np.inf


def test_s16_output_is_refused_and_leaves_the_destination(amd, torch, converters):
    eng = converters[1]
    K = amd._capi
    rows = torch.zeros(2 * 64, dtype=torch.float64, device="cuda")
    dst = torch.full((1024,), 0xA5, dtype=torch.uint8, device="cuda")
    for layout in (M.PLANAR, M.INTERLEAVED):
        assert eng._lib.cpq_pcm_pack_device(eng._h, C.c_void_p(rows.data_ptr()), C.c_void_p(dst.data_ptr()), M.S16, layout, 64) == K.CPQ_ERR_UNSUPPORTED
    host = np.full(1024, 0xA5, dtype=np.uint8)
    hrows = np.zeros((2, 64))
    assert eng._lib.cpq_pcm_pack(eng._h, C.c_void_p(hrows.ctypes.data), C.c_void_p(host.ctypes.data), M.S16, M.PLANAR, 64) == K.CPQ_ERR_UNSUPPORTED
    eng.synchronize()
    assert np.all(dst.cpu().numpy() == 0xA5) and np.all(host == 0xA5)
    # the other refusals of the converters
    assert eng._lib.cpq_pcm_pack_device(eng._h, C.c_void_p(rows.data_ptr()), C.c_void_p(dst.data_ptr()), 9, M.PLANAR, 64) == K.CPQ_ERR_INVALID_ARG
    assert eng._lib.cpq_pcm_unpack_device(eng._h, C.c_void_p(dst.data_ptr()), M.F32, 2, 0, C.c_void_p(rows.data_ptr()), 64) == K.CPQ_ERR_INVALID_ARG
    assert eng._lib.cpq_pcm_unpack_device(eng._h, C.c_void_p(dst.data_ptr()), M.F32, 0, 2, C.c_void_p(rows.data_ptr()), 64) == K.CPQ_ERR_INVALID_ARG
    assert eng._lib.cpq_pcm_unpack_device(eng._h, C.c_void_p(dst.data_ptr() + 2), M.F32, 0, 0, C.c_void_p(rows.data_ptr()), 64) == K.CPQ_ERR_INVALID_ARG
    assert eng._lib.cpq_pcm_unpack_device(eng._h, C.c_void_p(dst.data_ptr()), M.F32, 0, 0, C.c_void_p(rows.data_ptr()), 0) == K.CPQ_ERR_INVALID_ARG


def test_host_converters_equal_model(converters):
    """the host-pointer converters (upload, kernel, download) on S = 3, odd n"""
    eng = converters[3]
    n = 4097
    for fmt in (M.F32, M.S16, M.S24, M.S32):
        for layout in (M.PLANAR, M.INTERLEAVED):
            samples = input_samples(fmt, 6, n, seed=fmt)
            assert same_bits(eng.pcm_unpack(M.to_bytes(samples, fmt, layout), fmt, n, layout), M.decode(samples, fmt))
    for fmt in (M.F32, M.S24, M.S32):
        for layout in (M.PLANAR, M.INTERLEAVED):
            rows = output_rows(fmt, 6, n, seed=fmt)
            got = M.from_bytes(eng.pcm_pack(rows, fmt, layout), fmt, layout, 6, n)
            assert same_bits(got, M.encode(rows, fmt))


# ------------------------------------------------------------------------------------------------------- whole chain
S_CHAIN, BLOCK, T_CHAIN = 2, 64, 32


def _copy_params(po, pa):
    for i in range(20):
        b, o = pa.bands[i], po.bands[i]
        b.frequency, b.gain, b.q, b.enabled, b.type, b.channel_mode = o.frequency, o.gain, o.q, o.enabled, o.type, o.channelMode
    pa.nonlinear_saturation = po.nonlinearSaturation
    pa.total_gain_db = po.totalGainDb
    pa.filter_structure = po.filterStructure
    pa.agc_enabled = po.agcEnabled
    return pa


def chain_engine(amd, O):
    """block 64 / partition 64, 256-tap IRs, two streams, EQ on"""
    eng = amd.BatchedEngine(S_CHAIN, block_size=BLOCK, max_ir_len=256, max_blocks_per_call=T_CHAIN, partition_size=BLOCK)
    assert eng.partition_size() == BLOCK
    eng.prepare_to_play(48000.0, BLOCK * T_CHAIN)
    for s in range(S_CHAIN):
        eng.set_impulse(s, O.gen_ir(256, stream=s, channel=0), O.gen_ir(256, stream=s, channel=1))
    eng.set_eq_params(amd.CPQ_ALL_STREAMS, _copy_params(O.eq_params_bench(0.2), amd.eq_params_default()))
    return eng


def reset(eng):
    eng.conv_reset()
    eng.eq_reset()
    if eng.os_factor > 1:
        eng.os_reset()


class Pinned:
    """cpq_host_register around numpy buffers"""
    def __init__(self, eng, bufs, on):
        self.eng, self.bufs = eng, (bufs if on else [])

    def __enter__(self):
        for b in self.bufs:
            assert self.eng._lib.cpq_host_register(C.c_void_p(b.ctypes.data), b.nbytes) == 0
        return self

    def __exit__(self, *a):
        for b in self.bufs:
            assert self.eng._lib.cpq_host_unregister(C.c_void_p(b.ctypes.data)) == 0


def run_f64(eng, x, pin):
    """cpq_engine_process_block after a reset, on buffers of the given pinnedness"""
    reset(eng)
    x = np.ascontiguousarray(x)
    y = np.empty_like(x)
    with Pinned(eng, [x, y], pin):
        eng._ck(eng._lib.cpq_engine_process_block(eng._h, x.ctypes.data_as(C.POINTER(C.c_double)), y.ctypes.data_as(C.POINTER(C.c_double)), x.shape[1]))
    return y


def run_pcm(eng, samples, in_fmt, out_fmt, layout, pin, flags=0):
    """cpq_engine_process_block_pcm after a reset; returns [channels][n] of the output format's dtype (S24: codes)"""
    reset(eng)
    channels, n = samples.shape
    src = M.to_bytes(samples, in_fmt, layout)
    dst = np.empty(channels * n * M.BYTES[out_fmt], dtype=np.uint8)
    with Pinned(eng, [src, dst], pin):
        eng.process_pcm(src, in_fmt, out_fmt, n, layout, flags, out=dst)
    return M.from_bytes(dst, out_fmt, layout, channels, n)


def chain_input(fmt, n, seed=3):
    rng = np.random.default_rng(seed)
    if fmt == M.F32:
        return rng.uniform(-0.5, 0.5, (2 * S_CHAIN, n)).astype(np.float32)
    return rng.integers(-(1 << 22), 1 << 22, (2 * S_CHAIN, n)).astype(np.int32)          # S24 codes at about -6 dB


@pytest.fixture(scope="module")
def chain(amd, oracle):
    eng = chain_engine(amd, oracle)
    yield eng
    eng.close()


@pytest.mark.parametrize("pin,n", [(False, 512), (True, 2048)])
def test_whole_chain_equals_fp64_call_narrowed(chain, pin, n):
    """pageable at n = 512 (one upload, one download) and cpq_host_register'ed at n = 2048 (T = 32: the four-chunk path); the
    fp64 comparison call has the same pinnedness and n"""
    eng = chain
    for in_fmt, out_fmt, layout in ((M.F32, M.F32, M.PLANAR), (M.S24, M.S32, M.PLANAR), (M.F32, M.F32, M.INTERLEAVED)):
        samples = chain_input(in_fmt, n)
        x64 = M.decode(samples, in_fmt)
        y1, y2 = run_f64(eng, x64, pin), run_f64(eng, x64, pin)
        assert same_bits(y1, y2), "the fp64 call is not reproducible at this shape"
        assert np.abs(y1).max() > 1e-3
        got = run_pcm(eng, samples, in_fmt, out_fmt, layout, pin)
        assert same_bits(got, M.encode(y1, out_fmt)), (in_fmt, out_fmt, layout, pin)


def test_device_variant_equals_host_variant(torch, chain):
    eng = chain
    n = 512
    for in_fmt, out_fmt, layout in ((M.F32, M.F32, M.PLANAR), (M.S24, M.S32, M.INTERLEAVED)):
        samples = chain_input(in_fmt, n, seed=5)
        want = run_pcm(eng, samples, in_fmt, out_fmt, layout, False)
        reset(eng)
        src = torch.from_numpy(M.to_bytes(samples, in_fmt, layout)).cuda()
        dst = torch.zeros(samples.size * M.BYTES[out_fmt], dtype=torch.uint8, device="cuda")
        eng.process_pcm_device(src.data_ptr(), in_fmt, dst.data_ptr(), out_fmt, n, layout)
        eng.synchronize()
        assert same_bits(M.from_bytes(dst.cpu().numpy(), out_fmt, layout, samples.shape[0], n), want)


def test_with_oversampling(amd, oracle):
    eng = chain_engine(amd, oracle)
    try:
        eng.set_oversampling(2, amd.CPQ_OS_IIR)
        n = 512                                   # base-rate samples in and out; the routing runs 1024
        samples = chain_input(M.F32, n, seed=7)
        y1, y2 = run_f64(eng, M.decode(samples, M.F32), False), run_f64(eng, M.decode(samples, M.F32), False)
        assert same_bits(y1, y2) and y1.shape == (2 * S_CHAIN, n)
        assert same_bits(run_pcm(eng, samples, M.F32, M.F32, M.PLANAR, False), M.encode(y1, M.F32))
        codes = chain_input(M.S24, n, seed=8)
        y = run_f64(eng, M.decode(codes, M.S24), False)
        assert same_bits(run_pcm(eng, codes, M.S24, M.S24, M.INTERLEAVED, False), M.encode(y, M.S24))
    finally:
        eng.close()


def test_with_metering(amd, oracle):
    eng = chain_engine(amd, oracle)
    try:
        eng.set_metering(amd.CPQ_METER_LOUDNESS | amd.CPQ_METER_TRUE_PEAK)
        n = 512
        samples = chain_input(M.F32, n, seed=9)
        eng.meter_reset()
        y = run_f64(eng, M.decode(samples, M.F32), False)
        rec64, _ = eng.meter_read_blocks()
        eng.meter_reset()
        got = run_pcm(eng, samples, M.F32, M.F32, M.PLANAR, False)
        rec_pcm, _ = eng.meter_read_blocks()
        assert same_bits(got, M.encode(y, M.F32))
        assert rec64.shape == (S_CHAIN, n // BLOCK) and rec_pcm.tobytes() == rec64.tobytes()
        assert "k_pcm" not in eng.profile_read()
        eng.profile_enable(True)
        run_pcm(eng, samples, M.F32, M.F32, M.PLANAR, False)
        assert eng.profile_read()["k_pcm"][0] == 2          # one unpack, one pack
        eng.profile_enable(False)
    finally:
        eng.close()


def test_aliasing(amd, oracle):
    K = amd._capi
    eng, twin = chain_engine(amd, oracle), chain_engine(amd, oracle)
    try:
        n = 512
        samples = chain_input(M.F32, n, seed=11)
        want = run_pcm(eng, samples, M.F32, M.F32, M.PLANAR, False)
        reset(eng)
        buf = M.to_bytes(samples, M.F32, M.PLANAR).copy()
        eng.process_pcm(buf, M.F32, M.F32, n, M.PLANAR, out=buf)                        # in place
        assert same_bits(M.from_bytes(buf, M.F32, M.PLANAR, 2 * S_CHAIN, n), want)

        reset(eng)
        reset(twin)
        buf = np.zeros(2 * 4 * S_CHAIN * n * 4 + 64, dtype=np.uint8)
        base = buf.ctypes.data + (-buf.ctypes.data % 16)
        call = eng._lib.cpq_engine_process_block_pcm
        before = np.frombuffer(buf, dtype=np.uint8).copy()
        for layout in (M.PLANAR, M.INTERLEAVED):
            assert call(eng._h, C.c_void_p(base), M.F32, C.c_void_p(base), M.S32, layout, 0, n) == K.CPQ_ERR_INVALID_ARG    # same pointer, other format
        total = 2 * S_CHAIN * n * 4
        assert call(eng._h, C.c_void_p(base), M.F32, C.c_void_p(base + total - 16), M.F32, M.PLANAR, 0, n) == K.CPQ_ERR_INVALID_ARG    # overlapping
        assert call(eng._h, C.c_void_p(base + 16), M.F32, C.c_void_p(base), M.S32, M.INTERLEAVED, 0, n) == K.CPQ_ERR_INVALID_ARG
        assert b"overlap" in eng._lib.cpq_last_error(eng._h)
        assert call(eng._h, C.c_void_p(base), M.F32, C.c_void_p(base + total), M.S16, M.PLANAR, 0, n) == K.CPQ_ERR_UNSUPPORTED
        assert call(eng._h, C.c_void_p(base), M.F32, C.c_void_p(base + total), M.F32, M.PLANAR, 0, n + 1) == K.CPQ_ERR_INVALID_ARG   # not whole blocks
        assert np.array_equal(buf, before)
        assert call(eng._h, C.c_void_p(base), M.F32, C.c_void_p(base + total), M.F32, M.PLANAR, 0, n) == K.CPQ_OK                   # touching ranges are fine
        # the refusals moved no state: after them eng answers like its untouched twin (the accepted call above was on silence)
        reset(eng)
        x64 = M.decode(samples, M.F32)
        x = np.ascontiguousarray(x64)
        ya, yb = np.empty_like(x), np.empty_like(x)
        reset(twin)
        eng2 = chain_engine(amd, oracle)
        try:
            for layout in (M.PLANAR, M.INTERLEAVED):
                assert call(eng2._h, C.c_void_p(base), M.F32, C.c_void_p(base), M.S32, layout, 0, n) == K.CPQ_ERR_INVALID_ARG
            assert call(eng2._h, C.c_void_p(base), M.F32, C.c_void_p(base + total - 16), M.F32, M.PLANAR, 0, n) == K.CPQ_ERR_INVALID_ARG
            dp = C.POINTER(C.c_double)
            eng2._ck(eng2._lib.cpq_engine_process_block(eng2._h, x.ctypes.data_as(dp), ya.ctypes.data_as(dp), n))   # no reset in between
            twin._ck(twin._lib.cpq_engine_process_block(twin._h, x.ctypes.data_as(dp), yb.ctypes.data_as(dp), n))
            assert same_bits(ya, yb) and np.abs(ya).max() > 1e-3
        finally:
            eng2.close()
    finally:
        eng.close()
        twin.close()
