"""tests/pcm_model.py is the reference of the packed PCM GPU tests (test_gpu_pcm_io.py).  Here it is pinned, without a GPU, to
what the project already has: its decode to cpq_ir_load_wav bit for bit (WAV files of every input format written here, edge
values included; the loader applies the high-quality transform with the whole file as one callback, so the sanitise model is
pinned with it), its integer pack to a restatement in Python integers and fractions, its float32 pack to ndarray.astype.  And
the host-only parts of the new C ABI: cpq_pcm_bytes_per_sample, and the refusals that need no device."""
import ctypes as C
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import pcm_model as M


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def write_wav(path, payload, channels, bits, is_float, rate=48000):
    fmt = struct.pack("<HHIIHH", 3 if is_float else 1, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    data = bytes(payload)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    if len(data) & 1:
        body += b"\0"
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def int_edges(bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    v = [lo, lo + 1, hi, hi - 1, 0, 1, -1, 2, -2, hi // 2, lo // 2, 12345 % hi, -(54321 % hi), (1 << (bits - 2)) + 1]
    if bits == 32:
        v += [(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 25) + 2, (1 << 25) + 6, 0x7FFFFF7F, 0x7FFFFF80, 0x7FFFFFBF, 0x7FFFFFC0]   # ties of the float rounding
    return np.array(v, dtype=np.int64)


def float_edges():
    tiny = np.array([1, 0x007FFFFF, 0x80000001], dtype=np.uint32).view(np.float32)          # denormals
    return np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 0.5, 1e-25, -1e-25, 1e-20, 9.9e-21, 1.0000001e-20, np.nan, np.inf,
                                     -np.inf, 0.99999994, -0.99999994, 1.0000001, 3.4028235e38, 1.17549435e-38], dtype=np.float32), tiny])


@pytest.mark.parametrize("fmt,bits", [(M.S16, 16), (M.S24, 24), (M.S32, 32), (M.F32, 32)])
@pytest.mark.parametrize("frames_mod", [0, 1, 3])
def test_decode_and_sanitize_equal_the_wav_loader(amd, tmp_path, fmt, bits, frames_mod):
    from convopeq_amd import engine
    rng = np.random.default_rng(bits + frames_mod)
    if fmt == M.F32:
        edge = float_edges()
        body = rng.uniform(-1.5, 1.5, 64).astype(np.float32)
        vals = np.concatenate([edge, body, edge[::-1]])
    else:
        edge = int_edges(bits)
        body = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), 64)
        vals = np.concatenate([edge, body, edge[::-1]])
    channels = 2
    frames = (len(vals) // channels - 4) // 4 * 4 + frames_mod      # the last frames % 4 frames are the loader's scalar tail
    vals = np.concatenate([vals[:(frames - 4) * channels], vals[-4 * channels:]])       # keeps edge values at both ends
    planes = np.array(vals.reshape(frames, channels).T)             # the file is interleaved
    if fmt == M.F32:
        planes[:, -1] = [np.inf, -np.inf]                           # in the scalar tail when there is one, else in the body
        planes[:, 0] = [-np.inf, np.inf]
    payload = M.to_bytes(planes, fmt, M.INTERLEAVED)
    path = tmp_path / "edge.wav"
    write_wav(path, payload, channels, bits, fmt == M.F32)
    got, rate = engine.ir_load_wav(str(path))
    assert rate == 48000.0 and got.shape == (channels, frames)
    dec = M.decode(planes, fmt)
    want = M.sanitize(dec, frames)                                  # the whole file is one callback
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if fmt != M.F32:
        # integer codes are in [-1, 1) and, except 0, at least 2^-31 in magnitude: the transform leaves them alone -- decode itself is pinned
        assert np.array_equal(dec.view(np.uint64), want.view(np.uint64))
        if bits < 32:
            assert np.array_equal(dec, planes.astype(np.float64) / float(1 << (bits - 1)))     # S16 / S24 are exact
        else:
            assert np.array_equal(dec, planes.astype(np.float32).astype(np.float64) / 2.0 ** 31)   # 24 significant bits
    else:
        assert np.array_equal(dec.view(np.uint64), planes.astype(np.float64).view(np.uint64))


def test_sanitize_infinity_in_body_and_tail_per_callback():
    x = np.zeros((1, 23))
    x[0, [0, 3, 4, 6, 7, 13, 14, 20, 21, 22]] = [np.inf, -np.inf, np.inf, -np.inf, 2.0, np.inf, np.nan, -np.inf, 1e-25, np.inf]
    y = M.sanitize(x, 7)          # callbacks [0,7) [7,14) [14,21) and the ragged [21,23): body 4 + tail 3; the last one all tail
    want = np.zeros(23)
    want[[0, 3]] = [1.0, -1.0]    # body of callback 0
    want[7] = 1.0                 # 2.0 clamps
    #  4, 6: tail of callback 0 -> 0; 13: tail of callback 1; 14: NaN; 20: tail of callback 2; 21, 22: the ragged callback has len 2, all tail
    assert np.array_equal(y[0].view(np.uint64), want.view(np.uint64))           # every zero is +0.0
    assert np.array_equal(M.sanitize(np.array([[-0.0, -1e-21, np.inf, -np.inf]]), 4).view(np.uint64),
                          np.array([[0.0, 0.0, 1.0, -1.0]]).view(np.uint64))


def exact_pack(x, bits):
    """rint(x * 2^(bits-1)) ties to even, saturated, NaN -> 0, in integers and fractions"""
    if math.isnan(x):
        return 0
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if math.isinf(x):
        return hi if x > 0 else lo
    q = Fraction(x) * (1 << (bits - 1))
    fl = q.numerator // q.denominator
    r = q - fl
    k = fl if r < Fraction(1, 2) else fl + 1 if r > Fraction(1, 2) else fl + (fl & 1)
    return max(lo, min(hi, k))


@pytest.mark.parametrize("fmt,bits", [(M.S24, 24), (M.S32, 32)])
def test_integer_pack_equals_exact_arithmetic(fmt, bits):
    s = float(1 << (bits - 1))
    ks = [0, 1, 2, 3, 4, 5, 1000, 1001, (1 << (bits - 2)), (1 << (bits - 2)) + 1, (1 << (bits - 1)) - 3, (1 << (bits - 1)) - 2]
    vals = []
    for k in ks:
        for sign in (1.0, -1.0):
            vals += [sign * (k + 0.5) / s, sign * k / s, sign * (k + 0.25) / s, sign * (k + 0.75) / s]      # ties for even and odd k
    vals += [1.0, -1.0, (s - 1.0) / s, (s - 0.5) / s, (s - 0.50001) / s, (s - 1.5) / s, -(s + 0.5) / s, -(s + 0.49) / s, -(s + 1.5) / s,
             np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), 2.0, -2.0, 1e300, -1e300,
             np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-300, 5e-324]
    x = np.array(vals, dtype=np.float64)
    got = M.encode(x, fmt)
    want = np.array([exact_pack(float(v), bits) for v in x], dtype=np.int64)
    assert np.array_equal(got.astype(np.int64), want)
    if fmt == M.S24:
        assert np.array_equal(M.s24_from_bytes(M.s24_to_bytes(got)), got)


def test_float32_pack_equals_astype():
    x = np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1e300, -1e300, np.inf, -np.inf, 3.4028235677973366e38, 1e-45, 1e-39],
                 dtype=np.float64)
    with np.errstate(over="ignore"):
        assert np.array_equal(M.encode(x, M.F32).view(np.uint32), x.astype(np.float32).view(np.uint32))
    assert np.isnan(M.encode(np.array([np.nan]), M.F32)[0]) and M.encode(np.array([1e300]), M.F32)[0] == np.inf


def test_layouts_round_trip():
    a = np.arange(4 * 5, dtype=np.int32).reshape(4, 5)
    for fmt in (M.S16, M.S24, M.S32):
        for layout in (M.PLANAR, M.INTERLEAVED):
            b = M.to_bytes(a, fmt, layout)
            assert b.size == 4 * 5 * M.BYTES[fmt]
            assert np.array_equal(M.from_bytes(b, fmt, layout, 4, 5), a)
    inter = M.to_layout(a, M.INTERLEAVED)
    assert inter.shape == (2, 5, 2) and inter[1, 3, 0] == a[2, 3] and inter[1, 3, 1] == a[3, 3]


def test_bytes_per_sample(amd):
    from convopeq_amd import _capi as K, engine
    lib = K.load()
    for fmt, size in M.BYTES.items():
        assert lib.cpq_pcm_bytes_per_sample(fmt) == size == engine.pcm_bytes_per_sample(fmt)
    for bad in (-1, 5, 100):
        assert lib.cpq_pcm_bytes_per_sample(bad) == -1
    assert (K.CPQ_PCM_F64, K.CPQ_PCM_F32, K.CPQ_PCM_S16, K.CPQ_PCM_S24, K.CPQ_PCM_S32) == (M.F64, M.F32, M.S16, M.S24, M.S32)
    assert (K.CPQ_PCM_PLANAR, K.CPQ_PCM_INTERLEAVED, K.CPQ_PCM_SANITIZE) == (M.PLANAR, M.INTERLEAVED, 1)
    assert K.KERNEL_IDS["k_pcm"] == 10 and lib.cpq_kernel_name(10) == b"k_pcm" and lib.cpq_abi_revision() == 1


def test_entry_points_refuse_null_and_bad_enums_without_a_device(amd):
    from convopeq_amd import _capi as K
    lib = K.load()
    buf = np.zeros(64, dtype=np.float64)
    p = C.c_void_p(buf.ctypes.data)
    bad = K.CPQ_ERR_INVALID_ARG
    for fmt in (K.CPQ_PCM_F32, 99, -1):
        for layout in (K.CPQ_PCM_PLANAR, 7):
            assert lib.cpq_pcm_unpack(None, p, fmt, layout, 0, p, 4) == bad
            assert lib.cpq_pcm_unpack_device(None, p, fmt, layout, 0, p, 4) == bad
            assert lib.cpq_pcm_pack(None, p, p, fmt, layout, 4) == bad
            assert lib.cpq_pcm_pack_device(None, p, p, fmt, layout, 4) == bad
            assert lib.cpq_engine_process_block_pcm(None, p, fmt, p, fmt, layout, 0, 64) == bad
            assert lib.cpq_engine_process_block_pcm_device(None, p, fmt, p, fmt, layout, 0, 64) == bad
    assert lib.cpq_pcm_unpack(None, None, 1, 0, 0, None, 4) == bad
    assert lib.cpq_engine_process_block_pcm(None, None, 1, None, 1, 0, 0, 64) == bad
