"""The refusals of cpq_quantizer in the order the header documents them, each with the state and the destination untouched, on the
host object; the feature define and the exported symbols."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import convopeq_amd as amd
from convopeq_amd import _capi as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = ("cpq_quantizer_create", "cpq_quantizer_destroy", "cpq_quantizer_last_error", "cpq_quantizer_set_stream", "cpq_quantizer_reset",
           "cpq_quantizer_set_gains", "cpq_quantizer_set_adaptive_coeffs", "cpq_quantizer_get_adaptive_coeffs",
           "cpq_quantizer_process_device", "cpq_quantizer_process", "cpq_quantizer_last_kernel_ms")
F4, F15, A9 = K.CPQ_DITHER_FIXED4, K.CPQ_DITHER_FIXED15, K.CPQ_DITHER_ADAPTIVE9
S16, S24, S32 = K.CPQ_PCM_S16, K.CPQ_PCM_S24, K.CPQ_PCM_S32


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def create(n_streams=1, rate=48000.0, shaper=F4, bits=16, fmt=S16, flags=K.CPQ_QUANT_HOST, out=True):
    h = C.c_void_p()
    rc = K.load().cpq_quantizer_create(n_streams, rate, shaper, bits, fmt, flags, C.byref(h) if out else None)
    return rc, h


def test_the_header_announces_the_feature_and_the_symbols_are_exported():
    header = open(os.path.join(ROOT, "include", "convopeq_mi355x.h")).read()
    assert "#define CPQ_HAS_QUANTIZER 1" in header and "#define CPQ_QUANT_HOST   1u" in header and "#define CPQ_QUANT_DEVICE 2u" in header
    lib = K.load()
    names = subprocess.run(["nm", "-D", "--defined-only", K.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert name in header and hasattr(lib, name) and f" T {name}\n" in names, name
        assert name in K.SYMBOLS
    assert amd.Quantizer.__name__ in amd.__all__


def test_create_refuses_in_the_documented_order():
    lib = K.load()
    E, U = K.CPQ_ERR_INVALID_ARG, K.CPQ_ERR_UNSUPPORTED
    # each case is wrong in its own argument and in every later one of the order: the earlier rule answers
    cases = [(dict(out=False, n_streams=0), E, "null"),
             (dict(n_streams=0, flags=8), E, "n_streams"), (dict(n_streams=32768, flags=8), E, "n_streams"),
             (dict(flags=4, rate=math.nan), E, "unknown flags"),
             (dict(flags=K.CPQ_QUANT_HOST | K.CPQ_QUANT_DEVICE, rate=0.0), E, "exclude"),
             (dict(rate=math.inf, shaper=3), E, "sample_rate"), (dict(rate=-1.0, shaper=3), E, "sample_rate"),
             (dict(shaper=3, fmt=K.CPQ_PCM_F32), E, "shaper"), (dict(shaper=K.CPQ_DITHER_OFF, fmt=K.CPQ_PCM_F32), E, "shaper"),
             (dict(fmt=K.CPQ_PCM_F32, bits=0), E, "container_format"), (dict(fmt=K.CPQ_PCM_F64, bits=0), E, "container_format"),
             (dict(fmt=7, bits=0), E, "container_format"),
             (dict(bits=0, flags=0), E, "bit_depth"), (dict(bits=33, fmt=S32, flags=0), E, "bit_depth"),
             (dict(bits=17, fmt=S16, flags=0), U, "above the 16 bits"), (dict(bits=25, fmt=S24, flags=0), U, "above the 24 bits"),
             (dict(flags=0), U, "CPQ_QUANT_HOST or CPQ_QUANT_DEVICE")]
    for kw, status, word in cases:
        rc, h = create(**kw)
        assert rc == status and not h.value, kw
        assert word in lib.cpq_quantizer_last_error(None).decode(), (kw, lib.cpq_quantizer_last_error(None))
    for bits, fmt in ((1, S16), (16, S16), (24, S24), (32, S32), (1, S32)):
        rc, h = create(bits=bits, fmt=fmt)
        assert rc == K.CPQ_OK and h.value
        lib.cpq_quantizer_destroy(h)
    if not has_gpu():
        rc, h = create(flags=K.CPQ_QUANT_DEVICE)
        assert rc == K.CPQ_ERR_NO_DEVICE and not h.value
        with pytest.raises(amd.CpqError) as e:
            amd.Quantizer(1, 48000, F4, 16, device=True)
        assert e.value.status == K.CPQ_ERR_NO_DEVICE
    with pytest.raises(amd.CpqError) as e:
        amd.Quantizer(1, 48000, F4, 16)
    assert e.value.status == U
    with pytest.raises(ValueError):
        amd.Quantizer(1, 48000, F4, 16, host=True, device=True)


def test_null_handles():
    lib = K.load()
    x = np.zeros((2, 32))
    k = x.ctypes.data_as(K.c_double_p)
    E = K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_quantizer_reset(None) == E and lib.cpq_quantizer_set_stream(None, None) == E and lib.cpq_quantizer_set_gains(None, k) == E
    assert lib.cpq_quantizer_set_adaptive_coeffs(None, 0, k, 9) == E and lib.cpq_quantizer_get_adaptive_coeffs(None, 0, k) == E
    assert lib.cpq_quantizer_process(None, x.ctypes.data, 32, x.ctypes.data, 64, 0, 32) == E
    assert lib.cpq_quantizer_process_device(None, x.ctypes.data, 32, x.ctypes.data, 64, 0, 32) == E
    assert lib.cpq_quantizer_last_kernel_ms(None) == -1.0
    lib.cpq_quantizer_destroy(None)


def test_call_refusals_in_order_leave_state_and_destination_untouched():
    lib = K.load()
    E = K.CPQ_ERR_INVALID_ARG
    x = 0.3 * np.random.default_rng(1).standard_normal((4, 400))
    q = amd.Quantizer(2, 48000, A9, 16, S16, host=True)
    ref = amd.Quantizer(2, 48000, A9, 16, S16, host=True)
    for o in (q, ref):
        o.set_gains([1.2, 0.7])
    assert np.array_equal(q.process(x[:, :100]), ref.process(x[:, :100]))
    h = q._h
    p = lambda a: a.ctypes.data
    seg = np.ascontiguousarray(x[:, 100:132])
    dst = np.full(4 * 64 + 16, 0x5A, dtype=np.uint8)
    both = np.zeros(4 * 32 + 8)                                  # rows and bytes in one block: the overlap cases
    nine = np.zeros(9)
    P, I = K.CPQ_PCM_PLANAR, K.CPQ_PCM_INTERLEAVED
    refused = [
        # process: null buffers, n, layout, stride, pitch, alignment of in, of the packed side, overlap -- each wrong in every
        # later rule as well
        (lambda: lib.cpq_quantizer_process(h, None, 0, None, 0, 7, 0), E, "null"),
        (lambda: lib.cpq_quantizer_process(h, p(seg), 0, None, 0, 7, 0), E, "null"),
        (lambda: lib.cpq_quantizer_process(h, p(seg) + 4, 0, p(dst) + 1, 0, 7, 0), E, "n_samples"),
        (lambda: lib.cpq_quantizer_process(h, p(seg) + 4, 0, p(dst) + 1, 0, 7, (1 << 30) + 1), E, "n_samples"),
        (lambda: lib.cpq_quantizer_process(h, p(seg) + 4, 0, p(dst) + 1, 0, 7, 32), E, "layout"),
        (lambda: lib.cpq_quantizer_process(h, p(seg) + 4, 31, p(dst) + 1, 0, P, 32), E, "in_stride"),
        (lambda: lib.cpq_quantizer_process(h, p(seg) + 4, 32, p(dst) + 1, 63, P, 32), E, "pcm_pitch_bytes"),
        (lambda: lib.cpq_quantizer_process(h, p(seg) + 4, 32, p(dst) + 1, 127, I, 32), E, "pcm_pitch_bytes"),
        (lambda: lib.cpq_quantizer_process(h, p(seg) + 4, 32, p(dst) + 1, 64, P, 32), E, "8-byte"),
        (lambda: lib.cpq_quantizer_process(h, p(both), 32, p(both) + 9, 64, P, 32), E, "element"),
        (lambda: lib.cpq_quantizer_process(h, p(both), 32, p(both) + 8, 65, P, 32), E, "element"),
        (lambda: lib.cpq_quantizer_process(h, p(both), 32, p(both) + 8, 64, P, 32), E, "overlap"),
        (lambda: lib.cpq_quantizer_process(h, p(both), 32, p(both) + 8 * 4 * 32 - 2, 64, P, 32), E, "overlap"),
        # the device entries on a host object
        (lambda: lib.cpq_quantizer_process_device(h, None, 0, None, 0, 7, 0), E, "host object"),
        (lambda: lib.cpq_quantizer_set_stream(h, None), E, "host object"),
        # gains: null, value, then the programme that has started
        (lambda: lib.cpq_quantizer_set_gains(h, None), E, "null"),
        (lambda: lib.cpq_quantizer_set_gains(h, np.array([1.0, math.nan]).ctypes.data_as(K.c_double_p)), E, "stream 1"),
        (lambda: lib.cpq_quantizer_set_gains(h, np.array([-0.5, 1.0]).ctypes.data_as(K.c_double_p)), E, "stream 0"),
        (lambda: lib.cpq_quantizer_set_gains(h, np.array([math.inf, 1.0]).ctypes.data_as(K.c_double_p)), E, "stream 0"),
        (lambda: lib.cpq_quantizer_set_gains(h, np.array([2.0, 2.0]).ctypes.data_as(K.c_double_p)), K.CPQ_ERR_NOT_READY, "start of a programme"),
        # adaptive coefficients: stream, n, null
        (lambda: lib.cpq_quantizer_set_adaptive_coeffs(h, 2, None, 10), E, "stream 2"),
        (lambda: lib.cpq_quantizer_set_adaptive_coeffs(h, -2, None, 10), E, "stream -2"),
        (lambda: lib.cpq_quantizer_set_adaptive_coeffs(h, 0, None, 10), E, "coefficients outside"),
        (lambda: lib.cpq_quantizer_set_adaptive_coeffs(h, 0, None, -1), E, "coefficients outside"),
        (lambda: lib.cpq_quantizer_set_adaptive_coeffs(h, K.CPQ_ALL_STREAMS, None, 3), E, "null coefficients"),
    ]
    for call, status, word in refused:
        assert call() == status, word
        assert word in lib.cpq_quantizer_last_error(h).decode(), (word, lib.cpq_quantizer_last_error(h))
    assert (dst == 0x5A).all() and not both.any()
    assert lib.cpq_quantizer_get_adaptive_coeffs(h, 2, nine.ctypes.data_as(K.c_double_p)) == E
    assert lib.cpq_quantizer_get_adaptive_coeffs(h, K.CPQ_ALL_STREAMS, nine.ctypes.data_as(K.c_double_p)) == E
    assert lib.cpq_quantizer_get_adaptive_coeffs(h, 0, None) == E
    assert q.last_kernel_ms == -1.0
    # nothing moved: the rest of the programme equals the object that was never asked, gains, states and coefficients included
    assert np.array_equal(q.process(x[:, 100:]), ref.process(x[:, 100:]))
    assert np.array_equal(q.adaptive_coeffs(1), ref.adaptive_coeffs(1))
    # rows and bytes that only touch are allowed
    touching = np.zeros(4 * 32 + 4 * 8)
    assert lib.cpq_quantizer_process(h, p(touching), 32, p(touching) + 8 * 4 * 32, 64, P, 32) == K.CPQ_OK


def test_the_fixed_shapers_have_no_adaptive_coefficients():
    lib = K.load()
    nine = np.zeros(9)
    for shaper in (F4, F15):
        q = amd.Quantizer(1, 48000, shaper, 16, S24, host=True)
        assert lib.cpq_quantizer_set_adaptive_coeffs(q._h, 0, nine.ctypes.data_as(K.c_double_p), 9) == K.CPQ_ERR_NOT_READY
        assert "adaptive" in lib.cpq_quantizer_last_error(q._h).decode()
        assert lib.cpq_quantizer_get_adaptive_coeffs(q._h, 0, nine.ctypes.data_as(K.c_double_p)) == K.CPQ_ERR_NOT_READY
