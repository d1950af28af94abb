"""The refusals of cpq_limiter in the order the header documents them, each with the state untouched, on the host object; the
feature define and the exported symbols."""
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
SYMBOLS = ("cpq_limiter_default_window", "cpq_limiter_create", "cpq_limiter_destroy", "cpq_limiter_last_error", "cpq_limiter_set_stream",
           "cpq_limiter_reset", "cpq_limiter_latency", "cpq_limiter_window", "cpq_limiter_set_gains", "cpq_limiter_process_device",
           "cpq_limiter_process", "cpq_limiter_flush_device", "cpq_limiter_flush", "cpq_limiter_read_telemetry", "cpq_limiter_last_kernel_ms")


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def create(n_streams=1, rate=48000.0, ceiling=-1.0, window=8, flags=K.CPQ_LIM_HOST, out=True):
    h = C.c_void_p()
    rc = K.load().cpq_limiter_create(n_streams, rate, ceiling, window, flags, C.byref(h) if out else None)
    return rc, h


def test_the_header_announces_the_feature_and_the_symbols_are_exported():
    header = open(os.path.join(ROOT, "include", "convopeq_mi355x.h")).read()
    assert "#define CPQ_HAS_TRUE_PEAK_LIMITER 1" in header and "#define CPQ_ABI_REVISION 1" in header
    assert C.sizeof(K.LimiterTelemetry) == 16
    lib = K.load()
    names = subprocess.run(["nm", "-D", "--defined-only", K.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert name in header and hasattr(lib, name) and f" T {name}\n" in names, name
        assert name in K.SYMBOLS


def test_create_refuses_in_the_documented_order():
    lib = K.load()
    E = K.CPQ_ERR_INVALID_ARG
    # each case is wrong in its own argument and in every later one of the order: the earlier rule answers
    cases = [(dict(out=False, n_streams=0), E, "null"),
             (dict(n_streams=0, flags=8), E, "n_streams"), (dict(n_streams=32768, flags=8), E, "n_streams"),
             (dict(flags=4, rate=math.nan), E, "unknown flags"),
             (dict(flags=K.CPQ_LIM_HOST | K.CPQ_LIM_DEVICE, rate=0.0), E, "exclude"),
             (dict(rate=math.inf, ceiling=math.nan), E, "sample_rate"), (dict(rate=-1.0, ceiling=math.nan), E, "sample_rate"),
             (dict(ceiling=math.nan, window=5), E, "ceiling"), (dict(ceiling=201.0, window=5), E, "ceiling"),
             (dict(window=7, rate=44105.0), E, "window"), (dict(window=1025, rate=44105.0), E, "window"), (dict(window=-1, flags=0), E, "window"),
             (dict(rate=44105.0, flags=0), K.CPQ_ERR_UNSUPPORTED, "divisible by 10"), (dict(rate=7000.0, flags=0), K.CPQ_ERR_UNSUPPORTED, "8000"),
             (dict(flags=0), K.CPQ_ERR_UNSUPPORTED, "CPQ_LIM_HOST or CPQ_LIM_DEVICE")]
    for kw, status, word in cases:
        rc, h = create(**kw)
        assert rc == status and not h.value, kw
        assert word in lib.cpq_limiter_last_error(None).decode(), (kw, lib.cpq_limiter_last_error(None))
    if not has_gpu():
        rc, h = create(flags=K.CPQ_LIM_DEVICE)
        assert rc == K.CPQ_ERR_NO_DEVICE and not h.value
        with pytest.raises(amd.CpqError) as e:
            amd.TruePeakLimiter(1, 48000, device=True)
        assert e.value.status == K.CPQ_ERR_NO_DEVICE
    with pytest.raises(amd.CpqError) as e:
        amd.TruePeakLimiter(1, 48000)
    assert e.value.status == K.CPQ_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        amd.TruePeakLimiter(1, 48000, host=True, device=True)


def test_null_handles():
    lib = K.load()
    x = np.zeros((2, 32))
    tel = K.LimiterTelemetry()
    E = K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_limiter_reset(None) == E and lib.cpq_limiter_latency(None) == E and lib.cpq_limiter_window(None) == E
    assert lib.cpq_limiter_set_stream(None, None) == E and lib.cpq_limiter_set_gains(None, x.ctypes.data_as(K.c_double_p)) == E
    assert lib.cpq_limiter_process(None, x.ctypes.data, 32, x.ctypes.data, 32, 32) == E
    assert lib.cpq_limiter_process_device(None, x.ctypes.data, 32, x.ctypes.data, 32, 32) == E
    assert lib.cpq_limiter_flush(None, x.ctypes.data, 32) == E and lib.cpq_limiter_flush_device(None, x.ctypes.data, 32) == E
    assert lib.cpq_limiter_read_telemetry(None, C.byref(tel)) == E
    assert lib.cpq_limiter_last_kernel_ms(None) == -1.0
    assert lib.cpq_limiter_default_window(math.nan) == E and lib.cpq_limiter_default_window(0.0) == E
    lib.cpq_limiter_destroy(None)


def test_call_refusals_in_order_leave_the_state_untouched():
    lib = K.load()
    E = K.CPQ_ERR_INVALID_ARG
    W, D = 8, 19
    rng = np.random.default_rng(1)
    x = 0.3 * rng.standard_normal((4, 400))
    x[1, 37] = 3.0
    x[2, 250] = -2.0
    lim = amd.TruePeakLimiter(2, 48000, -1.0, W, host=True)
    ref = amd.TruePeakLimiter(2, 48000, -1.0, W, host=True)
    for l in (lim, ref):
        l.set_gains([1.2, 0.7])
    head = lim.process(x[:, :100])
    assert np.array_equal(head.view(np.uint64), ref.process(x[:, :100]).view(np.uint64))
    h = lim._h
    big = np.full((4, 64), -7.0)
    p = lambda a: a.ctypes.data
    seg = np.ascontiguousarray(x[:, 100:132])
    flat = np.zeros(4 * 32 + 16)
    refused = [
        # process: null buffers, n, strides, partial overlap -- each wrong in every later rule as well
        (lambda: lib.cpq_limiter_process(h, None, 0, None, 0, 0), E, "null"),
        (lambda: lib.cpq_limiter_process(h, p(seg), 32, None, 0, 0), E, "null"),
        (lambda: lib.cpq_limiter_process(h, p(seg), 0, p(big), 0, 0), E, "n_samples"),
        (lambda: lib.cpq_limiter_process(h, p(seg), 0, p(big), 0, (1 << 30) + 1), E, "n_samples"),
        (lambda: lib.cpq_limiter_process(h, p(flat), 31, p(flat) + 64, 32, 32), E, "strides"),
        (lambda: lib.cpq_limiter_process(h, p(flat), 32, p(flat) + 64, 31, 32), E, "strides"),
        (lambda: lib.cpq_limiter_process(h, p(flat), 32, p(flat) + 64, 32, 32), E, "overlap"),
        (lambda: lib.cpq_limiter_process(h, p(flat), 32, p(flat), 33, 32), E, "overlap"),
        # the device entries on a host object
        (lambda: lib.cpq_limiter_process_device(h, None, 0, None, 0, 0), E, "host object"),
        (lambda: lib.cpq_limiter_flush_device(h, None, 0), E, "host object"),
        (lambda: lib.cpq_limiter_set_stream(h, None), E, "host object"),
        # flush: null, stride
        (lambda: lib.cpq_limiter_flush(h, None, 0), E, "null"),
        (lambda: lib.cpq_limiter_flush(h, p(big), D - 1), E, "stride"),
        # gains: null, value, then the programme that has started
        (lambda: lib.cpq_limiter_set_gains(h, None), E, "null"),
        (lambda: lib.cpq_limiter_set_gains(h, np.array([1.0, math.nan]).ctypes.data_as(K.c_double_p)), E, "stream 1"),
        (lambda: lib.cpq_limiter_set_gains(h, np.array([-0.5, 1.0]).ctypes.data_as(K.c_double_p)), E, "stream 0"),
        (lambda: lib.cpq_limiter_set_gains(h, np.array([math.inf, 1.0]).ctypes.data_as(K.c_double_p)), E, "stream 0"),
        (lambda: lib.cpq_limiter_set_gains(h, np.array([2.0, 2.0]).ctypes.data_as(K.c_double_p)), K.CPQ_ERR_NOT_READY, "start of a programme"),
        (lambda: lib.cpq_limiter_read_telemetry(h, None), E, "null"),
    ]
    for call, status, word in refused:
        assert call() == status, word
        assert word in lib.cpq_limiter_last_error(h).decode(), (word, lib.cpq_limiter_last_error(h))
    assert (big == -7.0).all() and not flat.any()
    assert lim.last_kernel_ms == -1.0
    # nothing moved: the rest of the programme equals the object that was never asked, gains, history and telemetry included
    for a, b in ((lim.process(x[:, 100:]), ref.process(x[:, 100:])), (lim.flush(), ref.flush())):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert lim.telemetry() == ref.telemetry() and lim.telemetry()[0]["limited_samples"] > 0
    # in place on host rows is allowed
    both = x[:, :200].copy()
    assert lib.cpq_limiter_process(h, p(both), 200, p(both), 200, 200) == K.CPQ_OK
    assert np.array_equal(both.view(np.uint64), ref.process(x[:, :200]).view(np.uint64))
