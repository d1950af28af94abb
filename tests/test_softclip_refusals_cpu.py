"""The soft clipper's refusals that need no device, cpq_soft_clip_latency, and what the interface announces.  The refusals of
an engine that exists (stream out of range, amount out of range, clipper off, row arguments), each before any state moves, are
in tests/test_gpu_soft_clip.py: an engine needs a device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import convopeq_amd as amd
from convopeq_amd import _capi as K

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_header_announces_the_stage():
    header = open(os.path.join(os.path.dirname(HERE), "include", "convopeq_mi355x.h")).read()
    assert "#define CPQ_HAS_SOFT_CLIP 1" in header and "#define CPQ_ABI_VERSION 2" in header and "#define CPQ_ABI_REVISION 1" in header
    assert "CPQ_K_SOFTCLIP = 14" in header and "Not built: the soft clipper" not in header
    lib = K.load()
    assert lib.cpq_abi_version() == 2 and lib.cpq_abi_revision() == 1
    assert K.CPQ_K_SOFTCLIP == 14 and lib.cpq_kernel_name(14) == b"k_soft_clip"
    assert lib.cpq_kernel_name(13) == b"?" and lib.cpq_kernel_name(15) == b"?" and "k_soft_clip" not in K.KERNEL_IDS


def test_latency():
    lib = K.load()
    assert lib.cpq_soft_clip_latency(1) == 15.0 == amd.soft_clip_latency(1)
    for factor in (2, 4, 8, 0, 3, 16, -1):
        assert lib.cpq_soft_clip_latency(factor) == 0.0
    # the 31-tap stage, up and down: 2 * 15 samples at twice the rate
    info, _ = amd.os_design_stage(2, amd.CPQ_OS_IIR)
    assert info["taps"] == 31 and info["conv_count"] == 16 and 2 * info["center_tap"] / 2 == 15.0


@pytest.mark.parametrize("bad", (-1.0e-6, 1.0 + 1.0e-6, -1.0, 2.0, math.nan, math.inf, -math.inf))
def test_amounts_outside_the_setters_range_are_refused(bad):
    lib = K.load()
    t, k, a = C.c_double(-1.0), C.c_double(-1.0), C.c_double(-1.0)
    assert lib.cpq_soft_clip_params(bad, C.byref(t), C.byref(k), C.byref(a)) == K.CPQ_ERR_INVALID_ARG
    assert (t.value, k.value, a.value) == (-1.0, -1.0, -1.0)
    x = np.array([2.0, -2.0, 0.1])
    assert lib.cpq_soft_clip_host(x.ctypes.data_as(C.POINTER(C.c_double)), 3, 3, bad) == K.CPQ_ERR_INVALID_ARG
    assert x.tolist() == [2.0, -2.0, 0.1]
    with pytest.raises(amd.CpqError) as e:
        amd.soft_clip_params(bad)
    assert e.value.status == K.CPQ_ERR_INVALID_ARG


def test_the_ends_of_the_range_are_admitted():
    assert amd.soft_clip_params(0.0) == (0.95, 0.05, 0.0)
    assert amd.soft_clip_params(1.0) == (0.95 - 0.45, 0.05 + 0.35, 0.10)


def test_host_entry_refusals_leave_the_row_alone():
    lib = K.load()
    x = np.array([2.0, -2.0, 0.1])
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    t = C.c_double()
    assert lib.cpq_soft_clip_host(None, 3, 3, 0.5) == K.CPQ_ERR_INVALID_ARG
    for n, cb in ((0, 3), (-1, 3), (3, 0), (3, -4)):
        assert lib.cpq_soft_clip_host(p, n, cb, 0.5) == K.CPQ_ERR_INVALID_ARG
    assert x.tolist() == [2.0, -2.0, 0.1]
    assert lib.cpq_soft_clip_params(0.5, None, C.byref(t), C.byref(t)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_soft_clip_params(0.5, C.byref(t), None, C.byref(t)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_soft_clip_params(0.5, C.byref(t), C.byref(t), None) == K.CPQ_ERR_INVALID_ARG


def test_null_handles():
    lib = K.load()
    x = np.zeros((2, 16))
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    tel = K.OsTelemetry()
    assert lib.cpq_engine_set_soft_clip(None, 0, 1, 0.5) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_soft_clip_reset(None) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_soft_clip_process(None, p, p, 16, 16) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_soft_clip_process_device(None, x.ctypes.data, x.ctypes.data, 16, 16) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_soft_clip_read_telemetry(None, 0, C.byref(tel)) == K.CPQ_ERR_INVALID_ARG
    assert not x.any()
