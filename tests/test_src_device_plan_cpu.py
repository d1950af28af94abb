"""The device object of cpq_src without a GPU: its launch arithmetic (csrc/src_device_plan.hpp) under sanitizers, and the
refusals of the C ABI around it (CPQ_SRC_DEVICE, cpq_src_process_device, cpq_src_set_stream, cpq_src_last_kernel_ms)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import convopeq_amd as amd
from convopeq_amd import _capi as K

HERE = os.path.dirname(os.path.abspath(__file__))


def test_launch_arithmetic_under_sanitizers(tmp_path):
    """tests/sanitize/src_device_check.cpp: k_src_resample and k_src_keep restated as host loops over grid, lanes and chunks on
    exactly sized heap blocks, under ASan and UBSan, against cpq::SrcHost bit for bit -- seven ratios, the call lengths around
    the latency and the tile, random splits, flushes in mid-stream, start periods up to 2^40, sums that underflow"""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "convopeq_amd", "csrc")
    exe = tmp_path / "src_device_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + csrc, "-I" + os.path.join(root, "include"),
                    os.path.join(HERE, "sanitize", "src_device_check.cpp"), os.path.join(csrc, "resample_design.cpp"),
                    os.path.join(csrc, "ir_ingest.cpp"), "-o", str(exe), "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failed checks" in r.stdout and "FAILED" not in r.stdout


def _create(flags, n_channels=2, a=44100, b=48000, max_in=64):
    h = C.c_void_p()
    rc = K.load().cpq_src_create(C.byref(K.SrcDesc(n_channels, a, b, max_in, 0, flags, 0)), C.byref(h))
    return rc, h


def test_the_header_announces_the_device_object():
    header = open(os.path.join(os.path.dirname(HERE), "include", "convopeq_mi355x.h")).read()
    assert "#define CPQ_HAS_STREAM_RESAMPLING 1" in header and "#define CPQ_SRC_DEVICE 2u" in header
    assert K.CPQ_SRC_DEVICE == 2 and K.CPQ_SRC_HOST == 1


def test_flag_refusals():
    lib = K.load()
    for flags, status in ((K.CPQ_SRC_HOST | K.CPQ_SRC_DEVICE, K.CPQ_ERR_INVALID_ARG), (4, K.CPQ_ERR_INVALID_ARG),
                          (K.CPQ_SRC_DEVICE | 8, K.CPQ_ERR_INVALID_ARG), (0, K.CPQ_ERR_UNSUPPORTED)):
        rc, h = _create(flags)
        assert rc == status and not h.value, flags
        assert lib.cpq_src_last_error(None)
    # what is wrong with the request comes before the question of a device
    for desc in (K.SrcDesc(0, 44100, 48000, 64, 0, K.CPQ_SRC_DEVICE, 0), K.SrcDesc(2, 44100, 48000, 0, 0, K.CPQ_SRC_DEVICE, 0)):
        h = C.c_void_p()
        assert lib.cpq_src_create(C.byref(desc), C.byref(h)) == K.CPQ_ERR_INVALID_ARG and not h.value
    h = C.c_void_p()
    assert lib.cpq_src_create(C.byref(K.SrcDesc(2, 44100.5, 48000, 64, 0, K.CPQ_SRC_DEVICE, 0)), C.byref(h)) == K.CPQ_ERR_UNSUPPORTED


def test_the_device_object_needs_a_device():
    """CPQ_ERR_NO_DEVICE where no gfx950 is visible, never the host object in its place; CPQ_OK where one is"""
    lib = K.load()
    rc, h = _create(K.CPQ_SRC_DEVICE)
    assert rc in (K.CPQ_OK, K.CPQ_ERR_NO_DEVICE)
    if rc == K.CPQ_OK:
        assert h.value
        lib.cpq_src_destroy(h)
    else:
        assert not h.value and lib.cpq_src_last_error(None)
        with pytest.raises(amd.CpqError) as e:
            amd.StreamResampler(2, 44100, 48000, 64, device=True)
        assert e.value.status == K.CPQ_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        amd.StreamResampler(2, 44100, 48000, 64, host=True, device=True)


def test_device_entry_points_on_a_host_object():
    lib = K.load()
    src = amd.StreamResampler(2, 44100, 48000, 1000, host=True)
    x = np.random.default_rng(1).uniform(-0.5, 0.5, size=(2, 700))
    count = src.out_count(700)
    out = np.zeros((2, count))
    n = C.c_int32(-7)
    assert lib.cpq_src_process_device(src._h, x.ctypes.data, 700, 700, out.ctypes.data, count, count, 0, C.byref(n)) == K.CPQ_ERR_INVALID_ARG
    assert n.value == -7 and not out.any() and lib.cpq_src_last_error(src._h)
    assert lib.cpq_src_set_stream(src._h, None) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_src_last_kernel_ms(src._h) == -1.0 and lib.cpq_src_last_kernel_ms(None) == -1.0
    assert lib.cpq_src_process_device(None, x.ctypes.data, 700, 700, out.ctypes.data, count, count, 0, C.byref(n)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_src_set_stream(None, None) == K.CPQ_ERR_INVALID_ARG
    with pytest.raises(amd.CpqError):
        src.process_device(None)
    # the refused calls moved nothing: the object gives the rows of one that was never asked
    want = amd.StreamResampler(2, 44100, 48000, 1000, host=True).process(x, flush=True)
    got = src.process(x, flush=True)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert src.last_kernel_ms == -1.0
