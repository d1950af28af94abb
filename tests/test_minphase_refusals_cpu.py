"""cpq_ir_minimum_phase_batch and cpq_ir_prepare_batch without a device: what is refused before anything is allocated, the per-IR
status of an IR the reference skips, and the batch's host-only mode (CPQ_PHASE_AS_IS) against cpq_ir_prepare, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import convopeq_amd as amd
from convopeq_amd import _capi as K


def buffers(arrays):
    keep = [np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for a in arrays]
    bufs = (K.IrBuffer * len(keep))(*[K.IrBuffer(a.shape[0], a.shape[1], 48000.0, a.ctypes.data_as(K.c_double_p)) for a in keep])
    ptrs = (C.POINTER(K.IrBuffer) * len(keep))(*[C.pointer(bufs[i]) for i in range(len(keep))])
    return keep, bufs, ptrs


def noise(shape, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, size=shape)


def test_call_refusals_leave_outputs_zeroed():
    lib = K.load()
    keep, bufs, ptrs = buffers([noise((1, 16), 1), noise((2, 8), 2)])
    outs = (K.IrBuffer * 2)()
    status = (C.c_int32 * 2)()

    def poisoned():
        for o in outs:
            o.n_channels, o.n_samples, o.sample_rate = 7, 7, 7.0
        return outs

    assert lib.cpq_ir_minimum_phase_batch(ptrs, -1, 0, outs, status) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_ir_minimum_phase_batch(None, 2, 0, outs, status) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_ir_minimum_phase_batch(ptrs, 2, 0, None, status) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_ir_minimum_phase_batch(ptrs, 2, 0, outs, None) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_ir_minimum_phase_batch(ptrs, 2, -1, outs, status) == K.CPQ_ERR_INVALID_ARG
    for broken in ("null", "channels", "samples", "data"):
        keep2, bufs2, ptrs2 = buffers([noise((1, 16), 1), noise((2, 8), 2)])
        if broken == "null":
            ptrs2[1] = C.POINTER(K.IrBuffer)()
        elif broken == "channels":
            bufs2[1].n_channels = 0
        elif broken == "samples":
            bufs2[1].n_samples = 0
        else:
            bufs2[1].data = None
        assert lib.cpq_ir_minimum_phase_batch(ptrs2, 2, 0, poisoned(), status) == K.CPQ_ERR_INVALID_ARG, broken
        assert "IR 1" in lib.cpq_last_error(None).decode()
        assert all(not o.data and o.n_channels == 0 and o.n_samples == 0 for o in outs)
    # a cap below one row's need: 16 n + 32 bytes on the small path; the message names the need
    assert lib.cpq_ir_minimum_phase_batch(ptrs, 2, 16 * 16 + 31, poisoned(), status) == K.CPQ_ERR_INVALID_ARG
    assert str(16 * 16 + 32) in lib.cpq_last_error(None).decode()
    assert all(not o.data and o.n_channels == 0 for o in outs)
    assert lib.cpq_ir_minimum_phase(None, outs) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_ir_minimum_phase(bufs, None) == K.CPQ_ERR_INVALID_ARG


def test_empty_batch_and_too_long_ir_need_no_device():
    lib = K.load()
    assert lib.cpq_ir_minimum_phase_batch(None, 0, 0, None, None) == K.CPQ_OK
    assert lib.cpq_ir_minimum_phase_last_kernel_ms() < 0.0
    assert amd.ir_minimum_phase_batch([]) == ([], [])
    long_ir = np.zeros((1, 2097153))
    long_ir[0, 0] = 1.0
    outs, status = amd.ir_minimum_phase_batch([long_ir, long_ir[:, :2097153]])
    assert outs == [None, None] and status == [K.CPQ_ERR_UNSUPPORTED, K.CPQ_ERR_UNSUPPORTED]
    assert lib.cpq_ir_minimum_phase_last_kernel_ms() < 0.0
    with pytest.raises(amd.CpqError) as e:
        amd.ir_minimum_phase(long_ir)
    assert e.value.status == K.CPQ_ERR_UNSUPPORTED
    assert K.CPQ_ERR_UNSUPPORTED == -5 and lib.cpq_abi_revision() == 1


def test_no_device_is_an_error_not_a_fallback():
    """a batch that needs the device: CPQ_ERR_NO_DEVICE with the reason where there is none (never a host result in its place);
    where there is one the same calls succeed"""
    lib = K.load()
    keep, bufs, ptrs = buffers([noise((1, 16), 1)])
    outs = (K.IrBuffer * 1)()
    status = (C.c_int32 * 1)()
    rc = lib.cpq_ir_minimum_phase_batch(ptrs, 1, 0, outs, status)
    assert rc in (K.CPQ_OK, K.CPQ_ERR_NO_DEVICE)
    if rc == K.CPQ_OK:
        assert outs[0].data and outs[0].n_samples == 16 and status[0] == K.CPQ_OK
        lib.cpq_ir_buffer_free(C.byref(outs[0]))
        return
    assert not outs[0].data and outs[0].n_samples == 0 and "no CPU fallback" in lib.cpq_last_error(None).decode()
    assert lib.cpq_ir_minimum_phase_last_kernel_ms() < 0.0
    for call in (lambda: amd.ir_minimum_phase_batch([noise((1, 64), 3), noise((2, 5000), 4)]),
                 lambda: amd.ir_minimum_phase(noise((2, 5000), 4)),
                 lambda: amd.ir_prepare_batch([(noise((1, 600), 5), 48000.0)], 48000.0, 0.01, phase_mode=K.CPQ_PHASE_MINIMUM)):
        with pytest.raises(amd.CpqError) as e:
            call()
        assert e.value.status == K.CPQ_ERR_NO_DEVICE
    x = np.zeros((1, 1 << 14))
    assert lib.cpq_diag_cfft(x.ctypes.data_as(K.c_double_p), 13, 1, 0, x.ctypes.data_as(K.c_double_p)) == K.CPQ_ERR_NO_DEVICE


def test_diag_cfft_refusals():
    lib = K.load()
    x = np.zeros(64)
    p = x.ctypes.data_as(K.c_double_p)
    for args in ((None, 3, 1, 0, p), (p, 3, 1, 0, None), (p, 0, 1, 0, p), (p, 24, 1, 0, p), (p, 3, 0, 0, p), (p, 23, 17, 0, p)):
        assert lib.cpq_diag_cfft(*args) == K.CPQ_ERR_INVALID_ARG


def same_prepared(a, b):
    return (a["ir"].shape == b["ir"].shape and np.array_equal(a["ir"].view(np.uint64), b["ir"].view(np.uint64))
            and a["scale"] == b["scale"] and a["ir_peak_latency"] == b["ir_peak_latency"] and a["sample_rate"] == b["sample_rate"])


def test_prepare_batch_as_is_equals_prepare_bit_for_bit():
    t = np.arange(3000)
    irs = [noise((1, 900), 11) * np.exp(-t[:900] / 150.0), noise((2, 3000), 12) * np.exp(-t / 400.0), noise((2, 50), 13),
           np.concatenate([noise((1, 700), 14), np.zeros((1, 300))], axis=1)]
    loud = noise((2, 64), 15) * 4.0
    quiet = noise((1, 64), 16) * 1e-3
    singles = [amd.ir_prepare(ir, 48000.0, 48000.0, 0.02) for ir in irs]
    batch = amd.ir_prepare_batch([(ir, 48000.0) for ir in irs], 48000.0, 0.02)
    assert len(batch) == len(irs) and all(same_prepared(a, b) for a, b in zip(batch, singles))
    currents, scales = [loud, None, quiet, quiet], [0.5, 1.0, 0.25, 2.0]
    singles = [amd.ir_prepare(ir, 48000.0, 48000.0, 0.02, current_ir=c, current_scale=s) for ir, c, s in zip(irs, currents, scales)]
    batch = amd.ir_prepare_batch([(ir, 48000.0) for ir in irs], 48000.0, 0.02, current_irs=currents, current_scales=scales)
    assert all(same_prepared(a, b) for a, b in zip(batch, singles))
    assert amd.ir_prepare_batch([], 48000.0, 0.02, phase_mode=K.CPQ_PHASE_MINIMUM) == []


def test_prepare_batch_refusals_are_all_or_nothing():
    lib = K.load()
    good = noise((1, 500), 21)
    with pytest.raises(amd.CpqError) as e:
        amd.ir_prepare_batch([(good, 48000.0), (good, 48000.0)], 48000.0, 0.02, phase_mode=K.CPQ_PHASE_MIXED)
    assert e.value.status == K.CPQ_ERR_UNSUPPORTED and "IR 0" in str(e.value)
    with pytest.raises(amd.CpqError) as e:
        amd.ir_prepare_batch([(good, 48000.0), (good, 44100.0)], 48000.0, 0.02)
    assert e.value.status == K.CPQ_ERR_UNSUPPORTED and "IR 1" in str(e.value)
    with pytest.raises(amd.CpqError) as e:
        amd.ir_prepare_batch([(good, 48000.0)], 48000.0, 0.02, phase_mode=7)
    assert e.value.status == K.CPQ_ERR_INVALID_ARG
    keep, bufs, ptrs = buffers([good, good])
    bufs[1].sample_rate = 44100.0
    outs = (K.IrPrepared * 2)()
    assert lib.cpq_ir_prepare_batch(ptrs, 2, 48000.0, 0.02, K.CPQ_PHASE_AS_IS, None, None, outs) == K.CPQ_ERR_UNSUPPORTED
    assert all(not o.ir.data and o.ir.n_samples == 0 for o in outs)
    assert lib.cpq_ir_prepare_batch(ptrs, -1, 48000.0, 0.02, 0, None, None, outs) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_ir_prepare_batch(None, 2, 48000.0, 0.02, 0, None, None, outs) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_ir_prepare_batch(ptrs, 2, 48000.0, 0.02, 0, None, None, None) == K.CPQ_ERR_INVALID_ARG
