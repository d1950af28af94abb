"""Callers of cpq_diag_fdl_mac and cpq_diag_partition_fft_split and the tables of argument sets they must refuse, shared by
tests/test_gpu_fdl_mac.py and tests/test_gpu_fft_p4_frames.py (on the device) and tests/test_host_and_abi_cpu.py (the refusals
come before the device is looked for, so they are checked without one).

Every output array is filled with -7 (the variant with -99) here before the call: a refused call leaves all of that as it is.
The arrays are sized for the good arguments or the overridden ones, whichever is larger: a refusal must not depend on reading
them, and a call that is wrongly accepted stays inside them."""
import ctypes as C

import numpy as np

from fft_layout import dp

INVALID_ARG, NO_DEVICE = -1, -2

# ------------------------------------------------------------------------------------------------ cpq_diag_fdl_mac
MAC_GOOD = dict(P=64, n_ch=2, K=5, T=3, tile=4, head=1, ring=128, n_slots=2, h_rows=48, slots=(0, 1))
MAC_BAD = {
    "ring not a power of two": dict(ring=96),
    "ring below the engines' rule": dict(ring=64),                  # nextPow2(32 + 32 + 3) = 128
    "ring zero": dict(ring=0),
    "h_rows below alignUp(K, 32) + 16": dict(h_rows=47),
    "ir_slot negative": dict(slots=(0, -1)),
    "ir_slot = n_ir_slots": dict(slots=(2, 0)),
    "head negative": dict(head=-1),
    "head = ring_slots": dict(head=128),
    "P below 64": dict(P=32),
    "P above 4096": dict(P=8192),
    "P not a power of two": dict(P=96),
    "K zero": dict(K=0),
    "T zero": dict(T=0),
    "no channels": dict(n_ch=0),
    "no IR slots": dict(n_slots=0),
    "unknown tile": dict(tile=5),
}
MAC_POINTERS = ("x", "h", "ir_slot", "y", "variant_used")


def mac_buffers(a=MAC_GOOD):
    """(X, H, Y, used) of ones, -7 and -99 for the argument set a"""
    P, n_ch, ring = max(a["P"], 64), max(a["n_ch"], 2), max(a["ring"], 128)
    X = np.ones((n_ch, ring, P, 2))
    H = np.ones((max(a["n_slots"], 2), max(a["h_rows"], 48), P, 2))
    Y = np.full((n_ch, max(a["T"], 3), P, 2), -7.0)
    return X, H, Y, C.c_int32(-99)


def mac_call(lib, v, X, H, Y, used, null=None):
    """cpq_diag_fdl_mac with the argument set v on the arrays given; null: the one of MAC_POINTERS that is passed as NULL"""
    slots = np.array(v["slots"], dtype=np.int32)
    ptr = dict(x=dp(X), h=dp(H), ir_slot=slots.ctypes.data_as(C.POINTER(C.c_int32)), y=dp(Y), variant_used=C.byref(used))
    if null is not None:
        ptr[null] = None
    return lib.cpq_diag_fdl_mac(v["P"], v["n_ch"], v["K"], v["T"], v["tile"], v["head"], v["ring"], v["n_slots"], v["h_rows"], 0,
                                *(ptr[k] for k in MAC_POINTERS))


def mac_untouched(Y, used):
    return used.value == -99 and bool((Y == -7.0).all())


# ------------------------------------------------------------------------------------ cpq_diag_partition_fft_split
FFT_GOOD = dict(P=4096, n_ch=3, T=5, split=0)
FFT_VALID = {
    "split 0": dict(),
    "split negative": dict(split=-3),
    "split = T": dict(split=5),
    "split = T + 1 at P = 512 (ignored)": dict(P=512, split=6),
}
FFT_BAD = {
    "P below 64": dict(P=32),
    "P not a power of two": dict(P=96),
    "P above 131072": dict(P=262144, n_ch=1, T=1),
    "no channels": dict(n_ch=0),
    "T zero": dict(T=0),
    "split = T + 1": dict(split=6),
}
FFT_POINTERS = ("in", "spectra", "out")


def fft_split_call(lib, v, x=None, null=None):
    """cpq_diag_partition_fft_split with the argument set v on x [n_ch][T][P] (ones when not given): (status, spectra, out)"""
    shape = (max(v["n_ch"], 1), max(v["T"], 1), v["P"])
    x = np.ones(shape) if x is None else np.ascontiguousarray(x, dtype=np.float64)
    assert x.shape == shape
    spec, out = np.full(shape + (2,), -7.0), np.full(shape, -7.0)
    ptr = {"in": dp(x), "spectra": dp(spec), "out": dp(out)}
    if null is not None:
        ptr[null] = None
    return lib.cpq_diag_partition_fft_split(v["P"], v["n_ch"], v["T"], v["split"], *(ptr[k] for k in FFT_POINTERS)), spec, out


def fft_untouched(spec, out):
    return bool((spec == -7.0).all() and (out == -7.0).all())


# ----------------------------------------------------------------------------------------------------------- walks
def walk_refusals(lib):
    """every refusal rule once: [(entry, rule, status, outputs untouched)]"""
    res = []
    for rule, override in MAC_BAD.items():
        a = dict(MAC_GOOD, **override)
        X, H, Y, used = mac_buffers(a)
        res.append(("fdl_mac", rule, mac_call(lib, a, X, H, Y, used), mac_untouched(Y, used)))
    for name in MAC_POINTERS:
        X, H, Y, used = mac_buffers()
        res.append(("fdl_mac", name + " null", mac_call(lib, MAC_GOOD, X, H, Y, used, null=name), mac_untouched(Y, used)))
    for rule, override in FFT_BAD.items():
        rc, spec, out = fft_split_call(lib, dict(FFT_GOOD, **override))
        res.append(("partition_fft_split", rule, rc, fft_untouched(spec, out)))
    for name in FFT_POINTERS:
        rc, spec, out = fft_split_call(lib, FFT_GOOD, null=name)
        res.append(("partition_fft_split", name + " null", rc, fft_untouched(spec, out)))
    return res


def valid_calls(lib):
    """the valid argument sets themselves: [(entry, rule, status, outputs untouched)]"""
    X, H, Y, used = mac_buffers()
    res = [("fdl_mac", "good", mac_call(lib, MAC_GOOD, X, H, Y, used), mac_untouched(Y, used))]
    for rule, override in FFT_VALID.items():
        rc, spec, out = fft_split_call(lib, dict(FFT_GOOD, **override))
        res.append(("partition_fft_split", rule, rc, fft_untouched(spec, out)))
    return res
