"""What the tests of the partition FFT kernels share (test_gpu_fft.py, test_gpu_fft_p4_frames.py,
test_gpu_fft_variants.py): the storage order of a packed spectrum and the ctypes pointers of numpy arrays."""
import ctypes as C

import numpy as np


def bins(P):
    """storage element -> bin of the packed spectrum (element 0 = (DC, Nyquist))"""
    e = np.arange(P)
    if P <= 2048:
        return e
    m1 = P // 512
    return (e // 512) + m1 * (e % 512)


def dp(a):
    """double* of a C-contiguous float64 array"""
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_double))


def ip(a):
    """int64_t* of a C-contiguous int64 array"""
    assert a.dtype == np.int64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_int64))
