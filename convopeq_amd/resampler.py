"""StreamResampler -- ctypes wrapper of cpq_src (include/convopeq_mi355x.h): streaming sample-rate conversion of n_channels planar
float64 rows, call by call, the history kept by the object.  Host numpy arrays in and out.  Only the object that computes on the
host is built (host=True, no GPU); host=False asks for the device object and raises CpqError(CPQ_ERR_UNSUPPORTED): there is no
quiet fall-back."""
import ctypes as C

import numpy as np

from . import _capi as K
from .engine import CpqError


class StreamResampler:
    def __init__(self, n_channels, in_rate, out_rate, max_in, host=False, phase=K.CPQ_RESAMPLE_LINEAR_PHASE, start_period=0):
        self._lib = K.load()
        self._h = None
        desc = K.SrcDesc(n_channels, float(in_rate), float(out_rate), max_in, phase, K.CPQ_SRC_HOST if host else 0, start_period)
        h = C.c_void_p()
        rc = self._lib.cpq_src_create(C.byref(desc), C.byref(h))
        if rc != K.CPQ_OK:
            raise CpqError(rc, self._lib.cpq_src_last_error(None).decode())
        self._h, self.n_channels, self.max_in, self.host = h, n_channels, max_in, bool(host)

    def _check(self, rc):
        if rc != K.CPQ_OK:
            raise CpqError(rc, self._lib.cpq_src_last_error(self._h).decode())

    def close(self):
        if self._h is not None:
            self._lib.cpq_src_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def latency(self):
        """input samples between a sample and the output it is the centre of: T / 2"""
        return self._lib.cpq_src_latency(self._h)

    @property
    def max_out(self):
        return self._lib.cpq_src_max_out(self._h)

    def out_count(self, n_in, flush=False):
        n = self._lib.cpq_src_out_count(self._h, n_in, int(bool(flush)))
        if n < 0:
            raise CpqError(n, "cpq_src_out_count")
        return n

    def reset(self):
        self._check(self._lib.cpq_src_reset(self._h))

    def process(self, rows, flush=False):
        """rows [n_channels, n] float64 on the host -> the samples this call emits, [n_channels, n_out]"""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert rows.ndim == 2 and rows.shape[0] == self.n_channels
        n_in = rows.shape[1]
        cap = max(self.out_count(n_in, flush), 1)
        out = np.empty((self.n_channels, cap))
        n = C.c_int32()
        self._check(self._lib.cpq_src_process(self._h, rows.ctypes.data, max(n_in, 1), n_in, out.ctypes.data, cap, cap, int(bool(flush)), C.byref(n)))
        return out[:, :n.value].copy()
