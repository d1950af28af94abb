"""StreamResampler -- ctypes wrapper of cpq_src (include/convopeq_mi355x.h): streaming sample-rate conversion of n_channels planar
float64 rows, call by call, the history kept by the object.  host=True is the object that computes on the host (no GPU),
device=True the one that computes on the device (gfx950 kernels; CpqError(CPQ_ERR_NO_DEVICE) without one).  Their outputs are
equal bit for bit.  Neither flag raises CpqError(CPQ_ERR_UNSUPPORTED): the caller says where the rows are computed, and there is
no quiet fall-back either way.  process() takes and returns host numpy arrays on both objects; process_device() takes and returns
CUDA tensors and is asynchronous on the object's stream (set_stream)."""
import ctypes as C

import numpy as np

from . import _capi as K
from .engine import CpqError


class StreamResampler:
    def __init__(self, n_channels, in_rate, out_rate, max_in, host=False, phase=K.CPQ_RESAMPLE_LINEAR_PHASE, start_period=0, device=False):
        self._h = None
        if host and device:
            raise ValueError("host and device exclude each other")
        self._lib = K.load()
        flags = K.CPQ_SRC_HOST if host else K.CPQ_SRC_DEVICE if device else 0
        desc = K.SrcDesc(n_channels, float(in_rate), float(out_rate), max_in, phase, flags, start_period)
        h = C.c_void_p()
        rc = self._lib.cpq_src_create(C.byref(desc), C.byref(h))
        if rc != K.CPQ_OK:
            raise CpqError(rc, self._lib.cpq_src_last_error(None).decode())
        self._h, self.n_channels, self.max_in, self.host, self.device = h, n_channels, max_in, bool(host), bool(device)
        self._stream = None

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

    @property
    def last_kernel_ms(self):
        """device time of the launches of the last process() on a device object; -1 otherwise"""
        return self._lib.cpq_src_last_kernel_ms(self._h)

    def out_count(self, n_in, flush=False):
        n = self._lib.cpq_src_out_count(self._h, n_in, int(bool(flush)))
        if n < 0:
            raise CpqError(n, "cpq_src_out_count")
        return n

    def reset(self):
        self._check(self._lib.cpq_src_reset(self._h))

    def set_stream(self, stream):
        """the torch.cuda.Stream (None: the null stream) later calls enqueue on; the stream used so far is synchronised first"""
        self._check(self._lib.cpq_src_set_stream(self._h, C.c_void_p(stream.cuda_stream if stream is not None else None)))
        self._stream = stream           # kept alive as long as the object enqueues on it

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

    def process_device(self, t_in, flush=False, out=None):
        """t_in: CUDA float64 tensor [n_channels, n] of any row stride (elements of a row adjacent) -> a CUDA tensor
        [n_channels, n_out]: `out[:, :n_out]` where out is given (any row stride, at least n_out columns), else a new one.
        Asynchronous on the object's stream: t_in must stay as it is until that stream has reached the call."""
        if not self.device:
            raise CpqError(K.CPQ_ERR_INVALID_ARG, "process_device on an object that is not a device object")
        import torch
        assert t_in.is_cuda and t_in.dtype == torch.float64 and t_in.dim() == 2 and t_in.shape[0] == self.n_channels
        n_in = t_in.shape[1]
        assert n_in == 0 or t_in.stride(1) == 1
        count = self.out_count(n_in, flush)
        if out is None:
            out = torch.empty((self.n_channels, max(count, 1)), dtype=torch.float64, device=t_in.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.dim() == 2 and out.shape[0] == self.n_channels and out.stride(1) == 1
        in_stride = t_in.stride(0) if self.n_channels > 1 and n_in > 0 else max(n_in, 1)
        out_stride = out.stride(0) if self.n_channels > 1 else out.shape[1]
        n = C.c_int32()
        self._check(self._lib.cpq_src_process_device(self._h, C.c_void_p(t_in.data_ptr() if n_in else None), in_stride, n_in,
                                                     C.c_void_p(out.data_ptr()), out_stride, out.shape[1], int(bool(flush)), C.byref(n)))
        return out[:, :n.value]
