"""TruePeakLimiter -- ctypes wrapper of cpq_limiter (include/convopeq_mi355x.h): a look-ahead true-peak limiter over n_streams
stereo programmes at once.  Rows are planar float64, [2 n_streams, n]: L0 R0 L1 R1 ..., as BatchedEngine delivers them and
ProgrammeLoudness meters them.  host=True is the object that computes on the host (no GPU), device=True the one that computes on
the device (gfx950 kernels; CpqError(CPQ_ERR_NO_DEVICE) without one).  Their outputs are equal bit for bit, and equal for every
split of a programme into calls.  Neither flag raises CpqError(CPQ_ERR_UNSUPPORTED): there is no quiet fall-back either way.
process() and flush() take and return host numpy arrays on both objects; process_device() and flush_device() work on CUDA tensors
and are asynchronous on the object's stream (set_stream).  A call of n samples returns n samples, delayed by `latency`; the first
`latency` samples of a programme are zeros and flush() returns the last `latency`."""
import ctypes as C

import numpy as np

from . import _capi as K
from ._handle import StreamHandle
from .engine import CpqError


def limiter_default_window(sample_rate):
    """round(0.0015 * sample_rate) clamped to 8 ... 1024: the window window=0 takes"""
    w = K.load().cpq_limiter_default_window(float(sample_rate))
    if w < 0:
        raise CpqError(w, "cpq_limiter_default_window")
    return w


class TruePeakLimiter(StreamHandle):
    _PREFIX = "cpq_limiter"

    def __init__(self, n_streams, sample_rate, ceiling_dbtp=-1.0, window=0, host=False, device=False):
        if host and device:
            raise ValueError("host and device exclude each other")
        flags = K.CPQ_LIM_HOST if host else K.CPQ_LIM_DEVICE if device else 0
        self._open(n_streams, float(sample_rate), float(ceiling_dbtp), int(window), flags)
        self.n_streams, self.sample_rate, self.host, self.device = n_streams, float(sample_rate), bool(host), bool(device)
        self.ceiling = 10.0 ** (float(ceiling_dbtp) / 20.0)

    @property
    def latency(self):
        """samples between a sample and its output: window + 11"""
        return self._lib.cpq_limiter_latency(self._h)

    @property
    def window(self):
        return self._lib.cpq_limiter_window(self._h)

    @property
    def last_kernel_ms(self):
        """device time of the launches of the last call of a device object (waits for them); -1 otherwise"""
        return self._lib.cpq_limiter_last_kernel_ms(self._h)

    def reset(self):
        self._check(self._lib.cpq_limiter_reset(self._h))

    def set_gains(self, gains):
        """the pre-gain of every stream (ProgrammeLoudness.gain), only at the start of a programme: CpqError(CPQ_ERR_NOT_READY) later"""
        g = np.ascontiguousarray(gains, dtype=np.float64)
        assert g.shape == (self.n_streams,)
        self._check(self._lib.cpq_limiter_set_gains(self._h, g.ctypes.data_as(K.c_double_p)))

    def process(self, rows):
        """rows [2 n_streams, n] float64 on the host -> the n samples per row this call emits"""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert rows.ndim == 2 and rows.shape[0] == 2 * self.n_streams
        out = np.empty_like(rows)
        self._check(self._lib.cpq_limiter_process(self._h, rows.ctypes.data, rows.shape[1], out.ctypes.data, rows.shape[1], rows.shape[1]))
        return out

    def flush(self):
        """the last `latency` samples per row; the object is then at the start of a new programme"""
        out = np.empty((2 * self.n_streams, self.latency))
        self._check(self._lib.cpq_limiter_flush(self._h, out.ctypes.data, out.shape[1]))
        return out

    def process_device(self, t_in, t_out=None):
        """t_in: CUDA float64 tensor [2 n_streams, n] of any row stride (elements of a row adjacent) -> t_out (None: a new tensor;
        t_in itself: in place, which costs a device copy).  Asynchronous on the object's stream: t_in must stay as it is until
        that stream has reached the call."""
        if not self.device:
            raise CpqError(K.CPQ_ERR_INVALID_ARG, "process_device on an object that is not a device object")
        import torch
        if t_out is None:
            t_out = torch.empty_like(t_in, memory_format=torch.contiguous_format)
        for t in (t_in, t_out):
            assert t.is_cuda and t.dtype == torch.float64 and t.dim() == 2 and t.shape[0] == 2 * self.n_streams and t.stride(1) == 1
        assert t_in.shape == t_out.shape
        self._check(self._lib.cpq_limiter_process_device(self._h, C.c_void_p(t_in.data_ptr()), t_in.stride(0), C.c_void_p(t_out.data_ptr()),
                                                         t_out.stride(0), t_in.shape[1]))
        return t_out

    def flush_device(self, t_out=None, device=None):
        """the last `latency` samples per row as a CUDA tensor [2 n_streams, latency] (t_out: at least that wide; its first
        `latency` columns are returned)"""
        if not self.device:
            raise CpqError(K.CPQ_ERR_INVALID_ARG, "flush_device on an object that is not a device object")
        import torch
        if t_out is None:
            t_out = torch.empty((2 * self.n_streams, (self.latency + 1) & ~1), dtype=torch.float64, device=device or "cuda")
        assert t_out.is_cuda and t_out.dtype == torch.float64 and t_out.dim() == 2 and t_out.shape[0] == 2 * self.n_streams and t_out.stride(1) == 1
        assert t_out.shape[1] >= self.latency
        self._check(self._lib.cpq_limiter_flush_device(self._h, C.c_void_p(t_out.data_ptr()), t_out.stride(0)))
        return t_out[:, :self.latency]

    def telemetry(self):
        """one dict per stream: min_gain (the smallest envelope value, 1.0 where nothing was limited) and limited_samples, of the
        programme in progress or the one a flush just ended.  Synchronises the object's stream."""
        res = (K.LimiterTelemetry * self.n_streams)()
        self._check(self._lib.cpq_limiter_read_telemetry(self._h, res))
        return [{"min_gain": r.min_gain, "limited_samples": r.limited_samples} for r in res]
