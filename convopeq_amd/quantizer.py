"""Quantizer -- ctypes wrapper of cpq_quantizer (include/convopeq_mi355x.h): the stream's gain, a noise shaper and the PCM pack of
n_streams stereo programmes in one pass, the last step of a delivery after ProgrammeLoudness and TruePeakLimiter.  Rows are planar
float64, [2 n_streams, n]: L0 R0 L1 R1 ..., as TruePeakLimiter delivers them.  The packed side is bytes: CPQ_PCM_PLANAR,
[2 n_streams] rows of n samples; CPQ_PCM_INTERLEAVED, [n_streams] rows of n stereo frames; rows `pitch` bytes apart.
host=True is the object that computes on the host (no GPU), device=True the one that computes on the device (one gfx950 kernel per
call; CpqError(CPQ_ERR_NO_DEVICE) without one).  Their bytes are equal, and equal for every split of a programme into calls.
Neither flag raises CpqError(CPQ_ERR_UNSUPPORTED): there is no quiet fall-back either way.  process() takes and returns host
numpy arrays on both objects; process_device() works on CUDA tensors and is asynchronous on the object's stream (set_stream)."""
import ctypes as C

import numpy as np

from . import _capi as K
from ._handle import StreamHandle
from .engine import CpqError

_BYTES = {K.CPQ_PCM_S16: 2, K.CPQ_PCM_S24: 3, K.CPQ_PCM_S32: 4}


class Quantizer(StreamHandle):
    _PREFIX = "cpq_quantizer"

    def __init__(self, n_streams, sample_rate, shaper, bit_depth, container=K.CPQ_PCM_S16, host=False, device=False):
        if host and device:
            raise ValueError("host and device exclude each other")
        flags = K.CPQ_QUANT_HOST if host else K.CPQ_QUANT_DEVICE if device else 0
        self._open(n_streams, float(sample_rate), int(shaper), int(bit_depth), int(container), flags)
        self.n_streams, self.sample_rate, self.host, self.device = n_streams, float(sample_rate), bool(host), bool(device)
        self.shaper, self.bit_depth, self.container = int(shaper), int(bit_depth), int(container)
        self.bytes_per_sample = _BYTES[self.container]

    @property
    def last_kernel_ms(self):
        """device time of the launch of the last call of a device object (waits for it); -1 otherwise"""
        return self._lib.cpq_quantizer_last_kernel_ms(self._h)

    def packed_shape(self, layout, n):
        """(rows, width in bytes) of the packed side of a call of n samples"""
        if layout == K.CPQ_PCM_INTERLEAVED:
            return self.n_streams, 2 * n * self.bytes_per_sample
        return 2 * self.n_streams, n * self.bytes_per_sample

    def reset(self):
        """as new: errors cleared, generators reseeded; gains and adaptive coefficients stay"""
        self._check(self._lib.cpq_quantizer_reset(self._h))

    def set_gains(self, gains):
        """the gain of every stream (ProgrammeLoudness.gain), only at the start of a programme: CpqError(CPQ_ERR_NOT_READY) later"""
        g = np.ascontiguousarray(gains, dtype=np.float64)
        assert g.shape == (self.n_streams,)
        self._check(self._lib.cpq_quantizer_set_gains(self._h, g.ctypes.data_as(K.c_double_p)))

    def set_adaptive_coeffs(self, stream, k):
        """the set a ShaperLearner publishes, for one stream or CPQ_ALL_STREAMS: clamped, those streams' states cleared"""
        k = np.ascontiguousarray(k, dtype=np.float64)
        assert k.ndim == 1
        self._check(self._lib.cpq_quantizer_set_adaptive_coeffs(self._h, int(stream), k.ctypes.data_as(K.c_double_p), k.size))

    def adaptive_coeffs(self, stream):
        k = np.empty(9)
        rc = self._lib.cpq_quantizer_get_adaptive_coeffs(self._h, int(stream), k.ctypes.data_as(K.c_double_p))
        if rc != K.CPQ_OK:
            raise CpqError(rc, "cpq_quantizer_get_adaptive_coeffs")
        return k

    def process(self, rows, layout=K.CPQ_PCM_PLANAR, out=None):
        """rows [2 n_streams, n] float64 on the host -> uint8 [packed rows, width].  out: a uint8 array [packed rows, pitch] whose
        rows are written in place (pitch >= width; the bytes beyond the width stay as they are); its first `width` columns are
        returned"""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert rows.ndim == 2 and rows.shape[0] == 2 * self.n_streams
        n = rows.shape[1]
        r, width = self.packed_shape(layout, n)
        if out is None:
            out = np.zeros((r, width), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.ndim == 2 and out.shape[0] == r and out.strides[1] == 1
        self._check(self._lib.cpq_quantizer_process(self._h, rows.ctypes.data, n, out.ctypes.data, out.strides[0], int(layout), n))
        return out[:, :width]

    def process_device(self, t_in, layout=K.CPQ_PCM_PLANAR, t_out=None):
        """t_in: CUDA float64 tensor [2 n_streams, n] of any row stride (elements of a row adjacent) -> a CUDA uint8 tensor
        [packed rows, width] (t_out: [packed rows, pitch] of any row stride >= width; its first `width` columns are returned).
        Asynchronous on the object's stream: t_in must stay as it is until that stream has reached the call."""
        if not self.device:
            raise CpqError(K.CPQ_ERR_INVALID_ARG, "process_device on an object that is not a device object")
        import torch
        assert t_in.is_cuda and t_in.dtype == torch.float64 and t_in.dim() == 2 and t_in.shape[0] == 2 * self.n_streams and t_in.stride(1) == 1
        n = t_in.shape[1]
        r, width = self.packed_shape(layout, n)
        if t_out is None:
            t_out = torch.empty((r, width), dtype=torch.uint8, device=t_in.device)
        assert t_out.is_cuda and t_out.dtype == torch.uint8 and t_out.dim() == 2 and t_out.shape[0] == r and t_out.stride(1) == 1
        self._check(self._lib.cpq_quantizer_process_device(self._h, C.c_void_p(t_in.data_ptr()), t_in.stride(0), C.c_void_p(t_out.data_ptr()),
                                                           t_out.stride(0), int(layout), n))
        return t_out[:, :width]
