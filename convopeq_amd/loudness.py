"""ProgrammeLoudness -- ctypes wrapper of cpq_loudness (include/convopeq_mi355x.h): gated programme loudness (EBU R 128) of
n_streams stereo programmes at once, on the device (gfx950 kernels; CpqError(CPQ_ERR_NO_DEVICE) without one, there is no host
object).  Rows are planar float64, [2 n_streams, n]: L0 R0 L1 R1 ..., as BatchedEngine delivers them.  process() takes host numpy
rows and is synchronous; process_device() takes a CUDA tensor and is asynchronous on the object's stream (set_stream).
finish() may be called at any time and repeatedly: the programmes go on."""
import ctypes as C

import numpy as np

from . import _capi as K
from .engine import CpqError

FIELDS = tuple(name for name, _ in K.LoudnessResult._fields_)


def _as_dict(r):
    return {name: getattr(r, name) for name in FIELDS}


def loudness_finish_host(hops, sample_rate):
    """the figures of one stream from its hop sums, on the host, in the device's order of operations"""
    hops = np.ascontiguousarray(hops, dtype=np.float64)
    r = K.LoudnessResult()
    rc = K.load().cpq_loudness_finish_host(hops.ctypes.data_as(K.c_double_p), hops.size, float(sample_rate), C.byref(r))
    if rc != K.CPQ_OK:
        raise CpqError(rc, K.load().cpq_loudness_last_error(None).decode())
    return _as_dict(r)


class ProgrammeLoudness:
    def __init__(self, n_streams, sample_rate, max_seconds):
        self._h = None
        self._lib = K.load()
        desc = K.LoudnessDesc(n_streams, float(sample_rate), float(max_seconds), 0)
        h = C.c_void_p()
        rc = self._lib.cpq_loudness_create(C.byref(desc), C.byref(h))
        if rc != K.CPQ_OK:
            raise CpqError(rc, self._lib.cpq_loudness_last_error(None).decode())
        self._h, self.n_streams, self.sample_rate = h, n_streams, float(sample_rate)
        self._stream = None

    def _check(self, rc):
        if rc != K.CPQ_OK:
            raise CpqError(rc, self._lib.cpq_loudness_last_error(self._h).decode())

    def close(self):
        if self._h is not None:
            self._lib.cpq_loudness_destroy(self._h)
            self._h = None

    __del__ = close

    def reset(self):
        self._check(self._lib.cpq_loudness_reset(self._h))

    def set_stream(self, stream):
        """the torch.cuda.Stream (None: the null stream) later calls enqueue on; the stream used so far is synchronised first"""
        self._check(self._lib.cpq_loudness_set_stream(self._h, C.c_void_p(stream.cuda_stream if stream is not None else None)))
        self._stream = stream           # kept alive as long as the object enqueues on it

    def process(self, rows):
        """rows [2 n_streams, n] float64 on the host: n more samples of every programme"""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert rows.ndim == 2 and rows.shape[0] == 2 * self.n_streams
        self._check(self._lib.cpq_loudness_process(self._h, rows.ctypes.data, rows.shape[1], rows.shape[1]))

    def process_device(self, t):
        """t: CUDA float64 tensor [2 n_streams, n] of any row stride (elements of a row adjacent).  Asynchronous on the object's
        stream: t must stay as it is until that stream has reached the call."""
        import torch
        assert t.is_cuda and t.dtype == torch.float64 and t.dim() == 2 and t.shape[0] == 2 * self.n_streams and t.stride(1) == 1
        self._check(self._lib.cpq_loudness_process_device(self._h, C.c_void_p(t.data_ptr()), t.stride(0), t.shape[1]))

    def finish(self):
        """one dict per stream: integrated, range, momentary_max, short_term_max, relative_gate (LUFS / LU; -inf where a set is
        empty), n_hops and the counts n_blocks, n_abs, n_rel, n_short_kept"""
        res = (K.LoudnessResult * self.n_streams)()
        self._check(self._lib.cpq_loudness_finish(self._h, res))
        return [_as_dict(r) for r in res]

    def read_hops(self, stream):
        """the complete hop sums E[h] of one stream so far (diagnostic)"""
        n = C.c_int64()
        self._check(self._lib.cpq_loudness_read_hops(self._h, stream, None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1))
        self._check(self._lib.cpq_loudness_read_hops(self._h, stream, out.ctypes.data_as(K.c_double_p), n.value, C.byref(n)))
        return out[:n.value].copy()

    def gain(self, result, target_lufs=-23.0):
        """the linear gain that brings a finish() entry to target_lufs; CpqError(CPQ_ERR_NOT_READY) where nothing passed the gates"""
        r = K.LoudnessResult(**result)
        g = C.c_double()
        rc = self._lib.cpq_loudness_gain(C.byref(r), float(target_lufs), C.byref(g))
        if rc != K.CPQ_OK:
            raise CpqError(rc, self._lib.cpq_loudness_last_error(None).decode())
        return g.value
