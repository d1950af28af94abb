"""ProgrammeLoudness -- ctypes wrapper of cpq_loudness (include/convopeq_mi355x.h): gated programme loudness (EBU R 128) of
n_streams stereo programmes at once, on the device (gfx950 kernels; CpqError(CPQ_ERR_NO_DEVICE) without one, there is no host
object).  Rows are planar float64, [2 n_streams, n]: L0 R0 L1 R1 ..., as BatchedEngine delivers them.  process() takes host numpy
rows and is synchronous; process_device() takes a CUDA tensor and is asynchronous on the object's stream (set_stream).
finish() may be called at any time and repeatedly: the programmes go on."""
import ctypes as C
import math

import numpy as np

from . import _capi as K
from ._handle import StreamHandle
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


def _dbtp(v):
    return 20.0 * math.log10(v) if v > 0.0 else -math.inf


def loudness_peaks_host(rows, sample_rate):
    """(true_peak, sample_peak), linear, per row of rows [n_rows, n]: each row a programme from its start, on the host, to the
    bit what the device reads (BS.1770-4 Annex 2; csrc/prog_plan.hpp)"""
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float64)
    tp, sp = np.empty(rows.shape[0]), np.empty(rows.shape[0])
    rc = K.load().cpq_loudness_peaks_host(rows.ctypes.data_as(K.c_double_p), rows.shape[1], rows.shape[0], rows.shape[1], float(sample_rate),
                                          tp.ctypes.data_as(K.c_double_p), sp.ctypes.data_as(K.c_double_p))
    if rc != K.CPQ_OK:
        raise CpqError(rc, K.load().cpq_loudness_last_error(None).decode())
    return tp, sp


class ProgrammeLoudness(StreamHandle):
    _PREFIX = "cpq_loudness"

    def __init__(self, n_streams, sample_rate, max_seconds, true_peak=False):
        desc = K.LoudnessDesc(n_streams, float(sample_rate), float(max_seconds), 0)
        self._open(C.byref(desc))
        self.n_streams, self.sample_rate = n_streams, float(sample_rate)
        if true_peak:
            self.set_true_peak(True)

    def reset(self):
        self._check(self._lib.cpq_loudness_reset(self._h))

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

    def set_true_peak(self, on=True):
        """true peak per programme (BS.1770-4 Annex 2) beside the loudness; only at the start of a programme (after create or
        reset), CpqError(CPQ_ERR_NOT_READY) later"""
        self._check(self._lib.cpq_loudness_set_true_peak(self._h, 1 if on else 0))

    def peaks(self):
        """one dict per stream: true_peak and sample_peak, linear (L, R), their dBTP / dBFS values true_peak_db and
        sample_peak_db (-inf for 0), and max_dbtp, the largest of the four in dB"""
        res = (K.LoudnessPeaks * self.n_streams)()
        self._check(self._lib.cpq_loudness_read_peaks(self._h, res))
        out = []
        for r in res:
            tp, sp = tuple(r.true_peak), tuple(r.sample_peak)
            out.append({"true_peak": tp, "sample_peak": sp, "true_peak_db": tuple(_dbtp(v) for v in tp),
                        "sample_peak_db": tuple(_dbtp(v) for v in sp), "max_dbtp": _dbtp(max(tp + sp))})
        return out

    def gain_limited(self, result, peaks, target_lufs=-23.0, max_dbtp=-1.0):
        """(gain, limited): the smaller of the gain to target_lufs and the gain that brings the largest of the stream's peaks to
        max_dbtp; limited says the ceiling won.  result: a finish() entry, peaks: a peaks() entry"""
        r = K.LoudnessResult(**result)
        pk = K.LoudnessPeaks((C.c_double * 2)(*peaks["true_peak"]), (C.c_double * 2)(*peaks["sample_peak"]))
        g, lim = C.c_double(), C.c_int32()
        rc = self._lib.cpq_loudness_gain_limited(C.byref(r), C.byref(pk), float(target_lufs), float(max_dbtp), C.byref(g), C.byref(lim))
        if rc != K.CPQ_OK:
            raise CpqError(rc, self._lib.cpq_loudness_last_error(None).decode())
        return g.value, bool(lim.value)

    def apply_device(self, gains, t_in, t_out=None):
        """t_out = t_in * gains[stream] on CUDA float64 tensors [2 n_streams, n] (t_out None: in place); asynchronous on the
        object's stream.  The programme is not touched."""
        import torch
        t_out = t_in if t_out is None else t_out
        for t in (t_in, t_out):
            assert t.is_cuda and t.dtype == torch.float64 and t.dim() == 2 and t.shape[0] == 2 * self.n_streams and t.stride(1) == 1
        assert t_in.shape == t_out.shape
        g = np.ascontiguousarray(gains, dtype=np.float64)
        assert g.shape == (self.n_streams,)
        self._check(self._lib.cpq_loudness_apply_device(self._h, g.ctypes.data_as(K.c_double_p), C.c_void_p(t_in.data_ptr()), t_in.stride(0),
                                                        C.c_void_p(t_out.data_ptr()), t_out.stride(0), t_in.shape[1]))

    def normalise_device(self, t, target_lufs=-23.0, max_dbtp=-1.0):
        """finish, peaks, gains and apply, in place on t, the rows this object has metered (true peak switched on).  Returns
        (gains, limited) per stream; a programme of which nothing passed the gates keeps its level: gain 1, not limited."""
        res, pks = self.finish(), self.peaks()
        gains, limited = np.ones(self.n_streams), [False] * self.n_streams
        for s in range(self.n_streams):
            if math.isfinite(res[s]["integrated"]):
                gains[s], limited[s] = self.gain_limited(res[s], pks[s], target_lufs, max_dbtp)
        self.apply_device(gains, t)
        return gains, limited
