"""Host-side harness over the C ABI (tests / bench plumbing).

`BatchedEngine` mirrors the reference's processor surface for the hot path, batched over S stereo streams:
  prepare_to_play(sample_rate, max_block)   <- ConvolverProcessor/EQProcessor::prepareToPlay
  set_impulse(stream, ir_l, ir_r, ...)      <- StereoConvolver::init -> MKLNonUniformConvolver::SetImpulse
  set_eq_params(stream, params)             <- EQProcessor::createCoeffCache + process(block, params, cache)
  process(...) / conv_process / eq_process  <- ConvolverProcessor::process / EQProcessor::process
All numerical work happens in libconvopeq_mi355x.so on the GPU; numpy is only the host buffer type.
"""
import ctypes as C
import os

import numpy as np

from . import _capi as K


class CpqError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"cpq status {status} ({K.load().cpq_status_string(status).decode()}): {msg}")
        self.status = status


def _dp(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(K.c_double_p)


def nuc_plan(ir_len, block, direct=False, spec=None):
    p = K.NucPlan()
    rc = K.load().cpq_nuc_plan_compute(ir_len, block, int(direct), C.byref(spec) if spec is not None else None,
                                       C.byref(p))
    if rc != 0:
        raise CpqError(rc, "cpq_nuc_plan_compute")
    return p


def nuc_heff(ir, block, scale=1.0, spec=None):
    ir = np.ascontiguousarray(ir, dtype=np.float64)
    sp = C.byref(spec) if spec is not None else None
    n = K.load().cpq_nuc_heff(_dp(ir), len(ir), block, scale, sp, None, 0)
    if n < 0:
        raise CpqError(n, "cpq_nuc_heff")
    out = np.zeros(n, dtype=np.float64)
    K.load().cpq_nuc_heff(_dp(ir), len(ir), block, scale, sp, _dp(out), n)
    return out


def design_svf(btype, freq, gain_db, q, sr):
    c = K.SvfCoeffs()
    rc = K.load().cpq_eq_design_svf(btype, freq, gain_db, q, sr, C.byref(c))
    if rc != 0:
        raise CpqError(rc, "cpq_eq_design_svf")
    return c


def outfilter_design(conv_is_last, hc_mode, lc_mode, lp_mode, sr):
    out = (K.BiquadCoeffs * 3)()
    rc = K.load().cpq_outfilter_design(int(conv_is_last), hc_mode, lc_mode, lp_mode, sr, out)
    if rc != 0:
        raise CpqError(rc, "cpq_outfilter_design")
    return list(out)


def os_resolve_factor(base_rate, requested=0):
    """cpq_os_resolve_factor (OversamplingPolicy::resolve): requested 0 = Auto; 0 returned = rate not supported."""
    rc = K.load().cpq_os_resolve_factor(float(base_rate), int(requested))
    if rc < 0:
        raise CpqError(rc, "cpq_os_resolve_factor")
    return rc


def os_design_stage(stage, os_type=K.CPQ_OS_IIR):
    """cpq_os_design_stage: (info dict, raw taps float64) of one half-band stage."""
    info = K.OsStageInfo()
    n = K.load().cpq_os_design_stage(stage, os_type, C.byref(info), None, 0)
    if n < 0:
        raise CpqError(n, "cpq_os_design_stage")
    taps = np.zeros(n, dtype=np.float64)
    rc = K.load().cpq_os_design_stage(stage, os_type, None, _dp(taps), n)
    if rc < 0:
        raise CpqError(rc, "cpq_os_design_stage")
    return {f: getattr(info, f) for f, _ in K.OsStageInfo._fields_}, taps


def os_latency(factor, os_type=K.CPQ_OS_IIR):
    """cpq_os_latency: round-trip latency in base-rate samples (not an integer in general)."""
    v = K.load().cpq_os_latency(int(factor), int(os_type))
    if v < 0:
        raise CpqError(int(v), "cpq_os_latency")
    return v


def meter_kweighting(rate):
    """cpq_meter_kweighting: (pre, rlb) float64[5] each, {b0, b1, b2, a1, a2} of the two K-weighting biquads at `rate`."""
    pre, rlb = np.empty(5), np.empty(5)
    rc = K.load().cpq_meter_kweighting(float(rate), _dp(pre), _dp(rlb))
    if rc != 0:
        raise CpqError(rc, "cpq_meter_kweighting")
    return pre, rlb


def meter_tp_design_stage(stage):
    """cpq_meter_tp_design_stage: (info dict, raw taps float64) of one true-peak interpolator stage."""
    info = K.OsStageInfo()
    n = K.load().cpq_meter_tp_design_stage(stage, C.byref(info), None, 0)
    if n < 0:
        raise CpqError(n, "cpq_meter_tp_design_stage")
    taps = np.empty(n)
    rc = K.load().cpq_meter_tp_design_stage(stage, None, _dp(taps), n)
    if rc < 0:
        raise CpqError(rc, "cpq_meter_tp_design_stage")
    return {f: getattr(info, f) for f, _ in K.OsStageInfo._fields_}, taps


def out_design(rate):
    """cpq_out_design: (alpha float64[2] of the output DC blocker's sections, the limiter's release coefficient) at `rate`."""
    alpha, rel = np.empty(2), C.c_double()
    rc = K.load().cpq_out_design(float(rate), _dp(alpha), C.byref(rel))
    if rc != 0:
        raise CpqError(rc, "cpq_out_design")
    return alpha, rel.value


def soft_clip_params(amount):
    """cpq_soft_clip_params: (threshold, knee, asymmetry) of a saturation amount in 0 .. 1."""
    t, k, a = C.c_double(), C.c_double(), C.c_double()
    rc = K.load().cpq_soft_clip_params(float(amount), C.byref(t), C.byref(k), C.byref(a))
    if rc != 0:
        raise CpqError(rc, "cpq_soft_clip_params")
    return t.value, k.value, a.value


def soft_clip_host(x, callback_len, amount):
    """cpq_soft_clip_host: the host restatement of the soft clipper on one row, walked in callbacks of callback_len samples."""
    y = np.array(x, dtype=np.float64).reshape(-1)
    rc = K.load().cpq_soft_clip_host(_dp(y), y.size, int(callback_len), float(amount))
    if rc != 0:
        raise CpqError(rc, "cpq_soft_clip_host")
    return y


def soft_clip_latency(factor):
    """cpq_soft_clip_latency: base-rate samples the soft clipper adds at an oversampling factor (15 at factor 1, else 0)."""
    return K.load().cpq_soft_clip_latency(int(factor))


def dither_design(rate, shaper, bit_depth):
    """cpq_dither_design: (coefficients float64[16], scale) of a noise shaper's prepare(rate, bit_depth)."""
    coeffs, scale = np.empty(16), C.c_double()
    rc = K.load().cpq_dither_design(float(rate), int(shaper), int(bit_depth), _dp(coeffs), C.byref(scale))
    if rc != 0:
        raise CpqError(rc, "cpq_dither_design")
    return coeffs, scale.value


def pcm_bytes_per_sample(fmt):
    """cpq_pcm_bytes_per_sample: bytes of one packed sample, -1 for an unknown format."""
    return K.load().cpq_pcm_bytes_per_sample(int(fmt))


def pcm_buffer(fmt, layout, n_streams, n):
    """An empty host buffer of the packed side of a call: uint8 [n_streams * 2 * n * 3] for S24, else [2 S][n] (planar) or
    [S][n][2] (interleaved) of the format's own dtype."""
    if fmt == K.CPQ_PCM_S24:
        return np.empty(n_streams * 2 * n * 3, dtype=np.uint8)
    dt = {K.CPQ_PCM_F64: np.float64, K.CPQ_PCM_F32: np.float32, K.CPQ_PCM_S16: np.int16, K.CPQ_PCM_S32: np.int32}[fmt]
    return np.empty((n_streams, n, 2) if layout == K.CPQ_PCM_INTERLEAVED else (2 * n_streams, n), dtype=dt)


def eq_params_default():
    p = K.EqParams()
    K.load().cpq_eq_params_default(C.byref(p))
    return p


def _planes(a):
    a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
    ptrs = (K.c_double_p * a.shape[0])(*[a[c].ctypes.data_as(K.c_double_p) for c in range(a.shape[0])])
    return a, ptrs


def _ir_buffer(a, rate):
    a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
    return a, K.IrBuffer(a.shape[0], a.shape[1], float(rate), a.ctypes.data_as(K.c_double_p))


def _scale_dict(s):
    return {"scale_factor": s.scale_factor, "has_scale_factor": bool(s.has_scale_factor),
            "additional_attenuation_db": s.additional_attenuation_db, "peak_value": s.peak_value,
            "rms_value": s.rms_value, "frequency_peak_gain": s.frequency_peak_gain}


def ir_load_wav(path):
    """cpq_ir_load_wav: (planes [channels][samples] float64, sample rate)."""
    b = K.IrBuffer()
    rc = K.load().cpq_ir_load_wav(os.fsencode(path), C.byref(b))
    if rc != 0:
        raise CpqError(rc, f"cpq_ir_load_wav({path})")
    try:
        out = np.ctypeslib.as_array(b.data, shape=(b.n_channels, b.n_samples)).copy()
        return out, b.sample_rate
    finally:
        K.load().cpq_ir_buffer_free(C.byref(b))


def ir_prepare(ir, ir_rate, sample_rate, target_ir_length_sec=1.0, current_ir=None, current_scale=1.0, phase_mode=0):
    """cpq_ir_prepare: dict(ir=[channels][target] float64, scale=..., ir_peak_latency=...)."""
    keep, b = _ir_buffer(ir, ir_rate)
    cur = None
    if current_ir is not None:
        keep2, cur = _ir_buffer(current_ir, sample_rate)
    out = K.IrPrepared()
    rc = K.load().cpq_ir_prepare(C.byref(b), sample_rate, target_ir_length_sec, phase_mode, C.byref(cur) if cur is not None else None,
                                 current_scale, C.byref(out))
    if rc != 0:
        raise CpqError(rc, "cpq_ir_prepare")
    try:
        data = np.ctypeslib.as_array(out.ir.data, shape=(out.ir.n_channels, out.ir.n_samples)).copy()
        return {"ir": data, "sample_rate": out.ir.sample_rate, "scale": _scale_dict(out.scale),
                "ir_peak_latency": out.ir_peak_latency}
    finally:
        K.load().cpq_ir_prepared_free(C.byref(out))


def ir_convert_to_minimum_phase(ir, rate=48000.0):
    keep, b = _ir_buffer(ir, rate)
    out = K.IrBuffer()
    rc = K.load().cpq_ir_convert_to_minimum_phase(C.byref(b), C.byref(out))
    if rc != 0:
        raise CpqError(rc, "cpq_ir_convert_to_minimum_phase")
    try:
        return np.ctypeslib.as_array(out.data, shape=(out.n_channels, out.n_samples)).copy()
    finally:
        K.load().cpq_ir_buffer_free(C.byref(out))


def resample_design(in_rate, out_rate):
    """cpq_resample_design: dict(L, M, T, group_delay, cutoff, attenuation_db, in_rate, out_rate, taps=[L][T] float64)."""
    lib = K.load()
    info = K.ResampleInfo()
    n = lib.cpq_resample_design(float(in_rate), float(out_rate), C.byref(info), None, 0)
    if n < 0:
        raise CpqError(n, "cpq_resample_design")
    taps = np.zeros(n)
    rc = lib.cpq_resample_design(float(in_rate), float(out_rate), C.byref(info), _dp(taps), n)
    if rc < 0:
        raise CpqError(rc, "cpq_resample_design")
    return {"L": info.l, "M": info.m, "T": info.taps, "group_delay": info.group_delay, "cutoff": info.cutoff,
            "attenuation_db": info.attenuation_db, "in_rate": int(in_rate), "out_rate": int(out_rate), "taps": taps.reshape(info.l, info.taps)}


def _take_ir(b):
    try:
        return np.ctypeslib.as_array(b.data, shape=(b.n_channels, b.n_samples)).copy()
    finally:
        K.load().cpq_ir_buffer_free(C.byref(b))


def ir_resample(ir, rate, target_rate, phase=K.CPQ_RESAMPLE_LINEAR_PHASE, host=False):
    """cpq_ir_resample (host=True: cpq_ir_resample_host, no GPU): ir [channels][samples] at rate -> planes at target_rate."""
    lib = K.load()
    keep, b = _ir_buffer(ir, rate)
    out = K.IrBuffer()
    rc = (lib.cpq_ir_resample_host if host else lib.cpq_ir_resample)(C.byref(b), float(target_rate), phase, C.byref(out))
    if rc != 0:
        raise CpqError(rc, "cpq_ir_resample_host" if host else lib.cpq_last_error(None).decode())
    return _take_ir(out)


def ir_resample_batch(irs, target_rate, phase=K.CPQ_RESAMPLE_LINEAR_PHASE):
    """cpq_ir_resample_batch: irs a list of (ir [channels][samples], rate); one launch per source rate.  A list of planes."""
    lib = K.load()
    pairs = [_ir_buffer(ir, rate) for ir, rate in irs]
    bufs = (K.IrBuffer * len(pairs))(*[b for _, b in pairs])
    ptrs = (C.POINTER(K.IrBuffer) * len(pairs))(*[C.pointer(bufs[i]) for i in range(len(pairs))])
    outs = (K.IrBuffer * len(pairs))()
    rc = lib.cpq_ir_resample_batch(ptrs, len(pairs), float(target_rate), phase, outs)
    if rc != 0:
        raise CpqError(rc, lib.cpq_last_error(None).decode())
    return [_take_ir(outs[i]) for i in range(len(pairs))]


def _ir_buffer_list(irs, rate=48000.0):
    """irs: arrays [channels][samples], or (array, rate) pairs.  (what must stay alive, the pointer array)"""
    pairs = [_ir_buffer(*(ir if isinstance(ir, tuple) else (ir, rate))) for ir in irs]
    bufs = (K.IrBuffer * len(pairs))(*[b for _, b in pairs])
    ptrs = (C.POINTER(K.IrBuffer) * len(pairs))(*[C.pointer(bufs[i]) for i in range(len(pairs))])
    return (pairs, bufs), ptrs


def ir_minimum_phase_batch(irs, workspace_bytes=0):
    """cpq_ir_minimum_phase_batch on the device: irs a list of arrays [channels][samples].  (list of arrays, None where the IR was
    refused; list of statuses)."""
    lib = K.load()
    keep, ptrs = _ir_buffer_list(irs)
    n = len(irs)
    outs = (K.IrBuffer * n)()
    status = (C.c_int32 * n)()
    rc = lib.cpq_ir_minimum_phase_batch(ptrs, n, int(workspace_bytes), outs, status)
    if rc != 0:
        raise CpqError(rc, lib.cpq_last_error(None).decode())
    return [_take_ir(outs[i]) if status[i] == 0 else None for i in range(n)], [int(v) for v in status]


def ir_minimum_phase(ir, rate=48000.0):
    """cpq_ir_minimum_phase: one IR [channels][samples] on the device; CpqError(CPQ_ERR_UNSUPPORTED) where the reference gives up."""
    lib = K.load()
    keep, b = _ir_buffer(ir, rate)
    out = K.IrBuffer()
    rc = lib.cpq_ir_minimum_phase(C.byref(b), C.byref(out))
    if rc != 0:
        raise CpqError(rc, lib.cpq_last_error(None).decode())
    return _take_ir(out)


def ir_prepare_batch(irs, sample_rate, target_ir_length_sec=1.0, current_irs=None, current_scales=None, phase_mode=0):
    """cpq_ir_prepare_batch: irs a list of (ir [channels][samples], rate); current_irs None or a list with None entries;
    current_scales None or a list.  A list of ir_prepare's dicts."""
    lib = K.load()
    n = len(irs)
    keep, ptrs = _ir_buffer_list(irs)
    cur_ptrs = None
    if current_irs is not None:
        cur = [None if c is None else _ir_buffer(c, sample_rate) for c in current_irs]
        cur_ptrs = (C.POINTER(K.IrBuffer) * n)(*[C.POINTER(K.IrBuffer)() if c is None else C.pointer(c[1]) for c in cur])
    scales = None if current_scales is None else (C.c_double * n)(*[float(v) for v in current_scales])
    outs = (K.IrPrepared * n)()
    rc = lib.cpq_ir_prepare_batch(ptrs, n, float(sample_rate), float(target_ir_length_sec), int(phase_mode), cur_ptrs, scales, outs)
    if rc != 0:
        raise CpqError(rc, lib.cpq_last_error(None).decode())
    res = []
    for i in range(n):
        o = outs[i]
        try:
            data = np.ctypeslib.as_array(o.ir.data, shape=(o.ir.n_channels, o.ir.n_samples)).copy()
            res.append({"ir": data, "sample_rate": o.ir.sample_rate, "scale": _scale_dict(o.scale), "ir_peak_latency": o.ir_peak_latency})
        finally:
            lib.cpq_ir_prepared_free(C.byref(o))
    return res


def ir_compute_scale_factor(ir, current_ir=None, current_scale=1.0):
    a, pa = _planes(ir)
    cur_ptrs, cc, cn = None, 0, 0
    if current_ir is not None:
        c, cur_ptrs = _planes(current_ir)
        cc, cn = c.shape
    out = K.IrScale()
    rc = K.load().cpq_ir_compute_scale_factor(pa, a.shape[0], a.shape[1], cur_ptrs, cc, cn, current_scale, C.byref(out))
    if rc != 0:
        raise CpqError(rc, "cpq_ir_compute_scale_factor")
    return _scale_dict(out)


def ir_estimate_max_frequency_response_gain(ir):
    a, pa = _planes(ir)
    return K.load().cpq_ir_estimate_max_frequency_response_gain(pa, a.shape[0], a.shape[1])


def ir_estimate_peak_latency(ir):
    a, pa = _planes(ir)
    return K.load().cpq_ir_estimate_peak_latency(pa, a.shape[0], a.shape[1])


class BatchedEngine:
    def __init__(self, n_streams, block_size=512, max_ir_len=131072, max_blocks_per_call=64,
                 semantics=K.CPQ_SEM_REFERENCE, device=0, sample_rate=48000.0, mac_tile=0, partition_size=0,
                 schedule=K.CPQ_SCHED_UNIFORM, call_mode=K.CPQ_CALLS_WHOLE_BLOCKS):
        self._lib = K.load()
        self._h = K._E()
        d = K.EngineDesc(C.sizeof(K.EngineDesc), device, n_streams, block_size, max_ir_len, max_blocks_per_call,
                         semantics, mac_tile, sample_rate, partition_size, schedule, call_mode, 0)
        rc = self._lib.cpq_engine_create(C.byref(d), C.byref(self._h))
        if rc != 0:
            raise CpqError(rc, self._lib.cpq_last_error(None).decode())
        self.n_streams = n_streams
        self.n_channels = 2 * n_streams
        self.block_size = block_size
        self.os_factor = 1

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cpq_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _ck(self, rc):
        if rc != 0:
            raise CpqError(rc, self._lib.cpq_last_error(self._h).decode())

    # ---- control surface
    def set_stream(self, hip_stream_ptr):
        self._ck(self._lib.cpq_engine_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def synchronize(self):
        self._ck(self._lib.cpq_engine_synchronize(self._h))

    def arena_bytes(self):
        return self._lib.cpq_engine_arena_bytes(self._h)

    def partition_size(self):
        """The internal FFT partition in use (what CPQ_PARTITION_AUTO resolved to)."""
        return self._lib.cpq_engine_partition_size(self._h)

    def prepare_to_play(self, sample_rate, max_block):
        self._ck(self._lib.cpq_engine_prepare(self._h, sample_rate, max_block))

    def set_order(self, order):
        self._ck(self._lib.cpq_engine_set_order(self._h, order))

    def set_impulse(self, stream, ir_l, ir_r, scale=1.0, direct_head=False, spec=None):
        ir_l = np.ascontiguousarray(ir_l, dtype=np.float64)
        ir_r = np.ascontiguousarray(ir_r, dtype=np.float64)
        assert len(ir_l) == len(ir_r)
        self._ck(self._lib.cpq_conv_set_impulse(self._h, stream, _dp(ir_l), _dp(ir_r), len(ir_l), scale,
                                                int(direct_head), C.byref(spec) if spec is not None else None))

    def set_eq_params(self, stream, params):
        self._ck(self._lib.cpq_eq_set_params(self._h, stream, C.byref(params)))

    def set_gains(self, stream, conv_input_trim_gain=1.0, output_makeup_gain=1.0):
        self._ck(self._lib.cpq_engine_set_gains(self._h, stream, conv_input_trim_gain, output_makeup_gain))

    def set_conv_bypass(self, bypassed):
        self._ck(self._lib.cpq_engine_set_conv_bypass(self._h, int(bypassed)))

    def request_band_reset(self, stream, band_mask=0xFFFFFFFF):
        self._ck(self._lib.cpq_eq_request_band_reset(self._h, stream, band_mask))

    def request_agc_reset(self, stream):
        self._ck(self._lib.cpq_eq_request_agc_reset(self._h, stream))

    def set_eq_bypass(self, stream, bypassed):
        self._ck(self._lib.cpq_eq_set_bypass(self._h, stream, int(bypassed)))

    def set_convproc_params(self, stream, mix=1.0, bypassed=False, ir_peak_latency=0, smoothing_time_sec=0.0):
        p = K.ConvProcParams(mix, int(bypassed), ir_peak_latency, smoothing_time_sec)
        self._ck(self._lib.cpq_convproc_set_params(self._h, stream, C.byref(p)))

    def convproc_delay(self, stream):
        return self._lib.cpq_convproc_delay(self._h, stream)

    def set_conv_level(self, level):
        self._ck(self._lib.cpq_engine_set_conv_level(self._h, level))

    def convproc_process(self, x):
        return self._host(self._lib.cpq_convproc_process, x)

    def set_outfilter_params(self, stream, conv_is_last, hc_mode=1, lc_mode=0, lp_mode=1):
        self._ck(self._lib.cpq_outfilter_set_params(self._h, stream, int(conv_is_last), hc_mode, lc_mode, lp_mode))

    def outfilter_process(self, x):
        return self._host(self._lib.cpq_outfilter_process, x)

    def enable_output_filter(self, on=True):
        self._ck(self._lib.cpq_engine_enable_output_filter(self._h, int(on)))

    def outfilter_reset(self):
        self._ck(self._lib.cpq_outfilter_reset(self._h))

    def set_eq_mode(self, mode):
        self._ck(self._lib.cpq_eq_set_mode(self._h, mode))

    def conv_reset(self):
        self._ck(self._lib.cpq_conv_reset(self._h))

    def eq_reset(self):
        self._ck(self._lib.cpq_eq_reset(self._h))

    def is_ready(self):
        return bool(self._lib.cpq_conv_is_ready(self._h))

    def latency(self):
        return self._lib.cpq_conv_latency(self._h)

    def last_got(self, stream=0):
        return self._lib.cpq_conv_last_got(self._h, stream)

    def plan(self):
        p = K.NucPlan()
        self._ck(self._lib.cpq_conv_get_plan(self._h, C.byref(p)))
        return p

    # ---- oversampling (CustomInputOversampler around the routing)
    def set_oversampling(self, factor, os_type=K.CPQ_OS_IIR):
        self._ck(self._lib.cpq_engine_set_oversampling(self._h, int(factor), int(os_type)))
        self.os_factor = int(factor)

    def os_up(self, x):
        """processUp: [n_channels, n] -> [n_channels, n * factor]"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.ndim == 2 and x.shape[0] == self.n_channels
        y = np.empty((self.n_channels, x.shape[1] * self.os_factor), dtype=np.float64)
        self._ck(self._lib.cpq_os_up(self._h, _dp(x), _dp(y), x.shape[1]))
        return y

    def os_down(self, x):
        """processDown: [n_channels, n * factor] -> [n_channels, n]"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.ndim == 2 and x.shape[0] == self.n_channels and x.shape[1] % self.os_factor == 0
        y = np.empty((self.n_channels, x.shape[1] // self.os_factor), dtype=np.float64)
        self._ck(self._lib.cpq_os_down(self._h, _dp(x), _dp(y), y.shape[1]))
        return y

    def os_up_device(self, d_in, d_out, n_base):
        self._ck(self._lib.cpq_os_up_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n_base))

    def os_down_device(self, d_in, d_out, n_base):
        self._ck(self._lib.cpq_os_down_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n_base))

    def os_reset(self):
        self._ck(self._lib.cpq_os_reset(self._h))

    def os_telemetry(self, stream):
        t = K.OsTelemetry()
        self._ck(self._lib.cpq_os_read_telemetry(self._h, stream, C.byref(t)))
        return {f: getattr(t, f) for f, _ in K.OsTelemetry._fields_ if f != "reserved"}

    # ---- metering (LoudnessMeter / TruePeakDetector on the base-rate output rows)
    def set_metering(self, flags):
        self._ck(self._lib.cpq_engine_set_metering(self._h, int(flags)))

    def meter_reset(self):
        self._ck(self._lib.cpq_meter_reset(self._h))

    def meter_process(self, x):
        """Meter rows [n_channels, n] as the engine's output would be, without running the chain."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.ndim == 2 and x.shape[0] == self.n_channels
        self._ck(self._lib.cpq_meter_process(self._h, _dp(x), x.shape[1]))

    def meter_process_device(self, d_in, n_samples):
        self._ck(self._lib.cpq_meter_process_device(self._h, C.c_void_p(d_in), n_samples))

    def meter_read_blocks(self, max_blocks=K.METER_RING):
        """Pops up to max_blocks records per stream: (structured array [n_streams, n], records dropped since the last read)."""
        buf = (K.MeterBlock * (self.n_streams * max_blocks))()
        n = C.c_int32()
        dropped = C.c_int64()
        self._ck(self._lib.cpq_meter_read_blocks(self._h, buf, max_blocks, C.byref(n), C.byref(dropped)))
        dt = np.dtype([(f, np.uint64 if f == "block_index" else np.float64) for f, _ in K.MeterBlock._fields_])
        rec = np.frombuffer(buf, dtype=dt).reshape(self.n_streams, max_blocks)[:, :n.value].copy()
        return rec, dropped.value

    # ---- soft clipper (between the make-up gain and the down stages; at factor 1 with its local 2x pair)
    def set_soft_clip(self, stream, enabled, saturation_amount=0.0):
        self._ck(self._lib.cpq_engine_set_soft_clip(self._h, int(stream), int(bool(enabled)), float(saturation_amount)))

    def soft_clip_reset(self):
        self._ck(self._lib.cpq_soft_clip_reset(self._h))

    def soft_clip_process(self, x, callback_len):
        """The kernel alone on rows [n_channels, n], walked in callbacks of callback_len samples."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.ndim == 2 and x.shape[0] == self.n_channels
        y = np.empty_like(x)
        self._ck(self._lib.cpq_soft_clip_process(self._h, _dp(x), _dp(y), x.shape[1], int(callback_len)))
        return y

    def soft_clip_process_device(self, d_in, d_out, n_samples, callback_len):
        self._ck(self._lib.cpq_soft_clip_process_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n_samples, int(callback_len)))

    def soft_clip_telemetry(self, stream):
        t = K.OsTelemetry()
        self._ck(self._lib.cpq_soft_clip_read_telemetry(self._h, stream, C.byref(t)))
        return {f: getattr(t, f) for f, _ in K.OsTelemetry._fields_ if f != "reserved"}

    # ---- output stage (DC blocker, headroom + scrub, limiter, clamp on the base-rate rows)
    def set_output_stage(self, flags):
        self._ck(self._lib.cpq_engine_set_output_stage(self._h, int(flags)))

    def out_reset(self):
        self._ck(self._lib.cpq_out_reset(self._h))

    def out_process(self, x):
        """The stage alone on rows [n_channels, n], as the engine's output would pass it."""
        return self._host(self._lib.cpq_out_process, x)

    def out_process_device(self, d_in, d_out, n_samples):
        self._ck(self._lib.cpq_out_process_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n_samples))

    def out_read_envelope(self, stream):
        v = C.c_double()
        self._ck(self._lib.cpq_out_read_envelope(self._h, int(stream), C.byref(v)))
        return v.value

    # ---- dither stage (the fixed 4- and 15-tap and the adaptive lattice noise shaper; headroom and scrub follow the output-stage flags)
    def set_dither(self, shaper, bit_depth=0):
        self._ck(self._lib.cpq_engine_set_dither(self._h, int(shaper), int(bit_depth)))

    def dither_reset(self):
        self._ck(self._lib.cpq_dither_reset(self._h))

    def dither_set_adaptive_coeffs(self, stream, k):
        """applyMatchedCoefficients of one stream or CPQ_ALL_STREAMS: up to nine reflection coefficients, clamped; states cleared."""
        k = np.ascontiguousarray(k, dtype=np.float64).reshape(-1)
        self._ck(self._lib.cpq_dither_set_adaptive_coeffs(self._h, int(stream), _dp(k) if k.size else None, k.size))

    def dither_get_adaptive_coeffs(self, stream):
        k = np.empty(9)
        self._ck(self._lib.cpq_dither_get_adaptive_coeffs(self._h, int(stream), _dp(k)))
        return k

    def dither_process(self, x):
        """The stage alone on rows [n_channels, n]."""
        return self._host(self._lib.cpq_dither_process, x)

    def dither_process_device(self, d_in, d_out, n_samples):
        self._ck(self._lib.cpq_dither_process_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n_samples))

    # ---- host-buffer processing: x is [n_channels, n_samples] float64
    def _host(self, fn, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.ndim == 2 and x.shape[0] == self.n_channels
        y = np.empty_like(x)
        self._ck(fn(self._h, _dp(x), _dp(y), x.shape[1]))
        return y

    def conv_process(self, x):
        return self._host(self._lib.cpq_conv_process, x)

    def eq_process(self, x):
        return self._host(self._lib.cpq_eq_process, x)

    def process(self, x):
        return self._host(self._lib.cpq_engine_process_block, x)

    # ---- packed PCM in and out: buffers are contiguous numpy arrays of the packed side (pcm_buffer), n samples per channel
    def _pcm_ptr(self, a, fmt, n):
        assert a.flags["C_CONTIGUOUS"] and a.nbytes == self.n_channels * n * K.load().cpq_pcm_bytes_per_sample(fmt), "packed buffer size"
        return C.c_void_p(a.ctypes.data)

    def pcm_unpack(self, pcm, fmt, n, layout=K.CPQ_PCM_PLANAR, flags=0):
        """cpq_pcm_unpack: packed buffer -> rows [n_channels, n] float64"""
        rows = np.empty((self.n_channels, n), dtype=np.float64)
        self._ck(self._lib.cpq_pcm_unpack(self._h, self._pcm_ptr(pcm, fmt, n), fmt, layout, flags, C.c_void_p(rows.ctypes.data), n))
        return rows

    def pcm_pack(self, rows, fmt, layout=K.CPQ_PCM_PLANAR):
        """cpq_pcm_pack: rows [n_channels, n] float64 -> packed buffer"""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert rows.ndim == 2 and rows.shape[0] == self.n_channels
        out = pcm_buffer(fmt, layout, self.n_streams, rows.shape[1])
        self._ck(self._lib.cpq_pcm_pack(self._h, C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data), fmt, layout, rows.shape[1]))
        return out

    def pcm_unpack_device(self, d_pcm, fmt, d_rows, n, layout=K.CPQ_PCM_PLANAR, flags=0):
        self._ck(self._lib.cpq_pcm_unpack_device(self._h, C.c_void_p(d_pcm), fmt, layout, flags, C.c_void_p(d_rows), n))

    def pcm_pack_device(self, d_rows, d_pcm, fmt, n, layout=K.CPQ_PCM_PLANAR):
        self._ck(self._lib.cpq_pcm_pack_device(self._h, C.c_void_p(d_rows), C.c_void_p(d_pcm), fmt, layout, n))

    def process_pcm(self, x, in_format, out_format, n, layout=K.CPQ_PCM_PLANAR, flags=0, out=None):
        """cpq_engine_process_block_pcm: the whole chain on a packed buffer; returns the packed result (`out`, or a new buffer)."""
        if out is None:
            out = pcm_buffer(out_format, layout, self.n_streams, n)
        self._ck(self._lib.cpq_engine_process_block_pcm(self._h, self._pcm_ptr(x, in_format, n), in_format,
                                                        self._pcm_ptr(out, out_format, n), out_format, layout, flags, n))
        return out

    def process_pcm_device(self, d_in, in_format, d_out, out_format, n, layout=K.CPQ_PCM_PLANAR, flags=0):
        self._ck(self._lib.cpq_engine_process_block_pcm_device(self._h, C.c_void_p(d_in), in_format, C.c_void_p(d_out), out_format,
                                                               layout, flags, n))

    # ---- device-pointer processing (no sync): raw HBM addresses
    def conv_process_device(self, d_in, d_out, n_samples):
        self._ck(self._lib.cpq_conv_process_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n_samples))

    def eq_process_device(self, d_in, d_out, n_samples):
        self._ck(self._lib.cpq_eq_process_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n_samples))

    def process_device(self, d_in, d_out, n_samples):
        self._ck(self._lib.cpq_engine_process_block_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n_samples))

    # ---- profiling
    def profile_enable(self, on=True):
        self._ck(self._lib.cpq_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._ck(self._lib.cpq_profile_reset(self._h))

    def profile_read(self):
        out = {}
        for name, kid in K.KERNEL_IDS.items():
            n = C.c_int64()
            ms = C.c_double()
            self._ck(self._lib.cpq_profile_read(self._h, kid, C.byref(n), C.byref(ms)))
            if name in ("k_os_halfband", "k_meter", "k_pcm", "k_out", "k_dither") and n.value == 0:
                continue        # listed only for engines that oversample / meter / take packed PCM / run the output stage / dither
            out[name] = (n.value, ms.value)
        n, ms = C.c_int64(), C.c_double()
        self._ck(self._lib.cpq_profile_read(self._h, K.CPQ_K_SOFTCLIP, C.byref(n), C.byref(ms)))
        if n.value:
            out["k_soft_clip"] = (n.value, ms.value)      # listed only for engines that ran the soft clipper
        return out

    def eq_chain_status(self):
        """(chained launches of the EQ / output-filter cascade so far, hand-over gave up flag) -- diagnostics for tests"""
        n = C.c_uint32()
        bad = C.c_uint32()
        self._ck(self._lib.cpq_diag_eq_chain_status(self._h, C.byref(n), C.byref(bad)))
        return n.value, bad.value
