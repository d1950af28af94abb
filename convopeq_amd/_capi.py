"""ctypes binding of libconvopeq_mi355x.so (the C ABI declared in include/convopeq_mi355x.h).

The library is the product; this module only loads it.  There is no Python or CPU fallback: if the
shared object is missing or a symbol is absent, import fails loudly.
"""
import ctypes as C
import importlib.util
import os
import sys

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "libconvopeq_mi355x.so")

CPQ_OK = 0
CPQ_ERR_INVALID_ARG = -1
CPQ_ERR_NO_DEVICE = -2
CPQ_ERR_OOM = -3
CPQ_ERR_DEVICE = -4
CPQ_ERR_UNSUPPORTED = -5
CPQ_ERR_NOT_READY = -6
CPQ_ERR_SILENT_IR = -7
CPQ_ALL_STREAMS = -1
CPQ_SEM_REFERENCE = 0
CPQ_SEM_EXACT = 1
CPQ_SCHED_UNIFORM = 0
CPQ_SCHED_REFERENCE_NUC = 1
CPQ_CALLS_WHOLE_BLOCKS = 0
CPQ_CALLS_ANY = 1
CPQ_PARTITION_AUTO = -1
CPQ_ORDER_CONV_THEN_EQ = 0
CPQ_ORDER_EQ_THEN_CONV = 1
KERNEL_IDS = {"k_rfft_fwd_ols": 0, "k_fdl_mac": 1, "k_fdl_mac_dcnyq": 2, "k_rfft_inv_ols": 3, "k_svf_cascade": 4,
              "k_svf_cascade_tp": 5, "k_convproc_mix": 6, "k_outfilter_cascade": 7, "k_os_halfband": 8, "k_meter": 9,
              "k_pcm": 10, "k_out": 11, "k_dither": 12}
CPQ_K_SOFTCLIP = 14         # id 13 stays unassigned (cpq_kernel_name(13) is "?"); profile_read lists "k_soft_clip" when it ran
CPQ_LEVEL_NUC = 0
CPQ_LEVEL_PROCESSOR = 1
CPQ_EQ_MODE_AUTO = 0
CPQ_EQ_MODE_SEQUENTIAL = 1
CPQ_PHASE_AS_IS = 0
CPQ_PHASE_MIXED = 1
CPQ_PHASE_MINIMUM = 2
CPQ_RESAMPLE_LINEAR_PHASE = 0
CPQ_RESAMPLE_MINIMUM_PHASE = 1
CPQ_RESAMPLE_MAX_FACTOR = 1280
CPQ_SRC_HOST = 1
CPQ_SRC_DEVICE = 2
CPQ_LIM_HOST = 1
CPQ_LIM_DEVICE = 2
CPQ_QUANT_HOST = 1
CPQ_QUANT_DEVICE = 2
CPQ_OS_IIR = 0
CPQ_OS_LINEAR_PHASE = 1
CPQ_METER_LOUDNESS = 1
CPQ_METER_TRUE_PEAK = 2
METER_RING = 4096
CPQ_OUT_DC_BLOCK = 1
CPQ_OUT_HEADROOM = 2
CPQ_OUT_LIMITER = 4
CPQ_OUT_CLAMP = 8
CPQ_OUT_ALL = 15
CPQ_DITHER_OFF = 0
CPQ_DITHER_FIXED4 = 1
CPQ_DITHER_FIXED15 = 2
CPQ_DITHER_ADAPTIVE9 = 4
CPQ_DITHER_TILE = 64
CPQ_SCORE_RNG_FRESH = 0
CPQ_SCORE_RNG_CHAINED = 1
CPQ_SCORE_SEGMENT_LEN = 4096
CPQ_SCORE_MAX_SEGMENTS = 16
CPQ_SCORE_RECENT = 4096 + 2048 * 15
CPQ_SCORE_BINS = 2049
CPQ_SCORE_MAX_CANDIDATES = 1024
CPQ_SCORE_UNSTABLE = 1e18
CPQ_LEARN_DIM = 9
CPQ_LEARN_POPULATION = 18
CPQ_LEARN_ELITE = 6
CPQ_LEARN_MAX_GENERATIONS = 4096
CPQ_LEARN_MAX_TRIES = 32
CPQ_LEARN_SHORTEST, CPQ_LEARN_SHORT, CPQ_LEARN_MIDDLE, CPQ_LEARN_LONG, CPQ_LEARN_ULTRA, CPQ_LEARN_CONTINUOUS = range(6)
CPQ_SEGMENT_BROADBAND = 0
CPQ_SEGMENT_TONAL = 1
CPQ_SEGMENT_TRANSIENT = 2
CPQ_PCM_F64 = 0
CPQ_PCM_F32 = 1
CPQ_PCM_S16 = 2
CPQ_PCM_S24 = 3
CPQ_PCM_S32 = 4
CPQ_PCM_PLANAR = 0
CPQ_PCM_INTERLEAVED = 1
CPQ_PCM_SANITIZE = 1

c_double_p = C.POINTER(C.c_double)


class FilterSpec(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("hc_mode", C.c_int32), ("lc_mode", C.c_int32),
                ("tail_mode", C.c_int32), ("tail_enabled", C.c_int32), ("tail_start_seconds", C.c_double),
                ("tail_strength", C.c_double), ("tail_l1l2_multiplier", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def defaults(cls, **kw):
        s = cls(48000.0, 1, 0, 1, 1, 0.085, 1.0, 8, 0)
        for k, v in kw.items():
            setattr(s, k, v)
        return s


class NucPlan(C.Structure):
    _fields_ = [("num_layers", C.c_int32), ("part_size", C.c_int32 * 3), ("offset", C.c_int32 * 3),
                ("len", C.c_int32 * 3), ("num_parts_ir", C.c_int32 * 3), ("num_parts", C.c_int32 * 3),
                ("parts_per_callback", C.c_int32 * 3), ("output_delay", C.c_int32 * 3),
                ("gain", C.c_double * 3), ("direct_taps", C.c_int32), ("latency", C.c_int32),
                ("lti_valid", C.c_int32), ("done_callback", C.c_int32 * 3), ("lag", C.c_int32 * 3),
                ("heff_len", C.c_int32)]


class SvfCoeffs(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("g", "k", "a1", "a2", "a3", "m0", "m1", "m2")]


class EqBand(C.Structure):
    _fields_ = [("frequency", C.c_float), ("gain", C.c_float), ("q", C.c_float),
                ("enabled", C.c_int32), ("type", C.c_int32), ("channel_mode", C.c_int32)]


class EqParams(C.Structure):
    _fields_ = [("bands", EqBand * 20), ("total_gain_db", C.c_float), ("agc_enabled", C.c_int32),
                ("nonlinear_saturation", C.c_float), ("filter_structure", C.c_int32)]


class BiquadCoeffs(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("b0", "b1", "b2", "a1", "a2")]


class ConvProcParams(C.Structure):
    _fields_ = [("mix", C.c_float), ("bypassed", C.c_int32), ("ir_peak_latency", C.c_int32), ("smoothing_time_sec", C.c_float)]


class IrBuffer(C.Structure):
    _fields_ = [("n_channels", C.c_int32), ("n_samples", C.c_int32), ("sample_rate", C.c_double), ("data", c_double_p)]


class IrScale(C.Structure):
    _fields_ = [("scale_factor", C.c_double), ("has_scale_factor", C.c_int32), ("additional_attenuation_db", C.c_float),
                ("peak_value", C.c_double), ("rms_value", C.c_double), ("frequency_peak_gain", C.c_double)]


class IrPrepared(C.Structure):
    _fields_ = [("ir", IrBuffer), ("scale", IrScale), ("ir_peak_latency", C.c_int32), ("reserved", C.c_int32)]


class ResampleInfo(C.Structure):
    _fields_ = [("l", C.c_int32), ("m", C.c_int32), ("taps", C.c_int32), ("reserved", C.c_int32), ("group_delay", C.c_double),
                ("cutoff", C.c_double), ("attenuation_db", C.c_double)]


class SrcDesc(C.Structure):
    _fields_ = [("n_channels", C.c_int32), ("in_rate", C.c_double), ("out_rate", C.c_double), ("max_in", C.c_int32), ("phase", C.c_int32),
                ("flags", C.c_uint32), ("start_period", C.c_int64)]


class LoudnessDesc(C.Structure):
    _fields_ = [("n_streams", C.c_int32), ("sample_rate", C.c_double), ("max_seconds", C.c_double), ("flags", C.c_int32)]


class LoudnessResult(C.Structure):
    _fields_ = [("integrated", C.c_double), ("range", C.c_double), ("momentary_max", C.c_double), ("short_term_max", C.c_double),
                ("relative_gate", C.c_double), ("n_hops", C.c_int64), ("n_blocks", C.c_int32), ("n_abs", C.c_int32),
                ("n_rel", C.c_int32), ("n_short_kept", C.c_int32)]


class LoudnessPeaks(C.Structure):
    _fields_ = [("true_peak", C.c_double * 2), ("sample_peak", C.c_double * 2)]


class LimiterTelemetry(C.Structure):
    _fields_ = [("min_gain", C.c_double), ("limited_samples", C.c_int64)]


class OsStageInfo(C.Structure):
    _fields_ = [("taps", C.c_int32), ("center_tap", C.c_int32), ("center_parity", C.c_int32), ("conv_parity", C.c_int32),
                ("conv_count", C.c_int32), ("center_delay_input", C.c_int32), ("history_up_keep", C.c_int32),
                ("history_down_keep", C.c_int32), ("attenuation_db", C.c_double), ("center_coeff", C.c_double)]


class OsTelemetry(C.Structure):
    _fields_ = [("corruption_events", C.c_uint64), ("auto_clears", C.c_uint64), ("consecutive_auto_clears", C.c_int32),
                ("hard_fallback", C.c_int32), ("corruption_pending", C.c_int32), ("reserved", C.c_int32)]


class MeterBlock(C.Structure):
    _fields_ = [("mean_square", C.c_double), ("peak_linear", C.c_double), ("true_peak", C.c_double),
                ("true_peak_hold", C.c_double), ("block_index", C.c_uint64)]


class ScorerDesc(C.Structure):
    _fields_ = [("n_learners", C.c_int32), ("max_candidates", C.c_int32), ("sample_rate_hz", C.c_double), ("bit_depth", C.c_int32),
                ("level_weights", C.c_double * 4), ("coeff_safety_margin", C.c_double), ("stability_check", C.c_int32),
                ("rng_mode", C.c_int32)]


class ScoreParts(C.Structure):
    _fields_ = [("noise_power", C.c_double), ("spectral_flatness_penalty", C.c_double), ("hf_penalty", C.c_double),
                ("time_domain_rms", C.c_double), ("composite_score", C.c_double)]


class ScoreSegment(C.Structure):
    _fields_ = [("start", C.c_int32), ("level", C.c_int32), ("type", C.c_int32), ("reserved", C.c_int32), ("gain", C.c_double)]


class DiagScoreEval(C.Structure):
    _fields_ = [("row", C.c_int32), ("thr", C.c_int32), ("slot", C.c_int32), ("reserved", C.c_int32), ("alpha", C.c_double)]


class DiagScoreChain(C.Structure):
    _fields_ = [("src", C.c_int32), ("dst", C.c_int32), ("coef", C.c_int32), ("rng", C.c_int32)]


class LearnParams(C.Structure):
    _fields_ = [("sigma_min", C.c_double), ("sigma_max", C.c_double), ("cov_retention_target", C.c_double),
                ("cov_retention_step", C.c_double), ("level_weights", C.c_double * 4)]


class LearnState(C.Structure):
    _fields_ = [("mean", C.c_double * 9), ("cov_upper", C.c_double * 45), ("sigma", C.c_double), ("cov_retention", C.c_double),
                ("rng", C.c_uint64 * 4), ("best_score", C.c_double), ("best_raw", C.c_double * 9), ("best_scored", C.c_double * 9),
                ("generations", C.c_int32), ("rejected_pairs", C.c_int32)]


class EngineDesc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("n_streams", C.c_int32),
                ("block_size", C.c_int32), ("max_ir_len", C.c_int32), ("max_blocks_per_call", C.c_int32),
                ("semantics", C.c_int32), ("mac_tile", C.c_int32), ("sample_rate", C.c_double),
                ("partition_size", C.c_int32), ("schedule", C.c_int32), ("call_mode", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/convopeq_mi355x.h declares: (restype, argtypes)
_E = C.c_void_p
_i32p, _i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

SYMBOLS = {
    "cpq_abi_version": (C.c_int32, []),
    "cpq_abi_revision": (C.c_int32, []),
    "cpq_status_string": (C.c_char_p, [C.c_int32]),
    "cpq_last_error": (C.c_char_p, [_E]),
    "cpq_nuc_plan_compute": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(FilterSpec), C.POINTER(NucPlan)]),
    "cpq_nuc_heff": (C.c_int32, [c_double_p, C.c_int32, C.c_int32, C.c_double, C.POINTER(FilterSpec), c_double_p, C.c_int32]),
    "cpq_eq_design_svf": (C.c_int32, [C.c_int32, C.c_float, C.c_float, C.c_float, C.c_double, C.POINTER(SvfCoeffs)]),
    "cpq_eq_params_default": (None, [C.POINTER(EqParams)]),
    "cpq_engine_create": (C.c_int32, [C.POINTER(EngineDesc), C.POINTER(_E)]),
    "cpq_engine_destroy": (None, [_E]),
    "cpq_engine_set_stream": (C.c_int32, [_E, C.c_void_p]),
    "cpq_engine_synchronize": (C.c_int32, [_E]),
    "cpq_engine_arena_bytes": (C.c_int64, [_E]),
    "cpq_engine_partition_size": (C.c_int32, [_E]),
    "cpq_engine_prepare": (C.c_int32, [_E, C.c_double, C.c_int32]),
    "cpq_engine_set_order": (C.c_int32, [_E, C.c_int32]),
    "cpq_host_register": (C.c_int32, [C.c_void_p, C.c_size_t]),
    "cpq_host_unregister": (C.c_int32, [C.c_void_p]),
    "cpq_conv_set_impulse": (C.c_int32, [_E, C.c_int32, c_double_p, c_double_p, C.c_int32, C.c_double, C.c_int32, C.POINTER(FilterSpec)]),
    "cpq_conv_process": (C.c_int32, [_E, c_double_p, c_double_p, C.c_int32]),
    "cpq_conv_process_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32]),
    "cpq_conv_reset": (C.c_int32, [_E]),
    "cpq_conv_is_ready": (C.c_int32, [_E]),
    "cpq_conv_latency": (C.c_int32, [_E]),
    "cpq_conv_get_plan": (C.c_int32, [_E, C.POINTER(NucPlan)]),
    "cpq_conv_last_got": (C.c_int32, [_E, C.c_int32]),
    "cpq_convproc_set_params": (C.c_int32, [_E, C.c_int32, C.POINTER(ConvProcParams)]),
    "cpq_convproc_process": (C.c_int32, [_E, c_double_p, c_double_p, C.c_int32]),
    "cpq_convproc_process_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32]),
    "cpq_convproc_delay": (C.c_int32, [_E, C.c_int32]),
    "cpq_engine_set_conv_level": (C.c_int32, [_E, C.c_int32]),
    "cpq_eq_set_params": (C.c_int32, [_E, C.c_int32, C.POINTER(EqParams)]),
    "cpq_eq_process": (C.c_int32, [_E, c_double_p, c_double_p, C.c_int32]),
    "cpq_eq_process_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32]),
    "cpq_eq_set_bypass": (C.c_int32, [_E, C.c_int32, C.c_int32]),
    "cpq_eq_request_band_reset": (C.c_int32, [_E, C.c_int32, C.c_uint32]),
    "cpq_eq_request_agc_reset": (C.c_int32, [_E, C.c_int32]),
    "cpq_eq_set_mode": (C.c_int32, [_E, C.c_int32]),
    "cpq_eq_reset": (C.c_int32, [_E]),
    "cpq_outfilter_design": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.POINTER(BiquadCoeffs)]),
    "cpq_outfilter_set_params": (C.c_int32, [_E, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "cpq_outfilter_process": (C.c_int32, [_E, c_double_p, c_double_p, C.c_int32]),
    "cpq_outfilter_process_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32]),
    "cpq_outfilter_reset": (C.c_int32, [_E]),
    "cpq_engine_enable_output_filter": (C.c_int32, [_E, C.c_int32]),
    "cpq_engine_set_gains": (C.c_int32, [_E, C.c_int32, C.c_double, C.c_double]),
    "cpq_engine_set_conv_bypass": (C.c_int32, [_E, C.c_int32]),
    "cpq_engine_process_block": (C.c_int32, [_E, c_double_p, c_double_p, C.c_int32]),
    "cpq_engine_process_block_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32]),
    "cpq_os_resolve_factor": (C.c_int32, [C.c_double, C.c_int32]),
    "cpq_os_design_stage": (C.c_int32, [C.c_int32, C.c_int32, C.POINTER(OsStageInfo), c_double_p, C.c_int32]),
    "cpq_os_latency": (C.c_double, [C.c_int32, C.c_int32]),
    "cpq_engine_set_oversampling": (C.c_int32, [_E, C.c_int32, C.c_int32]),
    "cpq_os_up": (C.c_int32, [_E, c_double_p, c_double_p, C.c_int32]),
    "cpq_os_up_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32]),
    "cpq_os_down": (C.c_int32, [_E, c_double_p, c_double_p, C.c_int32]),
    "cpq_os_down_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32]),
    "cpq_os_reset": (C.c_int32, [_E]),
    "cpq_os_read_telemetry": (C.c_int32, [_E, C.c_int32, C.POINTER(OsTelemetry)]),
    "cpq_meter_kweighting": (C.c_int32, [C.c_double, c_double_p, c_double_p]),
    "cpq_meter_tp_design_stage": (C.c_int32, [C.c_int32, C.POINTER(OsStageInfo), c_double_p, C.c_int32]),
    "cpq_engine_set_metering": (C.c_int32, [_E, C.c_int32]),
    "cpq_meter_reset": (C.c_int32, [_E]),
    "cpq_meter_process": (C.c_int32, [_E, c_double_p, C.c_int32]),
    "cpq_meter_process_device": (C.c_int32, [_E, C.c_void_p, C.c_int32]),
    "cpq_meter_read_blocks": (C.c_int32, [_E, C.POINTER(MeterBlock), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "cpq_soft_clip_params": (C.c_int32, [C.c_float, c_double_p, c_double_p, c_double_p]),
    "cpq_soft_clip_host": (C.c_int32, [c_double_p, C.c_int32, C.c_int32, C.c_float]),
    "cpq_soft_clip_latency": (C.c_double, [C.c_int32]),
    "cpq_engine_set_soft_clip": (C.c_int32, [_E, C.c_int32, C.c_int32, C.c_float]),
    "cpq_soft_clip_reset": (C.c_int32, [_E]),
    "cpq_soft_clip_process": (C.c_int32, [_E, c_double_p, c_double_p, C.c_int32, C.c_int32]),
    "cpq_soft_clip_process_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "cpq_soft_clip_read_telemetry": (C.c_int32, [_E, C.c_int32, C.POINTER(OsTelemetry)]),
    "cpq_out_design": (C.c_int32, [C.c_double, c_double_p, c_double_p]),
    "cpq_engine_set_output_stage": (C.c_int32, [_E, C.c_int32]),
    "cpq_out_reset": (C.c_int32, [_E]),
    "cpq_out_process": (C.c_int32, [_E, c_double_p, c_double_p, C.c_int32]),
    "cpq_out_process_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32]),
    "cpq_out_read_envelope": (C.c_int32, [_E, C.c_int32, c_double_p]),
    "cpq_dither_design": (C.c_int32, [C.c_double, C.c_int32, C.c_int32, c_double_p, c_double_p]),
    "cpq_engine_set_dither": (C.c_int32, [_E, C.c_int32, C.c_int32]),
    "cpq_dither_reset": (C.c_int32, [_E]),
    "cpq_dither_set_adaptive_coeffs": (C.c_int32, [_E, C.c_int32, c_double_p, C.c_int32]),
    "cpq_dither_get_adaptive_coeffs": (C.c_int32, [_E, C.c_int32, c_double_p]),
    "cpq_dither_process": (C.c_int32, [_E, c_double_p, c_double_p, C.c_int32]),
    "cpq_dither_process_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32]),
    "cpq_pcm_bytes_per_sample": (C.c_int32, [C.c_int32]),
    "cpq_pcm_unpack": (C.c_int32, [_E, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32]),
    "cpq_pcm_unpack_device": (C.c_int32, [_E, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32]),
    "cpq_pcm_pack": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "cpq_pcm_pack_device": (C.c_int32, [_E, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "cpq_engine_process_block_pcm": (C.c_int32, [_E, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_int32]),
    "cpq_engine_process_block_pcm_device": (C.c_int32, [_E, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_int32]),
    "cpq_ir_load_wav": (C.c_int32, [C.c_char_p, C.POINTER(IrBuffer)]),
    "cpq_ir_buffer_free": (None, [C.POINTER(IrBuffer)]),
    "cpq_ir_prepare": (C.c_int32, [C.POINTER(IrBuffer), C.c_double, C.c_float, C.c_int32, C.POINTER(IrBuffer), C.c_double, C.POINTER(IrPrepared)]),
    "cpq_ir_convert_to_minimum_phase": (C.c_int32, [C.POINTER(IrBuffer), C.POINTER(IrBuffer)]),
    "cpq_ir_prepared_free": (None, [C.POINTER(IrPrepared)]),
    "cpq_ir_compute_scale_factor": (C.c_int32, [C.POINTER(c_double_p), C.c_int32, C.c_int32, C.POINTER(c_double_p), C.c_int32, C.c_int32, C.c_double, C.POINTER(IrScale)]),
    "cpq_ir_estimate_max_frequency_response_gain": (C.c_double, [C.POINTER(c_double_p), C.c_int32, C.c_int32]),
    "cpq_ir_estimate_peak_latency": (C.c_int32, [C.POINTER(c_double_p), C.c_int32, C.c_int32]),
    "cpq_resample_design": (C.c_int32, [C.c_double, C.c_double, C.POINTER(ResampleInfo), c_double_p, C.c_int32]),
    "cpq_ir_resample": (C.c_int32, [C.POINTER(IrBuffer), C.c_double, C.c_int32, C.POINTER(IrBuffer)]),
    "cpq_ir_resample_batch": (C.c_int32, [C.POINTER(C.POINTER(IrBuffer)), C.c_int32, C.c_double, C.c_int32, C.POINTER(IrBuffer)]),
    "cpq_ir_resample_host": (C.c_int32, [C.POINTER(IrBuffer), C.c_double, C.c_int32, C.POINTER(IrBuffer)]),
    "cpq_ir_resample_last_kernel_ms": (C.c_double, []),
    "cpq_src_create": (C.c_int32, [C.POINTER(SrcDesc), C.POINTER(C.c_void_p)]),
    "cpq_src_destroy": (None, [C.c_void_p]),
    "cpq_src_last_error": (C.c_char_p, [C.c_void_p]),
    "cpq_src_reset": (C.c_int32, [C.c_void_p]),
    "cpq_src_latency": (C.c_int32, [C.c_void_p]),
    "cpq_src_out_count": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32]),
    "cpq_src_max_out": (C.c_int32, [C.c_void_p]),
    "cpq_src_process": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _i32p]),
    "cpq_src_process_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _i32p]),
    "cpq_src_set_stream": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "cpq_src_last_kernel_ms": (C.c_double, [C.c_void_p]),
    "cpq_loudness_create": (C.c_int32, [C.POINTER(LoudnessDesc), C.POINTER(C.c_void_p)]),
    "cpq_loudness_destroy": (None, [C.c_void_p]),
    "cpq_loudness_last_error": (C.c_char_p, [C.c_void_p]),
    "cpq_loudness_reset": (C.c_int32, [C.c_void_p]),
    "cpq_loudness_set_stream": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "cpq_loudness_process_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "cpq_loudness_process": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "cpq_loudness_finish": (C.c_int32, [C.c_void_p, C.POINTER(LoudnessResult)]),
    "cpq_loudness_read_hops": (C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int64, _i64p]),
    "cpq_loudness_finish_host": (C.c_int32, [c_double_p, C.c_int64, C.c_double, C.POINTER(LoudnessResult)]),
    "cpq_loudness_gain": (C.c_int32, [C.POINTER(LoudnessResult), C.c_double, c_double_p]),
    "cpq_loudness_set_true_peak": (C.c_int32, [C.c_void_p, C.c_int32]),
    "cpq_loudness_read_peaks": (C.c_int32, [C.c_void_p, C.POINTER(LoudnessPeaks)]),
    "cpq_loudness_peaks_host": (C.c_int32, [c_double_p, C.c_int64, C.c_int32, C.c_int64, C.c_double, c_double_p, c_double_p]),
    "cpq_loudness_gain_limited": (C.c_int32, [C.POINTER(LoudnessResult), C.POINTER(LoudnessPeaks), C.c_double, C.c_double, c_double_p,
                                              C.POINTER(C.c_int32)]),
    "cpq_loudness_apply_device": (C.c_int32, [C.c_void_p, c_double_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32]),
    "cpq_limiter_default_window": (C.c_int32, [C.c_double]),
    "cpq_limiter_create": (C.c_int32, [C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "cpq_limiter_destroy": (None, [C.c_void_p]),
    "cpq_limiter_last_error": (C.c_char_p, [C.c_void_p]),
    "cpq_limiter_set_stream": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "cpq_limiter_reset": (C.c_int32, [C.c_void_p]),
    "cpq_limiter_latency": (C.c_int32, [C.c_void_p]),
    "cpq_limiter_window": (C.c_int32, [C.c_void_p]),
    "cpq_limiter_set_gains": (C.c_int32, [C.c_void_p, c_double_p]),
    "cpq_limiter_process_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32]),
    "cpq_limiter_process": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32]),
    "cpq_limiter_flush_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    "cpq_limiter_flush": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    "cpq_limiter_read_telemetry": (C.c_int32, [C.c_void_p, C.POINTER(LimiterTelemetry)]),
    "cpq_limiter_last_kernel_ms": (C.c_double, [C.c_void_p]),
    "cpq_quantizer_create": (C.c_int32, [C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "cpq_quantizer_destroy": (None, [C.c_void_p]),
    "cpq_quantizer_last_error": (C.c_char_p, [C.c_void_p]),
    "cpq_quantizer_set_stream": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "cpq_quantizer_reset": (C.c_int32, [C.c_void_p]),
    "cpq_quantizer_set_gains": (C.c_int32, [C.c_void_p, c_double_p]),
    "cpq_quantizer_set_adaptive_coeffs": (C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int32]),
    "cpq_quantizer_get_adaptive_coeffs": (C.c_int32, [C.c_void_p, C.c_int32, c_double_p]),
    "cpq_quantizer_process_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "cpq_quantizer_process": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "cpq_quantizer_last_kernel_ms": (C.c_double, [C.c_void_p]),
    "cpq_ir_minimum_phase_batch": (C.c_int32, [C.POINTER(C.POINTER(IrBuffer)), C.c_int32, C.c_int64, C.POINTER(IrBuffer), C.POINTER(C.c_int32)]),
    "cpq_ir_minimum_phase": (C.c_int32, [C.POINTER(IrBuffer), C.POINTER(IrBuffer)]),
    "cpq_ir_minimum_phase_last_kernel_ms": (C.c_double, []),
    "cpq_ir_prepare_batch": (C.c_int32, [C.POINTER(C.POINTER(IrBuffer)), C.c_int32, C.c_double, C.c_float, C.c_int32,
                                         C.POINTER(C.POINTER(IrBuffer)), c_double_p, C.POINTER(IrPrepared)]),
    "cpq_profile_enable": (C.c_int32, [_E, C.c_int32]),
    "cpq_profile_reset": (C.c_int32, [_E]),
    "cpq_profile_read": (C.c_int32, [_E, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "cpq_diag_partition_fft": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p]),
    "cpq_diag_partition_fft_split": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p]),
    "cpq_diag_fdl_mac": (C.c_int32, [C.c_int32] * 10 + [c_double_p, c_double_p, C.POINTER(C.c_int32), c_double_p, C.POINTER(C.c_int32)]),
    "cpq_diag_fft_forward": (C.c_int32, [C.c_int32] * 6 + [c_double_p, c_double_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64), C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                         C.POINTER(C.c_int64), c_double_p]),
    "cpq_diag_fft_inverse_store": (C.c_int32, [C.c_int32] * 4 + [c_double_p, c_double_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64, c_double_p,
                                               C.c_int32, C.POINTER(C.c_int64), c_double_p, c_double_p, C.c_int32, C.POINTER(C.c_int64),
                                               C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_double, C.c_double, c_double_p]),
    "cpq_diag_ir_spectra": (C.c_int32, [C.c_int32, C.c_int32, c_double_p, C.c_int32, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "cpq_diag_direct_head": (C.c_int32, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, c_double_p, c_double_p, _i32p, _i32p, c_double_p, _i32p,
                                         c_double_p, c_double_p, c_double_p, C.c_int64]),
    "cpq_diag_agc": (C.c_int32, [C.c_int32] * 4 + [C.c_int64, c_double_p, c_double_p, c_double_p, c_double_p, _i32p, c_double_p, C.c_double,
                                                   C.c_double, C.c_double, c_double_p, _i32p]),
    "cpq_diag_ring_chunks": (C.c_int32, [C.c_int32] * 5 + [C.c_int64, c_double_p, _i32p, c_double_p, C.c_int32, _i64p, _i64p, c_double_p,
                                                           C.c_int32, _i64p, C.c_double, c_double_p, C.c_int32, _i64p, C.c_double,
                                                           C.c_int32, _i64p, _i64p, c_double_p, c_double_p, c_double_p, _i64p, C.c_int32,
                                                           _i64p]),
    "cpq_diag_convproc_mix": (C.c_int32, [C.c_int32, C.c_int32, C.c_int64, c_double_p, c_double_p, C.c_int32, c_double_p, c_double_p,
                                          C.c_int32, C.c_int64, _i32p, _i32p, _i32p, c_double_p, C.c_int32, C.c_int32, _i32p, c_double_p,
                                          C.c_int32, C.c_int32, _i32p, c_double_p, C.c_int32, C.c_int64, c_double_p, C.c_int64, C.c_int32]),
    "cpq_diag_tail_reader": (C.c_int32, [C.c_int32, _i32p] + [C.c_int32] * 8 + [_i64p, _i64p, _i64p, C.c_int32, C.c_int32, c_double_p,
                                                                               c_double_p, C.c_int32]),
    "cpq_diag_rows": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, c_double_p, C.c_int64, C.c_int64, c_double_p, C.c_int64, C.c_int64,
                                  c_double_p, _i32p, _i32p, c_double_p, c_double_p, C.c_int32]),
    "cpq_diag_cfft": (C.c_int32, [c_double_p, C.c_int32, C.c_int32, C.c_int32, c_double_p]),
    "cpq_diag_eq_chain_status": (C.c_int32, [_E, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "cpq_kernel_name": (C.c_char_p, [C.c_int32]),
    "cpq_scorer_create": (C.c_int32, [C.POINTER(ScorerDesc), C.POINTER(C.c_void_p)]),
    "cpq_scorer_destroy": (None, [C.c_void_p]),
    "cpq_scorer_last_error": (C.c_char_p, [C.c_void_p]),
    "cpq_scorer_set_audio": (C.c_int32, [C.c_void_p, C.c_int32, c_double_p, c_double_p, C.c_int32, _i32p]),
    "cpq_scorer_set_audio_device": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, _i32p]),
    "cpq_scorer_get_segments": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(ScoreSegment), _i32p, _i32p]),
    "cpq_scorer_read_thresholds": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_double_p]),
    "cpq_scorer_score": (C.c_int32, [C.c_void_p, c_double_p, C.c_int32, c_double_p, C.POINTER(ScoreParts)]),
    "cpq_scorer_score_raw": (C.c_int32, [C.c_void_p, c_double_p, C.c_int32, c_double_p, C.POINTER(ScoreParts)]),
    "cpq_scorer_set_rng_start": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cpq_scorer_read_error": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p]),
    "cpq_scorer_last_timing": (C.c_int32, [C.c_void_p, c_double_p, c_double_p]),
    "cpq_score_design": (C.c_int32, [C.c_double, c_double_p, c_double_p, c_double_p, c_double_p, _i32p, _i32p, _i32p, c_double_p]),
    "cpq_score_select_segments": (C.c_int32, [c_double_p, c_double_p, C.c_int32, C.POINTER(ScoreSegment), _i32p, _i32p]),
    "cpq_diag_score_spectrum": (C.c_int32, [C.c_double, C.c_int32, c_double_p, C.c_int32, c_double_p, C.c_int32, C.POINTER(DiagScoreEval),
                                            C.c_int32, C.c_int32, C.POINTER(ScoreParts), c_double_p]),
    "cpq_diag_score_lattice": (C.c_int32, [C.c_int32, C.c_int32, c_double_p, C.c_int32, c_double_p, C.c_int32, C.POINTER(DiagScoreChain),
                                           C.c_int32, c_double_p, C.c_int32, C.POINTER(C.c_uint64)]),
    "cpq_diag_score_reduce": (C.c_int32, [C.c_int32, C.c_int32, _i32p, _i32p, c_double_p, c_double_p, c_double_p]),
    "cpq_learner_create": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "cpq_learner_destroy": (None, [C.c_void_p]),
    "cpq_learner_last_error": (C.c_char_p, [C.c_void_p]),
    "cpq_learner_init": (C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_uint64]),
    "cpq_learner_set_params": (C.c_int32, [C.c_void_p, C.POINTER(LearnParams)]),
    "cpq_learner_run": (C.c_int32, [C.c_void_p, C.c_int32]),
    "cpq_learner_get_state": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(LearnState)]),
    "cpq_learner_set_state": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(LearnState)]),
    "cpq_learner_read_generation": (C.c_int32, [C.c_void_p, C.c_int32, c_double_p, c_double_p, c_double_p, c_double_p, _i32p]),
    "cpq_learner_read_history": (C.c_int32, [C.c_void_p, C.c_int32, c_double_p, _i32p]),
    "cpq_learner_published": (C.c_int32, [C.c_void_p, C.c_int32, c_double_p]),
    "cpq_learner_last_timing": (C.c_int32, [C.c_void_p, c_double_p, c_double_p]),
    "cpq_learn_init_host": (C.c_int32, [c_double_p, C.c_uint64, C.POINTER(LearnParams), C.POINTER(LearnState)]),
    "cpq_learn_normals_host": (C.c_int32, [C.POINTER(LearnState), c_double_p, _i32p]),
    "cpq_learn_ask_host": (C.c_int32, [C.POINTER(LearnState), c_double_p, c_double_p]),
    "cpq_learn_tell_host": (C.c_int32, [C.POINTER(LearnState), C.POINTER(LearnParams), c_double_p, c_double_p, c_double_p, _i32p]),
    "cpq_learn_phase": (C.c_int32, [C.c_int32, C.c_double]),
    "cpq_learn_phase_params": (C.c_int32, [C.c_int32, C.c_int32, C.POINTER(LearnParams), c_double_p]),
    "cpq_diag_learn_tell": (C.c_int32, [C.c_int32, C.POINTER(LearnState), C.POINTER(LearnParams), c_double_p, c_double_p, c_double_p]),
    "cpq_diag_prog_finish": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_double, c_double_p, C.POINTER(LoudnessResult), c_double_p, _i32p]),
}

_lib = None


def _share_hip_runtime_with_torch():
    """One process, one HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as the system one
    this library links).  If this library is loaded first it pulls in /opt/rocm's copy, a later `import torch` maps the
    bundled copy as a second runtime, and torch.cuda then reports "No HIP GPUs are available".  When a torch installation
    is present (found WITHOUT importing it) its runtime is mapped first, so both sides resolve libamdhip64.so.7 to the
    same object whatever the import order.  No torch: nothing happens and the system runtime is used."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    for root in spec.submodule_search_locations:
        cand = os.path.join(root, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


def load():
    """Load the shared library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C convopeq_amd/csrc` (or __graft_entry__.build()). "
            "convopeq_amd has no CPU fallback.")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)        # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
