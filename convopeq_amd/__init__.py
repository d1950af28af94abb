"""convopeq_amd -- MI355X-native (gfx950) batched drop-in for ConvoPeq's convolver + 20-band EQ hot path.

The product is convopeq_amd/libconvopeq_mi355x.so (hand-written HIP kernels behind the C ABI in
include/convopeq_mi355x.h).  Importing this package loads that library and fails loudly if it is missing.
"""
from . import _capi
from ._capi import (CPQ_DITHER_OFF, CPQ_DITHER_FIXED4, CPQ_DITHER_FIXED15, CPQ_DITHER_ADAPTIVE9, CPQ_DITHER_TILE, CPQ_OUT_ALL, CPQ_OUT_CLAMP, CPQ_OUT_DC_BLOCK, CPQ_OUT_HEADROOM, CPQ_OUT_LIMITER, CPQ_METER_LOUDNESS, CPQ_METER_TRUE_PEAK, CPQ_ALL_STREAMS, CPQ_EQ_MODE_AUTO, CPQ_EQ_MODE_SEQUENTIAL, CPQ_LEVEL_NUC, CPQ_LEVEL_PROCESSOR, CPQ_ORDER_CONV_THEN_EQ, CPQ_ORDER_EQ_THEN_CONV, CPQ_SCHED_REFERENCE_NUC, CPQ_SCHED_UNIFORM, CPQ_SEM_EXACT, CPQ_CALLS_ANY, CPQ_CALLS_WHOLE_BLOCKS, CPQ_PARTITION_AUTO,
                    CPQ_SEM_REFERENCE, CPQ_OS_IIR, CPQ_OS_LINEAR_PHASE, EqParams, FilterSpec, NucPlan, SvfCoeffs)
from .engine import (BatchedEngine, CpqError, design_svf, eq_params_default, ir_compute_scale_factor, ir_convert_to_minimum_phase,
                     ir_estimate_max_frequency_response_gain, ir_estimate_peak_latency, ir_load_wav, ir_prepare, nuc_heff,
                     nuc_plan, os_design_stage, os_latency, os_resolve_factor, outfilter_design, meter_kweighting,
                     meter_tp_design_stage, out_design, dither_design, ir_resample, ir_resample_batch, resample_design,
                     ir_minimum_phase, ir_minimum_phase_batch, ir_prepare_batch, soft_clip_params, soft_clip_host,
                     soft_clip_latency)
from ._capi import CPQ_SCORE_RNG_CHAINED, CPQ_SCORE_RNG_FRESH, CPQ_SCORE_UNSTABLE
from .scorer import ShaperScorer, score_design, select_segments
from .learner import ShaperLearner
from .resampler import StreamResampler
from .loudness import ProgrammeLoudness, loudness_finish_host, loudness_peaks_host
from .limiter import TruePeakLimiter, limiter_default_window
from .quantizer import Quantizer

_capi.load()   # no fallback: ImportError if the HIP library is absent

__all__ = ["Quantizer", "TruePeakLimiter", "limiter_default_window", "soft_clip_params", "soft_clip_host", "soft_clip_latency", "ShaperLearner", "ProgrammeLoudness", "loudness_finish_host", "loudness_peaks_host", "StreamResampler", "ir_minimum_phase", "ir_minimum_phase_batch", "ir_prepare_batch", "ir_resample", "ir_resample_batch", "resample_design", "ShaperScorer", "score_design", "select_segments", "CPQ_SCORE_RNG_FRESH", "CPQ_SCORE_RNG_CHAINED", "CPQ_SCORE_UNSTABLE", "BatchedEngine", "CpqError", "design_svf", "eq_params_default", "nuc_heff", "nuc_plan", "outfilter_design", "ir_load_wav", "ir_prepare", "ir_compute_scale_factor", "ir_convert_to_minimum_phase",
           "ir_estimate_max_frequency_response_gain", "ir_estimate_peak_latency", "os_design_stage", "os_latency", "os_resolve_factor", "meter_kweighting", "meter_tp_design_stage",
           "CPQ_METER_LOUDNESS", "CPQ_METER_TRUE_PEAK", "out_design", "dither_design",
           "CPQ_DITHER_OFF", "CPQ_DITHER_FIXED4", "CPQ_DITHER_FIXED15", "CPQ_DITHER_ADAPTIVE9", "CPQ_DITHER_TILE",
           "CPQ_OUT_DC_BLOCK", "CPQ_OUT_HEADROOM", "CPQ_OUT_LIMITER", "CPQ_OUT_CLAMP", "CPQ_OUT_ALL",
           "EqParams", "FilterSpec", "NucPlan", "SvfCoeffs", "CPQ_ALL_STREAMS", "CPQ_SEM_REFERENCE",
           "CPQ_SEM_EXACT", "CPQ_CALLS_ANY", "CPQ_CALLS_WHOLE_BLOCKS", "CPQ_PARTITION_AUTO", "CPQ_SCHED_UNIFORM", "CPQ_SCHED_REFERENCE_NUC", "CPQ_ORDER_CONV_THEN_EQ", "CPQ_ORDER_EQ_THEN_CONV", "CPQ_EQ_MODE_AUTO",
           "CPQ_EQ_MODE_SEQUENTIAL", "CPQ_LEVEL_NUC", "CPQ_LEVEL_PROCESSOR", "CPQ_OS_IIR", "CPQ_OS_LINEAR_PHASE"]
