/*
 * convopeq_mi355x.h -- C ABI of libconvopeq_mi355x.so
 *
 * MI355X-native (gfx950) batched drop-in for ONE hot path of lonewolf-jp/ConvoPeq:
 * the fp64 impulse-response convolver plus the 20-band TPT-SVF parametric EQ,
 * batched over S independent stereo streams (channel c = 2*stream + {0:L,1:R}).
 *
 * Boundary: this header is what the reference's FFI for the path would bind.
 * Each entry point cites the reference interface it replaces (paths relative to
 * the reference tree).  Plain pointers and sizes only; no C++/torch types; no
 * exceptions cross the ABI; every call returns a cpq_status (0 = ok, <0 = error)
 * unless noted.  One host thread per engine handle; handles are independent
 * (one per GPU / per process).
 *
 * PCM layout: planar [stream][channel][sample] fp64, i.e. channel c starts at
 * c * nSamples doubles.  The *_device entry points take device (HBM) pointers
 * and enqueue on the engine's stream without synchronising; the host-pointer
 * twins stage through the engine's device arena and return when the result is
 * in host memory.
 */
#ifndef CONVOPEQ_MI355X_H
#define CONVOPEQ_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPQ_ABI_VERSION 2
/* additions that leave every earlier entry point as it was count here: 1 = the packed PCM entry points */
#define CPQ_ABI_REVISION 1
/* later additions announce themselves at compile time: defined when the output stage entry points
 * (cpq_engine_set_output_stage, cpq_out_*) exist.  cpq_abi_revision() does not count them, so at run time a caller that may
 * meet an older library finds out by looking the symbol up (dlsym) */
#define CPQ_HAS_OUTPUT_STAGE 1
/* likewise: defined when the dither stage (cpq_engine_set_dither, cpq_dither_*) and 16-bit PCM output exist */
#define CPQ_HAS_DITHER 1
/* likewise: defined when the adaptive 9th-order lattice shaper (CPQ_DITHER_ADAPTIVE9, cpq_dither_*_adaptive_coeffs) exists */
#define CPQ_HAS_ADAPTIVE_DITHER 1
/* likewise: defined when the soft clipper (cpq_engine_set_soft_clip, cpq_soft_clip_*) exists */
#define CPQ_HAS_SOFT_CLIP 1

typedef enum {
    CPQ_OK               =  0,
    CPQ_ERR_INVALID_ARG  = -1,
    CPQ_ERR_NO_DEVICE    = -2,   /* no gfx950 device / HIP runtime failure at create */
    CPQ_ERR_OOM          = -3,
    CPQ_ERR_DEVICE       = -4,   /* a HIP call failed; see cpq_last_error() */
    CPQ_ERR_UNSUPPORTED  = -5,   /* valid in the reference, not implemented by this engine yet */
    CPQ_ERR_NOT_READY    = -6,   /* process before set_impulse / prepare */
    CPQ_ERR_SILENT_IR    = -7    /* cpq_ir_resample*: the IR's peak is below 1e-12 (the reference's ResampleResult::SilentIR) */
} cpq_status;

#define CPQ_ALL_STREAMS (-1)
#define CPQ_NUM_BANDS   20       /* EQProcessor::NUM_BANDS, src/eqprocessor/EQProcessor.h:153 */

/* what "the convolution" means for IRs longer than the reference's layer 0 */
typedef enum {
    /* y = x * h_eff: the closed form of MKLNonUniformConvolver's observable output (tail-layer
     * contouring gains and the constant layer lags of the distributed-MAC schedule and the B13 delay
     * line, src/MKLNonUniformConvolver.cpp:626-684,988-994,1497-1545,1653-1688).
     * Valid iff the reference itself is LTI for the configuration (cpq_nuc_plan.lti_valid). */
    CPQ_SEM_REFERENCE = 0,
    /* y = x * h: the mathematically exact linear convolution (== reference whenever irLen <= layer 0) */
    CPQ_SEM_EXACT = 1
} cpq_semantics;

typedef enum { CPQ_ORDER_CONV_THEN_EQ = 0, CPQ_ORDER_EQ_THEN_CONV = 1 } cpq_order;

/* how the IR is partitioned on the GPU (reference semantics only) */
typedef enum {
    /* one partition size for the whole h_eff (block_size or partition_size): every FDL / IR row is streamed by one
     * MAC kernel -- the HBM-roofline path of BASELINE.json configs[1] */
    CPQ_SCHED_UNIFORM = 0,
    /* the reference's own non-uniform (Gardner) schedule: layer 0 at block_size, tail layers at block_size * m and
     * block_size * m^2 (src/MKLNonUniformConvolver.cpp:738-758), each on its own FFT grid, outputs merged through
     * the replayed delay-line reader.  ~K0 + K1/m + K2/m^2 partition MACs per block instead of irLen / block_size
     * (BASELINE.json configs[3]).  Every IR of the engine must have the same layer plan. */
    CPQ_SCHED_REFERENCE_NUC = 1
} cpq_schedule;

/* which call sizes the process entry points accept */
typedef enum {
    /* n_samples = T * block_size with block_size a power of two (64..4096): every B-sample quantum is one Add + Get
     * pair of the reference with a full layer-0 partition, the regime in which its output is one linear convolution
     * (h_eff) and the time-batched uniform schedule applies -- the throughput path */
    CPQ_CALLS_WHOLE_BLOCKS = 0,
    /* any block_size from 1 to 4096 (the reference's blockSize / callQuantum: 480, 441, 96 ...) and any n_samples >= 1.
     * The call is cut into chunks of block_size samples (the last one may be shorter), each chunk is one Add(chunk) +
     * Get(chunk) of every MKLNonUniformConvolver (StereoConvolver::process, src/convolver/ConvolverProcessor.Runtime.cpp:
     * 1159-1184; chunking :659-682): input accumulates per layer until a partition of nextPow2(max(block_size, 64)) *
     * {1, m, m^2} samples is full (src/MKLNonUniformConvolver.cpp:1431-1446), layer 0 goes through the output ring and a
     * short read is zero-filled at the END of the chunk (:1376-1402), the tail layers follow the distributed MAC's
     * completion schedule and the delay-line reader per chunk (:1497-1545, :1653-1688) -- including the reference's
     * start-up gaps and dropped tail blocks at awkward quanta.  Every stream runs on the reference's own layer plan. */
    CPQ_CALLS_ANY = 1
} cpq_call_mode;

/* POD mirror of convo::FilterSpec, src/MKLNonUniformConvolver.h:123-133 */
typedef struct {
    double  sample_rate;
    int32_t hc_mode;                 /* HCMode: 0 Sharp, 1 Natural, 2 Soft (src/OutputFilter.h:75-80) */
    int32_t lc_mode;                 /* LCMode: 0 Natural, 1 Soft         (src/OutputFilter.h:85-89) */
    int32_t tail_mode;               /* 0 air absorption, 1 layer tail contouring, 2 bypass */
    int32_t tail_enabled;
    double  tail_start_seconds;
    double  tail_strength;
    int32_t tail_l1l2_multiplier;
    int32_t reserved;
} cpq_filter_spec;

/* The layer plan SetImpulse derives (src/MKLNonUniformConvolver.cpp:738-758,784-786,988-994,
 * 1005-1024) plus the A6 closed-form lags.  Host-only computation, no GPU needed. */
typedef struct {
    int32_t num_layers;
    int32_t part_size[3];
    int32_t offset[3];
    int32_t len[3];
    int32_t num_parts_ir[3];
    int32_t num_parts[3];
    int32_t parts_per_callback[3];
    int32_t output_delay[3];
    double  gain[3];
    int32_t direct_taps;
    int32_t latency;                 /* MKLNonUniformConvolver::getLatency(), src/MKLNonUniformConvolver.h:242 */
    int32_t lti_valid;
    int32_t done_callback[3];
    int32_t lag[3];
    int32_t heff_len;                /* taps of h_eff */
} cpq_nuc_plan;

/* POD mirror of EQCoeffsSVF, src/eqprocessor/EQProcessor.h:91-96 */
typedef struct { double g, k, a1, a2, a3, m0, m1, m2; } cpq_svf_coeffs;

/* POD mirror of convo::EQBandParams / convo::EQParameters, src/core/EQParameters.h:13-47 */
typedef struct {
    float   frequency;
    float   gain;
    float   q;
    int32_t enabled;
    int32_t type;                    /* 0 LowShelf, 1 Peaking, 2 HighShelf, 3 LowPass, 4 HighPass */
    int32_t channel_mode;            /* 0 Stereo, 1 Left, 2 Right, 3 Mid, 4 Side (Mid/Side: basic process(block) path) */
} cpq_eq_band;

typedef struct {
    cpq_eq_band bands[CPQ_NUM_BANDS];
    float   total_gain_db;
    int32_t agc_enabled;             /* block-rate AGC (processAGC): replaces the total-gain stage */
    float   nonlinear_saturation;    /* default 0.2 */
    int32_t filter_structure;        /* 0 Serial, 1 Parallel (parallel runs on the lane-skewed kernel) */
} cpq_eq_params;

typedef struct {
    int32_t struct_size;             /* sizeof(cpq_engine_desc) */
    int32_t device;                  /* HIP device ordinal */
    int32_t n_streams;               /* S stereo streams -> 2*S channels */
    int32_t block_size;              /* B: the caller's block / callQuantum.  CPQ_CALLS_WHOLE_BLOCKS: a power of two,
                                        64..4096, partition size P == B (layer-0 partSize of the reference);
                                        CPQ_CALLS_ANY: 1..4096, layer-0 partition nextPow2(max(B, 64)).  512 has
                                        dedicated wave-level FFT kernels, other sizes use generic ones */
    int32_t max_ir_len;              /* longest IR (taps) any stream will be given */
    int32_t max_blocks_per_call;     /* T_max: a process call carries 1..T_max blocks of B samples (CPQ_CALLS_ANY:
                                        1..T_max * B samples)
                                        (reference: up to 524288 samples per process(),
                                        src/convolver/ConvolverProcessor.Runtime.cpp:609,667-682) */
    int32_t semantics;               /* cpq_semantics */
    int32_t mac_tile;                /* 0 = default; else outputs per lane in the FDL MAC kernel (4/8/16/32) */
    double  sample_rate;
    int32_t partition_size;          /* internal FFT partition P: 0 = block_size; CPQ_PARTITION_AUTO = the fastest P
                                        for calls of max_blocks_per_call blocks (4096 when block_size *
                                        max_blocks_per_call is a multiple of it and at least 32768, else 512 when
                                        a multiple of that, else block_size;
                                        uniform schedule, whole-block calls, plain IRs - a FilterSpec with tail
                                        layers needs P == block_size;
                                        read it back with cpq_engine_partition_size); else a power of two with
                                        block_size <= P <= 4096.  The result is the same convolution (with the
                                        h_eff the reference derives for block_size); larger P trades call
                                        granularity for fewer partitions: every call must then carry a multiple
                                        of P samples (offline / batched use).  The reference itself runs its tail
                                        layers at 8x and 64x the block size (src/MKLNonUniformConvolver.cpp:738-740). */
    int32_t schedule;                /* cpq_schedule (was reserved: 0 = uniform) */
    int32_t call_mode;               /* cpq_call_mode: 0 = whole power-of-two blocks (default), 1 = any quantum / ragged calls */
    int32_t reserved;
} cpq_engine_desc;

#define CPQ_PARTITION_AUTO (-1)

typedef struct cpq_engine cpq_engine;

/* ------------------------------------------------------------------ library */
int32_t     cpq_abi_version(void);
int32_t     cpq_abi_revision(void);
const char* cpq_status_string(int32_t status);
/* last error text of this handle (or of the last failed create when e == NULL) */
const char* cpq_last_error(const cpq_engine* e);

/* ------------------------------------------------- host-only design helpers */
/* MKLNonUniformConvolver::SetImpulse layer plan (src/MKLNonUniformConvolver.cpp:626-684,738-758).
 * spec may be NULL (reference default: tail mode 1, start 0.085 s, strength 1, multiplier 8). */
int32_t cpq_nuc_plan_compute(int32_t ir_len, int32_t block_size, int32_t enable_direct_head,
                             const cpq_filter_spec* spec, cpq_nuc_plan* plan);
/* h_eff for one mono IR; writes min(cap, plan.heff_len) taps, returns heff_len or <0. */
int32_t cpq_nuc_heff(const double* ir, int32_t ir_len, int32_t block_size, double scale,
                     const cpq_filter_spec* spec, double* heff, int32_t cap);
/* EQProcessor::calcSVFCoeffs (src/eqprocessor/EQProcessor.Coefficients.cpp:101-130,431-618) */
int32_t cpq_eq_design_svf(int32_t type, float freq, float gain_db, float q, double sample_rate,
                          cpq_svf_coeffs* out);
/* convo::EQParameters::EQParameters() defaults (src/core/EQParameters.h:31-46) */
void    cpq_eq_params_default(cpq_eq_params* p);

/* ------------------------------------------------------------------- engine */
/* replaces: construction of StereoConvolver + 2 MKLNonUniformConvolver + EQProcessor per stream
 * and every per-buffer aligned allocation under them (src/AlignedAllocation.h:22-163,
 * src/MKLNonUniformConvolver.h:288-365): one device arena sized from the descriptor. */
int32_t cpq_engine_create(const cpq_engine_desc* desc, cpq_engine** out);
void    cpq_engine_destroy(cpq_engine* e);
/* hipStream_t the engine enqueues on (NULL = default stream). */
int32_t cpq_engine_set_stream(cpq_engine* e, void* hip_stream);
int32_t cpq_engine_synchronize(cpq_engine* e);
/* bytes of the device arena */
int64_t cpq_engine_arena_bytes(const cpq_engine* e);
/* the internal FFT partition size in use (what CPQ_PARTITION_AUTO resolved to); calls carry multiples of it */
int32_t cpq_engine_partition_size(const cpq_engine* e);

/* replaces ConvolverProcessor::prepareToPlay(double,int) (src/convolver/ConvolverProcessor.Lifecycle.cpp:211-402)
 * and EQProcessor::prepareToPlay(double,int) (src/eqprocessor/EQProcessor.Core.cpp:679-826):
 * publishes the rate, zeroes all run-time state (FDL, overlap history, SVF state) and, when the rate changed, re-designs
 * the EQ and OutputFilter coefficients from the parameters set so far (the reference rebuilds its band nodes on a rate
 * change).  The smoothers take their present targets at once (mix, total gain, EQ bypass fade, latency), pending band /
 * AGC reset requests are dropped with the state they would have cleared.  IR spectra are not touched: an IR belongs to
 * a rate, load it again if needed.  max_block must not exceed block_size * max_blocks_per_call. */
int32_t cpq_engine_prepare(cpq_engine* e, double sample_rate, int32_t max_block);
int32_t cpq_engine_set_order(cpq_engine* e, int32_t order);
/* Pin / unpin a caller buffer that is passed to the host-pointer entry points (cpq_*_process, cpq_engine_process_block):
 * those calls pipeline upload, kernels and download over time chunks, which overlaps fully only for pinned memory. */
int32_t cpq_host_register(void* ptr, size_t bytes);
int32_t cpq_host_unregister(void* ptr);

/* ---------------------------------------------------------------- convolver */
/* replaces StereoConvolver::init (src/ConvolverProcessor.h:741-814) -> 2 x
 * MKLNonUniformConvolver::SetImpulse(impulse, irLen, blockSize, scale, enableDirectHead, filterSpec)
 * (src/MKLNonUniformConvolver.h:197-200).  stream = index or CPQ_ALL_STREAMS (one shared stereo IR).
 * The caller keeps ownership of ir_l/ir_r (copied).
 * On a stream that is already playing the call leaves, like SetImpulse, a convolver that has seen no input (its input
 * history -- delay-line spectra, overlap block, the direct head's last samples -- is cleared); the other streams play on.
 * spec: NULL (the primary parity surface), or a FilterSpec: its HC/LC spectral gains (:336-443) and, in tail mode 0,
 * the air-absorption damping (:1060-1097) are applied to every partition spectrum at that LAYER's FFT size, exactly
 * as the reference does.  Layer 0 runs in the main path; every tail layer of the plan runs on the reference's own
 * partition grid (block_size * multiplier, ...) and reaches the output through the delay-line lag done_callback * B.
 * Tail partitions up to 131072 samples are supported (above 4096 through a four-step FFT); plans that are time-varying
 * in the reference (cpq_nuc_plan.lti_valid == 0) follow the replayed delay-line reader.
 * Limits (CPQ_ERR_UNSUPPORTED): tail partitions that are not a power of two or exceed 131072 (no plan of the reference does), FilterSpec IRs with
 * different layer plans in one engine, partition_size != block_size.
 * enable_direct_head: the first min(ir_len, 32) taps leave the FFT path before the spectra (and any FilterSpec gains)
 * are formed and run as a time-domain FIR over [history | block], flushed below 1e-20, added before the tail layers
 * (src/MKLNonUniformConvolver.cpp:689-731, 1169-1232, 1606-1618). */
int32_t cpq_conv_set_impulse(cpq_engine* e, int32_t stream, const double* ir_l, const double* ir_r,
                             int32_t ir_len, double scale, int32_t enable_direct_head,
                             const cpq_filter_spec* spec);
/* replaces the per-quantum MKLNonUniformConvolver::Add + Get pair (src/MKLNonUniformConvolver.h:208,218;
 * call site StereoConvolver::process, src/convolver/ConvolverProcessor.Runtime.cpp:1159-1184) for every
 * channel of every stream and every B-sample quantum in the call.  n_samples = T*B, 1 <= T <= T_max.
 * in == out is allowed. */
int32_t cpq_conv_process(cpq_engine* e, const double* in, double* out, int32_t n_samples);
int32_t cpq_conv_process_device(cpq_engine* e, const double* d_in, double* d_out, int32_t n_samples);
/* MKLNonUniformConvolver::Reset (src/MKLNonUniformConvolver.h:224) for all channels */
int32_t cpq_conv_reset(cpq_engine* e);
/* MKLNonUniformConvolver::isReady / getLatency (src/MKLNonUniformConvolver.h:229,242) */
int32_t cpq_conv_is_ready(const cpq_engine* e);
int32_t cpq_conv_latency(const cpq_engine* e);
int32_t cpq_conv_get_plan(const cpq_engine* e, cpq_nuc_plan* plan);
/* the return value of Get (src/MKLNonUniformConvolver.cpp:1553-1634) for the last process call of one stream: samples
 * layer 0's output ring delivered, summed over the call's chunks (n_samples unless the ring ran short: start-up, awkward
 * quanta -- the missing samples are zero-filled in the output as ringRead does).  Main-path streams always deliver
 * every sample.  < 0: bad argument. */
int32_t cpq_conv_last_got(const cpq_engine* e, int32_t stream);

/* ------------------------------------------- convolver, processor level (N1) */
/* Restatement of ConvolverProcessor::process(AudioBlock<double>&), steady state and the transitions of a live stream,
 * (src/convolver/ConvolverProcessor.Runtime.cpp:209-810) around the kernel-level convolver:
 *   dry signal through a delay line of (algorithmLatency + irPeakLatency) samples (:266-288, :549-567),
 *   wet = convolver output with NaN / Inf / |x| >= 1e300 replaced by 0 (:50-60, :722),
 *   out = wet * wetG + dry * dryG, wetG = equalPowerSin(mix) * CONVOLUTION_HEADROOM_GAIN (= 1.0),
 *   dryG = mix < 0.999 ? equalPowerSin(1 - mix) : 0, equalPowerSin = the 9th-order Taylor form (:26-31),
 *   so mix = 1 scales the wet signal by 1.0000035... (:373-375, :675-676, :611-657);
 *   mix <= 0.001: dry only, the convolver is not run (:573-585); bypassed: pure delay, convolver not run (:123-186).
 * A mix change after the first processor-level call is smoothed like the reference's mixSmoother (LinearRamp over
 * smoothing_time_sec, per-sample gains equalPowerSin(mix_i) / equalPowerSin(1 - mix_i) for every callback that starts
 * while the ramp runs, :340-375, :591-607); before it (and after cpq_engine_prepare) the mix applies at once, as
 * prepareToPlay sets it.  The latency compensation follows :263-290 and :394-540: the dry delay line is a ring that
 *   remembers B + max_ir_len samples (more when a larger ir_peak_latency is set); a total latency that moves by >= 2
 *   samples on a live stream is cross-faded over 20 ms from the delay in use (a move of one sample is not followed, as in
 *   the reference), a move during a running fade waits for its end; processing starts from latency + irLatency
 *   (Lifecycle.cpp:377-388), so with the direct head the first 20 ms fade from B + ir_peak_latency to ir_peak_latency.
 *   The reader's Catmull-Rom branch needs a fractional delay, which nothing in the reference produces: not built.
 * mix / ir_peak_latency may differ per stream; bypassed and mix <= 0.001 must be set for CPQ_ALL_STREAMS. */
typedef struct {
    float   mix;                 /* 0..1, default 1 (src/ConvolverProcessor.h:950) */
    int32_t bypassed;
    int32_t ir_peak_latency;     /* StereoConvolver::irLatency (peak delay of the loaded IR), samples */
    float   smoothing_time_sec;  /* mix ramp length; 0 = default 0.1 s (SMOOTHING_TIME_DEFAULT_SEC), else 0.01 .. 0.5 */
} cpq_convproc_params;
int32_t cpq_convproc_set_params(cpq_engine* e, int32_t stream, const cpq_convproc_params* p);
int32_t cpq_convproc_process(cpq_engine* e, const double* in, double* out, int32_t n_samples);
int32_t cpq_convproc_process_device(cpq_engine* e, const double* d_in, double* d_out, int32_t n_samples);
/* total dry-path delay in samples of one stream (algorithmLatency + irPeakLatency) */
int32_t cpq_convproc_delay(const cpq_engine* e, int32_t stream);
/* CPQ_LEVEL_NUC (default): cpq_engine_process_block uses the kernel-level convolver (primary parity surface);
 * CPQ_LEVEL_PROCESSOR: it uses cpq_convproc_process, as DSPCore does with ConvolverProcessor::process. */
typedef enum { CPQ_LEVEL_NUC = 0, CPQ_LEVEL_PROCESSOR = 1 } cpq_conv_level;
int32_t cpq_engine_set_conv_level(cpq_engine* e, int32_t level);

/* ----------------------------------------------------------------------- EQ */
/* replaces EQProcessor::createCoeffCache(params, sr, maxBlock, gen) (src/eqprocessor/
 * EQProcessor.ProcessingCache.cpp:56-93) + the (EQParameters, EQCoeffCache*) arguments of process(). */
int32_t cpq_eq_set_params(cpq_engine* e, int32_t stream, const cpq_eq_params* params);
/* replaces EQProcessor::process(AudioBlock<double>&, const EQParameters&, const EQCoeffCache*)
 * (src/eqprocessor/EQProcessor.Processing.cpp:1019-1276), serial structure, steady total gain. */
int32_t cpq_eq_process(cpq_engine* e, const double* in, double* out, int32_t n_samples);
int32_t cpq_eq_process_device(cpq_engine* e, const double* d_in, double* d_out, int32_t n_samples);
/* replaces EQProcessor::setBypassFromRT(bool) as DSPCore calls it before every block
 * (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:384; src/eqprocessor/EQProcessor.Processing.cpp:499-526,
 * 977-1015), per stream.  After the first processed call a change runs the reference's 5 ms bypass fade
 * (BYPASS_FADE_TIME_SEC): the callbacks that start while it runs go through the basic process(block) -- whose band nodes
 * leave flat non-LP/HP bands out -- and are cross-faded with the dry block per sample; once faded out the EQ of the
 * stream does nothing (filter states, total-gain ramp and AGC frozen); releasing the bypass clears the stream's filter
 * states and fades back in.  Before the first call (and at prepare / reset) the state follows the request at once. */
int32_t cpq_eq_set_bypass(cpq_engine* e, int32_t stream, int32_t bypassed);
/* replaces EQProcessor::requestBandReset (src/eqprocessor/EQProcessor.h; consumed in process(),
 * src/eqprocessor/EQProcessor.Processing.cpp:1083-1112 / :595-624): the filter states of the bands in band_mask (bit b =
 * band b; 0xFFFFFFFF = all, Mid / Side states included) are cleared at the start of the first callback whose input
 * block is silent (no sample above 1e-8, isAudioBlockSilent :460-475) or that runs a bypass fade; until then the request
 * stays pending.  While a request is pending on a playing stream each EQ call synchronises the engine's stream once
 * (the silence flags are read back); without a pending request nothing changes. */
int32_t cpq_eq_request_band_reset(cpq_engine* e, int32_t stream, uint32_t band_mask);
/* replaces EQProcessor::requestAgcReset (src/eqprocessor/EQProcessor.h:538-541): at the stream's next processed block the AGC
 * envelopes return to 0 and its gain to 1 (src/eqprocessor/EQProcessor.Processing.cpp:586-593, 1070-1077). */
int32_t cpq_eq_request_agc_reset(cpq_engine* e, int32_t stream);
/* EQ kernel choice.  AUTO: time-parallel kernel (per band: zero-state chunk runs + state scan; equal to the
 * sequential recurrence up to rounding, measured <= 3e-15) whenever the host can prove the reference's state
 * guards cannot trip, else the sequential kernel.  SEQUENTIAL: lane-skewed kernel that reproduces the
 * reference recurrence operation for operation (bit-identical to the SSE2+FMA path given equal coefficients). */
typedef enum { CPQ_EQ_MODE_AUTO = 0, CPQ_EQ_MODE_SEQUENTIAL = 1 } cpq_eq_mode;
int32_t cpq_eq_set_mode(cpq_engine* e, int32_t mode);
/* zero filterState (EQProcessor::prepareToPlay, src/eqprocessor/EQProcessor.Core.cpp:769) */
int32_t cpq_eq_reset(cpq_engine* e);

/* ------------------------------------------------- output filter (N2, adjacent) */
/* POD mirror of convo::BiquadCoeff (src/OutputFilter.h:40-44), a0-normalised Direct Form II Transposed */
typedef struct { double b0, b1, b2, a1, a2; } cpq_biquad_coeffs;
/* OutputFilter::prepare coefficient design (src/OutputFilter.cpp:23-121) for the three sections process() runs:
 * conv_is_last: low cut, high cut stage 0, stage 1; else: 20 Hz high-pass, low-pass stage 0, stage 1.  Host only. */
int32_t cpq_outfilter_design(int32_t conv_is_last, int32_t hc_mode, int32_t lc_mode, int32_t lp_mode,
                             double sample_rate, cpq_biquad_coeffs out[3]);
/* replaces OutputFilter::prepare + the mode arguments of process() (src/OutputFilter.h:106-131) */
int32_t cpq_outfilter_set_params(cpq_engine* e, int32_t stream, int32_t conv_is_last, int32_t hc_mode,
                                 int32_t lc_mode, int32_t lp_mode);
/* replaces OutputFilter::process(block, convIsLast, hcMode, lcMode, lpMode) stereo path: three DF-II-T biquads per
 * sample (biquadStep128_FMA, src/OutputFilter.cpp:143-165, :214-392) */
int32_t cpq_outfilter_process(cpq_engine* e, const double* in, double* out, int32_t n_samples);
int32_t cpq_outfilter_process_device(cpq_engine* e, const double* d_in, double* d_out, int32_t n_samples);
/* OutputFilter::reset (src/OutputFilter.cpp:126-137) */
int32_t cpq_outfilter_reset(cpq_engine* e);
/* on != 0: cpq_engine_process_block also runs the output filter after the conv/EQ pair, as DSPCore does
 * (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:453 ff.); default off */
int32_t cpq_engine_enable_output_filter(cpq_engine* e, int32_t on);

/* ------------------------------------------------------- whole path per call */
/* The remaining per-block values of DSPCore's routing (RuntimeSnapshot fields,
 * src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:384-470), used by cpq_engine_process_block:
 * conv_input_trim_gain: convolverInputTrimGain, multiplied into the EQ output before the convolver in EQ -> conv order
 *   when it differs from 1 by more than 1e-12 (:438-447); output_makeup_gain: outputMakeupGain, multiplied into the
 *   block after the output filter (:465-469).
 * cpq_engine_set_conv_bypass: state.convBypassed -- the convolver stage is not called at all (no latency compensation;
 *   the processor-level bypass with its delay line is cpq_convproc_params.bypassed).  The EQ's bypass is
 *   cpq_eq_set_bypass.  With the output filter enabled it runs for the streams whose convolver or EQ is active (:453-463);
 *   conv_is_last of cpq_outfilter_set_params stays the caller's to pass, as DSPCore derives it (:458-459). */
int32_t cpq_engine_set_gains(cpq_engine* e, int32_t stream, double conv_input_trim_gain, double output_makeup_gain);
int32_t cpq_engine_set_conv_bypass(cpq_engine* e, int32_t bypassed);
/* replaces the DSPCore routing of convolverRt().process(block) and eqRt().process(block, params, cache)
 * (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:386-451) in the configured order. */
int32_t cpq_engine_process_block(cpq_engine* e, const double* in, double* out, int32_t n_samples);
int32_t cpq_engine_process_block_device(cpq_engine* e, const double* d_in, double* d_out, int32_t n_samples);

/* ------------------------------------------------------------- oversampling */
/* CustomInputOversampler (src/CustomInputOversampler.{h,cpp}) around the processing chain, as DSPCore::processDouble
 * runs it (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:359-376, :477-531): a cascade of 1..3 Kaiser
 * half-band FIR stages up, the chain at F x the base rate, the same stages down in reverse order.
 * Stage 0 works at the base rate.  Presets: IIRLike 511/127/31 taps (140/110/90 dB), LinearPhase 1023/255/63 taps
 * (160/140/120 dB). */
typedef enum { CPQ_OS_IIR = 0, CPQ_OS_LINEAR_PHASE = 1 } cpq_os_type;

/* One stage as prepareStage designs it (src/CustomInputOversampler.cpp:287-390). */
typedef struct {
    int32_t taps;                    /* raw taps (odd) */
    int32_t center_tap;              /* (taps - 1) / 2 */
    int32_t center_parity;           /* center_tap & 1 */
    int32_t conv_parity;             /* 1 - center_parity */
    int32_t conv_count;              /* taps of the polyphase FIR branch: raw[conv_parity + 2 r] */
    int32_t center_delay_input;      /* (center_tap - center_parity) / 2, input-rate samples */
    int32_t history_up_keep;         /* max(conv_count - 1, center_delay_input) */
    int32_t history_down_keep;       /* max(center_tap, conv_parity + 2 (conv_count - 1) + 6) */
    double  attenuation_db;
    double  center_coeff;            /* 0.5 */
} cpq_os_stage_info;

/* OversamplingPolicy::resolve (src/audioengine/OversamplingPolicy.h:36-85) for a base (input) rate: requested 0 = Auto
 * (the largest allowed factor), 1/2/4/8 = capped at the largest allowed factor, anything else = Auto.  Returns the
 * resolved factor, 0 when the rate is above 768 kHz (not supported), < 0 for a rate that is not positive and finite.
 * Host only. */
int32_t cpq_os_resolve_factor(double base_rate, int32_t requested);
/* prepareStage for stage 0..2 and a cpq_os_type: fills info (may be NULL) and, when taps is not NULL, the raw tap array
 * (info.taps values; capacity must hold them).  Returns the tap count or < 0.  Host only. */
int32_t cpq_os_design_stage(int32_t stage, int32_t type, cpq_os_stage_info* info, double* taps, int32_t capacity);
/* Round trip (up then down) latency in base-rate samples: sum over the stages i of 2 center_tap_i / 2^(i+1)
 * (290.25 for 8x IIR, 582.25 for 8x LinearPhase; 0 for factor 1).  < 0 for a bad factor or type.  Host only. */
double  cpq_os_latency(int32_t factor, int32_t type);

/* DSPCore::prepare's oversampling.prepare(...) (DSPCoreLifecycle.cpp:114-138, :182-192): factor 1, 2, 4 or 8 and a
 * cpq_os_type.  The engine descriptor and cpq_engine_prepare keep describing the PROCESSING domain (conv and EQ run
 * at the engine's sample rate, as DSPCore prepares them at sampleRate * factor); the base rate is sample_rate / factor.
 * Resets the oversampler's histories, flags and counters; touches no convolver / EQ state.
 * CPQ_ERR_INVALID_ARG: bad factor or type, a CPQ_CALLS_ANY engine whose block_size is not a multiple of the factor,
 * factor > 1 with a processing rate above 768 kHz.
 * With factor > 1, cpq_engine_process_block[_device] takes n_base samples per channel and runs up -> the routing on
 * n_base * factor samples -> down; the call limits apply to n_base * factor.  Factor 1 is the plain path. */
int32_t cpq_engine_set_oversampling(cpq_engine* e, int32_t factor, int32_t type);
/* processUp for every stream: in [channel][n_base] -> out [channel][n_base * factor].  The guards run on the device: a
 * bad (non-finite or |v| > 2^53) FIR sum is replaced by 0, a bad centre value zeroes both outputs of its sample and
 * flags the stream (one corruption event per sample).  A stream in hard fallback outputs silence and does not advance. */
/* CPQ_ERR_NOT_READY while the factor is 1. */
int32_t cpq_os_up(cpq_engine* e, const double* in, double* out, int32_t n_base);
int32_t cpq_os_up_device(cpq_engine* e, const double* d_in, double* d_out, int32_t n_base);
/* processDown for every stream: in [channel][n_base * factor] -> out [channel][n_base].  At the start of the call a
 * flagged stream is cleared (one auto-clear; all histories of the stream zeroed; the block is silence); after 4
 * consecutive auto-clears hard fallback latches.  Deviation from the reference: a stream in hard fallback outputs
 * silence and does not advance its oversampler until cpq_os_reset, cpq_engine_prepare or cpq_engine_set_oversampling
 * (the reference passes the base-rate block through a chain prepared for factor x the rate). */
int32_t cpq_os_down(cpq_engine* e, const double* in, double* out, int32_t n_base);
int32_t cpq_os_down_device(cpq_engine* e, const double* d_in, double* d_out, int32_t n_base);
/* CustomInputOversampler::reset (src/CustomInputOversampler.cpp:452-467): histories, flags, consecutive count and hard
 * fallback cleared; the event and auto-clear counters stay.  cpq_engine_prepare does the same. */
int32_t cpq_os_reset(cpq_engine* e);
/* per-stream counters of one stream; synchronises the engine's stream */
typedef struct {
    uint64_t corruption_events;      /* corruptionEventCount */
    uint64_t auto_clears;            /* corruptionAutoClearCount */
    int32_t  consecutive_auto_clears;
    int32_t  hard_fallback;          /* hardFallbackActive */
    int32_t  corruption_pending;     /* corruptionDetected: the next cpq_os_down silences the stream */
    int32_t  reserved;
} cpq_os_telemetry;
int32_t cpq_os_read_telemetry(cpq_engine* e, int32_t stream, cpq_os_telemetry* out);

/* ---------------------------------------------------------------- IR ingest (host only, no GPU needed) */
/* Everything between an IR file and cpq_engine_set_impulse(): SURVEY.md N3.  One-off loader-thread work in the
 * reference; plain host code here. */
typedef struct {
    int32_t n_channels;
    int32_t n_samples;
    double  sample_rate;
    double* data;                    /* planar [channel][sample], owned by the library: cpq_ir_buffer_free() */
} cpq_ir_buffer;

/* IRConverter::ScaleFactorResult (src/IRConverter.h) plus the stage-2 analysis values it is derived from */
typedef struct {
    double  scale_factor;
    int32_t has_scale_factor;
    float   additional_attenuation_db;
    double  peak_value;              /* of the unscaled IR */
    double  rms_value;
    double  frequency_peak_gain;     /* IRAnalyzer::estimateMaxFrequencyResponseGain of the unscaled IR */
} cpq_ir_scale;

typedef struct {
    cpq_ir_buffer ir;                /* conditioned IR of the target length (stepTrimmed) */
    cpq_ir_scale  scale;             /* scale.scale_factor is what StereoConvolver::init / SetImpulse receive as `scale` */
    int32_t       ir_peak_latency;   /* estimatePeakLatencySamples: the processor-level dry delay on top of the block */
    int32_t       reserved;
} cpq_ir_prepared;

/* LoaderThread::doLoadStep for a WAV file (src/convolver/ConvolverProcessor.LoaderThread.cpp:431-486): RIFF / RF64,
 * PCM 8 / 16 / 24 / 32 bit and IEEE float 32 (plain or WAVE_FORMAT_EXTENSIBLE) -> float as JUCE's reader produces it
 * -> double, NaN and |v| < 1e-20 to 0, clamped to [-1, 1] (src/InputBitDepthTransform.h:31-100).
 * Frames a short file does not hold read as zero (as the reference's reader does); a data chunk claiming more than
 * twice the file size + 1 MiB is refused as corrupted instead.
 * CPQ_ERR_INVALID_ARG: missing file / no frames; CPQ_ERR_UNSUPPORTED: not a WAV the reference's reader would accept. */
int32_t cpq_ir_load_wav(const char* path, cpq_ir_buffer* out);
void    cpq_ir_buffer_free(cpq_ir_buffer* b);

/* ConvolverProcessor::PhaseMode (src/ConvolverProcessor.h:117-122) */
typedef enum { CPQ_PHASE_AS_IS = 0, CPQ_PHASE_MIXED = 1 /* not built: CPQ_ERR_UNSUPPORTED */, CPQ_PHASE_MINIMUM = 2 } cpq_phase_mode;

/* doTrimStep + doTransformStep (LoaderThread.cpp:490-641, 644-709): trailing-silence trim, 1 Hz DC
 * blocker, asymmetric Tukey window about the peak, zero-padded / cut to int(rate * target_ir_length_sec) samples
 * (IR_LENGTH 0.5..3 s, default 1 s; cap 2^21) with a linear fade-out, computeScaleFactor against the IR playing now
 * (current_ir may be NULL), peak latency.  An IR whose rate differs from sample_rate is refused with CPQ_ERR_UNSUPPORTED:
 * convert it with cpq_ir_resample() first (the reference's loader does both in one step). */
int32_t cpq_ir_prepare(const cpq_ir_buffer* loaded, double sample_rate, float target_ir_length_sec, int32_t phase_mode,
                       const cpq_ir_buffer* current_ir, double current_scale, cpq_ir_prepared* out);
/* ConvolverProcessorInternal::convertToMinimumPhase (src/convolver/ConvolverProcessor.ResampleAndFallback.cpp:333-469):
 * homomorphic minimum-phase reconstruction at 4x zero padding, every channel on its own.  CPQ_ERR_UNSUPPORTED where the
 * reference gives up (4 n above 8388608 samples, non-finite intermediate values). */
int32_t cpq_ir_convert_to_minimum_phase(const cpq_ir_buffer* in, cpq_ir_buffer* out);
void    cpq_ir_prepared_free(cpq_ir_prepared* p);

/* IRConverter::computeScaleFactor(ir, currentIr, currentScale) (src/IRConverter.cpp:175-196): energy normalisation to
 * -6 dB, then peak (0.5) / RMS (0.25) / frequency-response (+3 dB) clamps and the 4x jump protection. */
int32_t cpq_ir_compute_scale_factor(const double* const* ir, int32_t n_channels, int32_t n_samples,
                                    const double* const* current_ir, int32_t current_channels, int32_t current_samples,
                                    double current_scale, cpq_ir_scale* out);
/* IRAnalyzer::estimateMaxFrequencyResponseGain (src/IRAnalyzer.cpp:63-155) */
double  cpq_ir_estimate_max_frequency_response_gain(const double* const* ir, int32_t n_channels, int32_t n_samples);
/* LoaderThread::estimatePeakLatencySamples (LoaderThread.cpp:149-209) */
int32_t cpq_ir_estimate_peak_latency(const double* const* ir, int32_t n_channels, int32_t n_samples);

/* ---------------------------------------------------------------- IR sample-rate conversion */
/* ConvolverProcessorInternal::resampleIR (src/convolver/ConvolverProcessor.ResampleAndFallback.cpp:18-108), which the reference's
 * loader runs on every IR before the trim (LoaderThread.cpp:555-587) with r8brain's CDSPResampler at a 2 % transition band,
 * 140 dB stop band, linear phase.  Here: one linear-phase Kaiser-windowed sinc of the same class, as a polyphase table, applied
 * by k_ir_resample to a whole batch of rows (a row is one channel of one IR) in one launch per source rate.
 *
 * Rates are whole numbers of Hz in 8000 ... 768000; in : out reduces by its gcd to M : L (L up, M down), and L or M above 1280
 * is refused.  Output j of a row x of n samples, for j < ceil(n out / in), is
 *     acc = 0;  for k = 0 ... T - 1:  acc = fma(taps[(j M) mod L][k], x[floor(j M / L) + T / 2 - k], acc)
 * in fp64, in that order, with x zero outside 0 ... n - 1: output 0 sits at input time 0, the filter's group delay (T / 2 input
 * samples) is removed and the ringing before t = 0 is dropped, as r8brain's oneshot() does.  The device and the host path compute
 * exactly this, so they agree bit for bit and a row's result does not depend on what else is in the batch. */
#define CPQ_HAS_IR_RESAMPLING 1
#define CPQ_RESAMPLE_MAX_FACTOR 1280
typedef enum { CPQ_RESAMPLE_LINEAR_PHASE = 0, CPQ_RESAMPLE_MINIMUM_PHASE = 1 /* not built: CPQ_ERR_UNSUPPORTED */ } cpq_resample_phase;
typedef struct {
    int32_t l, m;                    /* out : in reduced, l up and m down */
    int32_t taps;                    /* T: taps per phase (even); the table is [l][taps] */
    int32_t reserved;
    double  group_delay;             /* in input samples: taps / 2 */
    double  cutoff;                  /* -6 dB point as a fraction of the input's Nyquist frequency: 0.98 min(in, out) / in */
    double  attenuation_db;          /* the Kaiser window's design attenuation */
} cpq_resample_info;
/* The filter of a rate pair (host only, no GPU).  The pass band ends at 0.96 and the stop band begins at 1.0 of the lower of the
 * two Nyquist frequencies; every phase sums to 1.  Returns l * taps, the number of doubles of the table, and copies it to
 * table[phase][tap] when table is not NULL.  CPQ_ERR_UNSUPPORTED: a rate that is not a whole number, outside 8000 ... 768000, or
 * l or m above CPQ_RESAMPLE_MAX_FACTOR; CPQ_ERR_INVALID_ARG: capacity below l * taps.  Equal rates are not an error (l = m = 1). */
int32_t cpq_resample_design(double in_rate, double out_rate, cpq_resample_info* info, double* table, int32_t capacity);
/* in at in->sample_rate -> out at target_rate on the current device; out is the library's (cpq_ir_buffer_free) and is zeroed on
 * any error.  Rates no more than 1e-6 apart: a copy, without a device.  Every channel is converted to ceil(n out / in) samples,
 * then cut after the last run of 8 samples above -160 dB of its own peak (ResampleAndFallback.cpp:66-87, on the host); the buffer
 * is as long as the longest channel and a channel is zero beyond its own length.  Refused before anything is allocated:
 * CPQ_ERR_INVALID_ARG for a null argument, no channels, no samples, a rate that is not positive and finite (the reference hands
 * such a buffer back unchanged) or an unknown phase; CPQ_ERR_SILENT_IR for a peak below 1e-12; CPQ_ERR_UNSUPPORTED for
 * CPQ_RESAMPLE_MINIMUM_PHASE and for what cpq_resample_design refuses.  CPQ_ERR_NO_DEVICE without a gfx950 device: there is no
 * quiet fall-back, the host path is a call of its own.  The reason is in cpq_last_error(NULL). */
int32_t cpq_ir_resample(const cpq_ir_buffer* in, double target_rate, int32_t phase, cpq_ir_buffer* out);
/* n IRs in one call: IRs of one source rate share one launch.  out[i] is what cpq_ir_resample(in[i]) returns, bit for bit.  All
 * or nothing: on an error every out[i] is zeroed. */
int32_t cpq_ir_resample_batch(const cpq_ir_buffer* const* in, int32_t n, double target_rate, int32_t phase, cpq_ir_buffer* out /* [n] */);
/* milliseconds the kernel launches of this thread's last cpq_ir_resample* call took, from device events (the call's time also
 * holds the transfers and the trim); negative when that call launched nothing */
double  cpq_ir_resample_last_kernel_ms(void);
/* the same table in the same summation order on the host's threads (at most 16): what the device is checked against; no GPU */
int32_t cpq_ir_resample_host(const cpq_ir_buffer* in, double target_rate, int32_t phase, cpq_ir_buffer* out);

/* ---------------------------------------------------------------- streaming sample-rate conversion of audio */
/* cpq_src: the filter of cpq_resample_design applied to audio, call by call, for n_channels planar fp64 rows at once; an object of
 * its own beside cpq_engine (an engine runs at one rate: sources at another rate pass through a cpq_src in front of it).  The
 * object keeps the history between calls.  Two objects, one definition, equal bits: the one that computes on the host
 * (flags = CPQ_SRC_HOST, the counterpart of cpq_ir_resample_host, no GPU) and the one that computes on the device (flags =
 * CPQ_SRC_DEVICE, gfx950 kernels, CPQ_ERR_NO_DEVICE without one).  The caller says which: flags = 0 is CPQ_ERR_UNSUPPORTED, and
 * neither object ever stands in for the other.
 *
 * Let x be everything a stream received since creation, cpq_src_reset or the last flush, zero before index 0 and, after a flush,
 * zero from its end on.  Output j is the sum stated above for cpq_ir_resample, in that order and with that fma.  A call emits
 * every j, in order, whose newest input floor(j M / L) + T / 2 has been received; with flush != 0 it also emits the rest, up to
 * ceil(n_total L / M) outputs in all, and leaves the object as new.  So the concatenated output of a stream equals the one-shot
 * conversion of the concatenated input bit for bit, for every split into calls and every channel count; the latency is T / 2
 * input samples.  Rates no more than 1e-6 apart: a copy, latency 0.
 *
 * start_period = p >= 0 starts the stream at output p L and input p M, as if p whole periods of silence had passed (for
 * resuming); by the filter's periodicity the outputs are those of p = 0 bit for bit.
 *
 * Rows are [channel][stride] doubles; n_in may be 0 and *n_out may come back 0.  Refused before any state changes,
 * CPQ_ERR_INVALID_ARG: a null pointer (in may be NULL when n_in == 0, out when nothing is written), n_channels outside 1 ... 65535,
 * max_in < 1, start_period outside 0 ... 2^50, an unknown phase or flag, n_in < 0 or above max_in, a stride shorter than its row,
 * out_capacity below cpq_src_out_count, rows of in and out that overlap; CPQ_ERR_UNSUPPORTED: what cpq_resample_design refuses,
 * CPQ_RESAMPLE_MINIMUM_PHASE, a max_in whose cpq_src_max_out exceeds 2^30, and flags = 0.  The reason is in
 * cpq_src_last_error (with NULL: of a failed create). */
/* CPQ_HAS_STREAM_RESAMPLING_HOST announces the host object, CPQ_HAS_STREAM_RESAMPLING the device object with
 * cpq_src_process_device, cpq_src_set_stream and cpq_src_last_kernel_ms.  Both flags at once, or an unknown bit, are
 * CPQ_ERR_INVALID_ARG. */
#define CPQ_HAS_STREAM_RESAMPLING_HOST 1
#define CPQ_HAS_STREAM_RESAMPLING 1
#define CPQ_SRC_HOST 1u
#define CPQ_SRC_DEVICE 2u
typedef struct cpq_src cpq_src;
typedef struct {
    int32_t  n_channels;
    double   in_rate, out_rate;
    int32_t  max_in;                /* most samples per channel of one call */
    int32_t  phase;                 /* cpq_resample_phase */
    uint32_t flags;                 /* CPQ_SRC_* */
    int64_t  start_period;
} cpq_src_desc;
int32_t cpq_src_create(const cpq_src_desc* desc, cpq_src** out);
void    cpq_src_destroy(cpq_src* s);
const char* cpq_src_last_error(const cpq_src* s);
/* forgets the stream: the object is as new */
int32_t cpq_src_reset(cpq_src* s);
/* T / 2 in input samples; 0 for a copy; negative: s is NULL */
int32_t cpq_src_latency(const cpq_src* s);
/* samples per channel the next call of n_in samples will write: host arithmetic only.  CPQ_ERR_INVALID_ARG (negative) for a
 * NULL object or n_in outside 0 ... max_in. */
int32_t cpq_src_out_count(const cpq_src* s, int32_t n_in, int32_t flush);
/* the bound of cpq_src_out_count for any call: a call of max_in samples with flush */
int32_t cpq_src_max_out(const cpq_src* s);
/* host rows in and out.  On a device object the rows pass through buffers the object owns ([n_channels][max_in] and
 * [n_channels][cpq_src_max_out]): upload, the device call, download, and the object's stream is synchronised before the return. */
int32_t cpq_src_process(cpq_src* s, const double* in, int64_t in_stride, int32_t n_in, double* out, int64_t out_stride,
                        int32_t out_capacity, int32_t flush, int32_t* n_out);
/* Device object only (a host object: CPQ_ERR_INVALID_ARG): device rows in and out, the same refusals in the same order, all
 * before any state changes.  Asynchronous: the call enqueues its work on the object's stream and returns; d_in and d_out must stay
 * valid, and d_in unchanged, until the stream has reached the call.  d_out is written at [channel][0 ... *n_out) and nowhere else.
 * CPQ_ERR_DEVICE: a launch failed; the state is as before the call. */
int32_t cpq_src_process_device(cpq_src* s, const double* d_in, int64_t in_stride, int32_t n_in, double* d_out, int64_t out_stride,
                               int32_t out_capacity, int32_t flush, int32_t* n_out);
/* Device object only: the stream (a hipStream_t; NULL, the default, is the null stream) every later call enqueues on.  The stream
 * used so far is synchronised first, so the history a call reads has been written. */
int32_t cpq_src_set_stream(cpq_src* s, void* stream);
/* milliseconds between device events around the launches of the last cpq_src_process on a device object (transfers excluded);
 * -1 on a host object, for NULL, and before such a call.  cpq_src_process_device records no events. */
double  cpq_src_last_kernel_ms(const cpq_src* s);

/* ---------------------------------------------------------------- gated programme loudness (EBU R 128) per stream */
/* cpq_loudness: integrated loudness (BS.1770-4 gating), loudness range (EBU Tech 3342), the momentary and short-term maxima of
 * n_streams stereo programmes at once, computed on the device; an object of its own beside cpq_engine.  Rows are planar fp64,
 * [2 n_streams] of them, L0 R0 L1 R1 ... as cpq_engine_process_block_device writes them, so that an engine's output rows are
 * metered where they lie.  The K-weighting is cpq_meter_kweighting(sample_rate), the filter of the per-callback records
 * (cpq_engine_set_metering), its state carried over calls; samples are scrubbed as the meters scrub them (not finite or
 * |v| >= 1e300 reads as 0).  The K-weighted squares of both channels are added up on a grid of hops of sample_rate / 10
 * samples that belongs to the stream, not to a call: calls may have any length and a hop may straddle them.  The definition,
 * with the order of every sum and the rounding rule of the range's percentiles, is convopeq_amd/csrc/prog_plan.hpp's.
 *
 * sample_rate: a whole number of Hz in 8000 ... 768000 that is divisible by 10, else CPQ_ERR_UNSUPPORTED.  max_seconds: the
 * longest programme (hops are kept for all of it: 80 bytes per stream and second); more than 8192 short-term blocks at the 1 s
 * step (2 1/4 hours) is CPQ_ERR_UNSUPPORTED.  flags: 0.  CPQ_ERR_INVALID_ARG: a null argument, n_streams outside 1 ... 32767,
 * max_seconds not positive and finite, flags not 0.  CPQ_ERR_NO_DEVICE without a gfx950 device: there is no host object.
 * Everything the object keeps on the device is cleared before create returns.  The reason of a refusal is in
 * cpq_loudness_last_error (with NULL: of a failed create). */
#define CPQ_HAS_PROGRAMME_LOUDNESS 1
typedef struct cpq_loudness cpq_loudness;
typedef struct {
    int32_t n_streams;
    double  sample_rate;
    double  max_seconds;
    int32_t flags;
} cpq_loudness_desc;
/* Loudnesses in LUFS, range in LU.  An empty set gives -HUGE_VAL for its loudness and 0 for the range; the counts tell "silent"
 * (n_blocks > 0, n_abs == 0) from "too short" (n_blocks == 0). */
typedef struct {
    double  integrated;             /* mean of the momentary blocks past both gates */
    double  range;                  /* LRA */
    double  momentary_max;          /* over every 400 ms block */
    double  short_term_max;         /* over every 3 s block, at every hop */
    double  relative_gate;          /* the gate of `integrated`: 10 LU below the mean of the blocks above -70 LUFS */
    int64_t n_hops;                 /* complete hops so far */
    int32_t n_blocks;               /* momentary blocks: n_hops - 3 */
    int32_t n_abs;                  /* of those above -70 LUFS */
    int32_t n_rel;                  /* of those also above the relative gate */
    int32_t n_short_kept;           /* short-term blocks at the 1 s step past both gates of the range */
} cpq_loudness_result;
int32_t cpq_loudness_create(const cpq_loudness_desc* desc, cpq_loudness** out);
void    cpq_loudness_destroy(cpq_loudness* p);
const char* cpq_loudness_last_error(const cpq_loudness* p);
/* the programmes start again: hop sums, partial hops and filter states cleared; the object's stream is synchronised */
int32_t cpq_loudness_reset(cpq_loudness* p);
/* the stream (a hipStream_t; NULL, the default, is the null stream) every later call enqueues on; the stream used so far is
 * synchronised first */
int32_t cpq_loudness_set_stream(cpq_loudness* p, void* stream);
/* n_samples more samples of every programme from device rows d_rows[(2 s + channel) * row_stride + i].  Asynchronous: enqueued on
 * the object's stream; the rows must stay as they are until the stream has reached the call.  Refused before any state moves, in
 * this order: a null object (no message) or buffer, n_samples outside 1 ... 2^30, row_stride below n_samples, a buffer that is not
 * 16-byte aligned (all CPQ_ERR_INVALID_ARG), a call that would pass max_seconds (CPQ_ERR_UNSUPPORTED: no part of it is taken). */
int32_t cpq_loudness_process_device(cpq_loudness* p, const double* d_rows, int64_t row_stride, int32_t n_samples);
/* the same from host rows, through a buffer the object owns; the object's stream is synchronised before the return */
int32_t cpq_loudness_process(cpq_loudness* p, const double* rows, int64_t row_stride, int32_t n_samples);
/* out[n_streams]: the figures of everything taken so far.  Synchronises the object's stream.  May be called at any time and
 * repeatedly; the programmes go on. */
int32_t cpq_loudness_finish(cpq_loudness* p, cpq_loudness_result* out);
/* diagnostic and test hook: *n = the complete hops so far, out[0 ... min(*n, capacity)) = their sums E[h] of one stream.
 * Synchronises the object's stream. */
int32_t cpq_loudness_read_hops(cpq_loudness* p, int32_t stream, double* out, int64_t capacity, int64_t* n);
/* host only: the same figures from hop sums on the host (hops[n_hops] of one stream), in the device's order of operations */
int32_t cpq_loudness_finish_host(const double* hops, int64_t n_hops, double sample_rate, cpq_loudness_result* out);
/* host only: the linear gain 10^((target_lufs - integrated) / 20) that brings the programme to target_lufs.  Applying it is the
 * caller's.  CPQ_ERR_NOT_READY where nothing passed the gates (integrated is -HUGE_VAL); *gain is left alone. */
int32_t cpq_loudness_gain(const cpq_loudness_result* r, double target_lufs, double* gain);

/* True peak per programme (ITU-R BS.1770-4 Annex 2: the 48-tap, 4-phase interpolator) and normalisation under a ceiling: the
 * second number of a delivery specification (-23 LUFS and -1 dBTP for R 128).  Per channel, over the whole programme since create
 * or reset, on the scrubbed samples: true_peak = max |y| over every sample and the phases in use, sample_peak = max |x|, both
 * linear.  All four phases below 88200 Hz; phases 0 and 2 from 88200 Hz to below 176400 Hz; from 176400 Hz true_peak is
 * sample_peak.  The table, the order of the 12-term sum and the state carried over calls (the last 11 samples) are
 * convopeq_amd/csrc/prog_plan.hpp's; the result is defined to the bit.  This is not the engine's per-callback detector
 * (cpq_engine_set_metering: the reference's, and not a standard one). */
#define CPQ_HAS_PROGRAMME_TRUE_PEAK 1
typedef struct { double true_peak[2]; double sample_peak[2]; } cpq_loudness_peaks;   /* linear; L, R */
/* on: 1 or 0.  Accepted only at the start of a programme (after create or reset, before a sample was taken), else
 * CPQ_ERR_NOT_READY.  Switching on allocates and clears the peak state synchronously, all or nothing (CPQ_ERR_OOM); from then on
 * cpq_loudness_process and cpq_loudness_process_device also take the peaks of what they are given, and cpq_loudness_reset clears
 * them.  The hop sums do not depend on the switch. */
int32_t cpq_loudness_set_true_peak(cpq_loudness* p, int32_t on);
/* out[n_streams]: the peaks of everything taken so far.  Synchronises the object's stream.  CPQ_ERR_NOT_READY without the switch. */
int32_t cpq_loudness_read_peaks(cpq_loudness* p, cpq_loudness_peaks* out);
/* host only: the same two figures of n_rows rows of n_samples samples at rows[r * row_stride + i], each row a programme from its
 * start; true_peak[n_rows], sample_peak[n_rows].  The rate rule is create's. */
int32_t cpq_loudness_peaks_host(const double* rows, int64_t row_stride, int32_t n_rows, int64_t n_samples, double sample_rate,
                                double* true_peak, double* sample_peak);
/* host only: *gain = min(g_loud, g_peak), *limited = 1 where the ceiling won.  g_loud is cpq_loudness_gain's; g_peak =
 * 10^(max_true_peak_dbtp / 20) / peak with peak the largest of the stream's four values (the sample peaks included: at fs / 4 a
 * phase of the interpolator reads below the samples); peak == 0 sets no limit.  CPQ_ERR_INVALID_ARG: a null or non-finite
 * argument, a peak that is negative or not finite.  CPQ_ERR_NOT_READY where nothing passed the gates; *gain is left alone. */
int32_t cpq_loudness_gain_limited(const cpq_loudness_result* r, const cpq_loudness_peaks* pk, double target_lufs,
                                  double max_true_peak_dbtp, double* gain, int32_t* limited);
/* d_out[(2 s + channel) * out_stride + i] = d_in[(2 s + channel) * in_stride + i] * gains[s]: one rounding, nothing scrubbed.
 * gains[n_streams] on the host, uploaded into a buffer of the object on its stream by the call.  Works on any object, does not
 * touch the programme, asynchronous on the object's stream.  In place with d_out == d_in and equal strides.  Refused before
 * anything moves, all CPQ_ERR_INVALID_ARG: a null object (no message) or buffer, n_samples outside 1 ... 2^30, a stride below
 * n_samples, a device buffer that is not 16-byte aligned, a gain that is not finite, rows of d_in and d_out that overlap in part. */
int32_t cpq_loudness_apply_device(cpq_loudness* p, const double* gains, const double* d_in, int64_t in_stride, double* d_out,
                                  int64_t out_stride, int32_t n_samples);

/* ---------------------------------------------------------------- look-ahead true-peak limiter per programme */
/* cpq_limiter: where the ceiling would win in cpq_loudness_gain_limited, apply the loudness gain and pull down only the
 * neighbourhood of the peaks that would pass the ceiling.  An object of its own beside the engine, n_streams stereo programmes at
 * once, rows planar float64 at (2 s + channel) * stride + i.  The result is defined to the bit (csrc/lim_plan.hpp, DESIGN.md
 * 4.18), equal for every split of a programme into calls and equal from the object that computes on the host (CPQ_LIM_HOST, no
 * GPU needed) and the one that computes on the device (CPQ_LIM_DEVICE, gfx950 kernels).  With c the linear ceiling, W the window,
 * M = W + 12, D = W + 11 and g the stream's pre-gain:
 *     u[ch][i] = x[ch][i] * g, a product that is not finite or reaches 1e300 in magnitude read as 0.0 (so a sample that is not
 *                finite comes out as 0.0)
 *     p[i]     = the largest of |u[0][i]|, |u[1][i]| and the BS.1770-4 Annex 2 interpolator's phases in use over u[ch][i - 11 ... i]
 *                of both channels (all four phases below 88200 Hz, 0 and 2 below 176400 Hz, none from there on: cpq_loudness's rule)
 *     r[i]     = p[i] > c ? c / p[i] : 1.0          m[i] = min(r[i - M + 1 ... i])
 *     a[i]     = (m[i] + m[i - 1] + ... + m[i - W + 1]) / W, added in that order
 *     y[ch][i] = u[ch][i - D] * a[i]
 * with everything before the programme 0.0 (r = 1.0).  The channels of a stream are linked.  A call of n samples emits n outputs;
 * the first D of a programme are zeros; a flush emits the last D and leaves the object at the start of a new programme.
 * |y| <= c + (W + 3) ulp(c).  The true peak of y may pass c by the slope of a inside the interpolator's 12 taps: RESULTS.md has
 * the measured overshoot.  There is no release recurrence and no iteration to a loudness target.
 *
 * cpq_limiter_create refuses, in this order: a null out, n_streams outside 1 ... 32767, unknown flags, both flags, a sample_rate
 * that is not finite and > 0, a ceiling_dbtp outside -200 ... 200, a window_samples that is neither 0 nor in 8 ... 1024 (all
 * CPQ_ERR_INVALID_ARG); a rate that is not a whole number of Hz in 8000 ... 768000 divisible by 10, then flags == 0 (the caller says
 * where the rows are computed; both CPQ_ERR_UNSUPPORTED); CPQ_LIM_DEVICE without a gfx950 device (CPQ_ERR_NO_DEVICE).
 * window_samples = 0 takes cpq_limiter_default_window(sample_rate) = round(0.0015 * rate) clamped to 8 ... 1024.  The reason of
 * a refused create is in cpq_last_error(NULL). */
#define CPQ_HAS_TRUE_PEAK_LIMITER 1
#define CPQ_LIM_HOST   1u
#define CPQ_LIM_DEVICE 2u
typedef struct cpq_limiter cpq_limiter;
typedef struct {
    double  min_gain;           /* the smallest a of the programme's outputs so far; 1.0 where nothing was limited */
    int64_t limited_samples;    /* outputs with a < 1.0 */
} cpq_limiter_telemetry;
int32_t cpq_limiter_default_window(double sample_rate);     /* CPQ_ERR_INVALID_ARG (negative) for a rate not finite and > 0 */
int32_t cpq_limiter_create(int32_t n_streams, double sample_rate, double ceiling_dbtp, int32_t window_samples, uint32_t flags,
                           cpq_limiter** out);
void cpq_limiter_destroy(cpq_limiter* p);
const char* cpq_limiter_last_error(const cpq_limiter* p);
/* Device object only (a host object: CPQ_ERR_INVALID_ARG).  Synchronises the stream used so far, then later calls enqueue on
 * `stream` (a hipStream_t; NULL: the null stream). */
int32_t cpq_limiter_set_stream(cpq_limiter* p, void* stream);
/* Back to the start of a programme without the last D outputs: host state only.  The gains stay. */
int32_t cpq_limiter_reset(cpq_limiter* p);
int32_t cpq_limiter_latency(const cpq_limiter* p);          /* D = window + 11 samples */
int32_t cpq_limiter_window(const cpq_limiter* p);
/* gains[n_streams], the pre-gain of every stream (default 1.0; they stay over flush and reset).  Refused in this order: a null
 * object (no message) or null gains, a gain that is not finite or is negative (CPQ_ERR_INVALID_ARG), a programme that has
 * started (CPQ_ERR_NOT_READY: flush or reset first).  On a device object it synchronises the stream. */
int32_t cpq_limiter_set_gains(cpq_limiter* p, const double* gains);
/* n_samples more of every programme, device rows in and out, asynchronous on the object's stream: d_in must stay as it is
 * until that stream has reached the call.  Refused before any state moves, in this order, all CPQ_ERR_INVALID_ARG: a null object
 * (no message), a host object, a null buffer, n_samples outside 1 ... 2^30, a stride below n_samples, a buffer that is not
 * 16-byte aligned, rows of d_in and d_out that overlap in part.  In place (d_out == d_in, equal strides) is allowed and costs a
 * device copy of the call's rows into a buffer of the object, since a tile reads its neighbours' input; apart is the fast path.
 * Rows move 16 bytes at a time where both strides are even.  CPQ_ERR_OOM / CPQ_ERR_DEVICE: the state is as before the call. */
int32_t cpq_limiter_process_device(cpq_limiter* p, const double* d_in, int64_t in_stride, double* d_out, int64_t out_stride,
                                   int32_t n_samples);
/* The same on host rows, on either object (the device object copies through buffers it owns and synchronises); the same
 * refusals in the same order without the host-object and alignment rules. */
int32_t cpq_limiter_process(cpq_limiter* p, const double* in, int64_t in_stride, double* out, int64_t out_stride, int32_t n_samples);
/* The last D = cpq_limiter_latency outputs of every programme to rows of at least D samples, then the object is at the start of
 * a new programme (gains and telemetry stay; the next call starts the telemetry over).  Refused in this order, all
 * CPQ_ERR_INVALID_ARG: a null object, (flush_device) a host object, a null buffer, a stride below D, (flush_device) a buffer that
 * is not 16-byte aligned. */
int32_t cpq_limiter_flush_device(cpq_limiter* p, double* d_out, int64_t out_stride);
int32_t cpq_limiter_flush(cpq_limiter* p, double* out, int64_t out_stride);
/* out[n_streams]: the telemetry of the programme in progress, or of the one a flush just ended; { 1.0, 0 } after create and
 * reset.  It counts every output emitted, so it does not depend on how the programme was split into calls.  Synchronises the
 * object's stream.  CPQ_ERR_INVALID_ARG: a null object or result. */
int32_t cpq_limiter_read_telemetry(cpq_limiter* p, cpq_limiter_telemetry* out);
/* Device time of the two launches of the last call of a device object, waiting for them; -1 on a host object or before a call. */
double cpq_limiter_last_kernel_ms(cpq_limiter* p);

/* ---------------------------------------------------------------- minimum-phase conversion on the device */
/* cpq_ir_convert_to_minimum_phase for a whole IR library: convertToMinimumPhase (ResampleAndFallback.cpp:333-469) per row (a row
 * is one channel of one IR of n samples), rows of one FFT size N = nextPow2(4 n) batched into one sequence of launches:
 *     zero-pad to N -> FFT -> ln max(|X|, 1e-300) -> IFFT / N -> fold (bin 0 and N / 2 real, 1 ... N / 2 - 1 real * 2, rest 0)
 *     -> FFT -> clamp re and im to +-50, exp(re) (cos im, sin im) -> IFFT / N -> real part of the first n, |v| < 1e-18 -> 0
 * in fp64.  N <= 4096 stays in LDS from the samples in to the samples out; above, N = N1 N2 runs as column and row passes over a
 * complex scratch row.  The FFTs are not the host path's, so the result agrees with
 * cpq_ir_convert_to_minimum_phase to rounding, not bit for bit; an IR's result does not depend on what else is in the batch or
 * on workspace_bytes, bit for bit.
 *
 * Refused before anything is allocated (CPQ_ERR_INVALID_ARG): a null argument, n < 0, a buffer without channels, samples or data,
 * workspace_bytes < 0, workspace_bytes below what one row needs (cpq_last_error(NULL) names the need).  Per IR, in status[i]:
 * CPQ_ERR_UNSUPPORTED where the reference gives up -- 4 n above 8388608 (decided on the host; the other IRs still run), or a
 * value that is not finite after the exponential or in the output of one of its rows -- and out[i] is zeroed; else CPQ_OK and
 * out[i] is the library's (cpq_ir_buffer_free).  The call returns CPQ_OK when it ran, CPQ_ERR_NO_DEVICE without a gfx950 device
 * when a row needs one (no quiet fall-back: the host path is a call of its own), CPQ_ERR_OOM / CPQ_ERR_DEVICE otherwise; on an
 * error every out[i] is zeroed.
 *
 * workspace_bytes caps the device scratch of the call: per row 16 n + 32 bytes, plus 16 N above N = 4096; the rows of one FFT size
 * run in as many chunks as the cap needs.  0: 2 GiB.  The twiddle tables (at most 160 KB) are not counted. */
#define CPQ_HAS_IR_MINPHASE_DEVICE 1
int32_t cpq_ir_minimum_phase_batch(const cpq_ir_buffer* const* in, int32_t n, int64_t workspace_bytes, cpq_ir_buffer* out /* [n] */,
                                   int32_t* status /* [n] */);
/* a batch of one with the default workspace; returns status[0] */
int32_t cpq_ir_minimum_phase(const cpq_ir_buffer* in, cpq_ir_buffer* out);
/* milliseconds the kernel launches of this thread's last cpq_ir_minimum_phase* call took, from device events; negative when that
 * call launched nothing */
double  cpq_ir_minimum_phase_last_kernel_ms(void);
/* cpq_ir_prepare for n IRs: trim, DC blocker, window, target length per IR on the host, then with CPQ_PHASE_MINIMUM one
 * cpq_ir_minimum_phase_batch over all of them (a conversion that is refused or does not validate leaves that IR as trimmed, as
 * the reference does), then scale factor and peak latency per IR.  current_ir: NULL or [n] with NULL entries allowed;
 * current_scale: NULL (1.0) or [n].  With CPQ_PHASE_AS_IS no device is needed and out[i] is cpq_ir_prepare's result bit for bit.
 * CPQ_PHASE_MIXED is CPQ_ERR_UNSUPPORTED.  All or nothing: on an error every out[i] is zeroed and cpq_last_error(NULL) names the
 * IR ("IR i"). */
int32_t cpq_ir_prepare_batch(const cpq_ir_buffer* const* loaded, int32_t n, double sample_rate, float target_ir_length_sec,
                             int32_t phase_mode, const cpq_ir_buffer* const* current_ir /* NULL or [n], entries may be NULL */,
                             const double* current_scale /* NULL or [n] */, cpq_ir_prepared* out /* [n] */);

/* ---------------------------------------------------------------- metering */
/* The two meters DSPCore runs on the final block of every callback (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:
 * 695-701): LoudnessMeter::processBlock (src/LoudnessMeter.{h,cpp}; ITU-R BS.1770 K-weighting, mean square and peak per
 * callback) and TruePeakDetector::processBlock (src/TruePeakDetector.{h,cpp}; 4x oversampled peak from two half-band FIR
 * stages, decaying hold).  They read the base-rate output rows of cpq_engine_process_block[_device] (with oversampling: after
 * the down stages), one callback = block_size / factor samples at a time, and never alter them.  A sample that is not finite
 * or has |v| >= 1e300 is read as 0 (the scrub at :665-693 runs before the meters).  Off by default. */
#define CPQ_METER_LOUDNESS  1
#define CPQ_METER_TRUE_PEAK 2

/* one callback of one stream; the fields of a meter that is off are 0 */
typedef struct {
    double   mean_square;            /* (sum L^2 + sum R^2) / n of the K-weighted callback (BlockPower::meanSquare) */
    double   peak_linear;            /* max |K-weighted sample| over both channels (BlockPower::peakLinear) */
    double   true_peak;              /* max |4x oversampled sample| over both channels of this callback */
    double   true_peak_hold;         /* peakHold after this callback: tp > hold ? tp : hold * 0.999 */
    uint64_t block_index;            /* blockCounter++: counts on for records dropped on a full ring */
} cpq_meter_block;

/* LoudnessMeter::updateCoefficients(fs) in the reference's operation order: pre[5] = the +4 dB high shelf at 1500 Hz
 * (Q = 1/sqrt 2), rlb[5] = the 38 Hz high-pass (Q = 0.5), both {b0, b1, b2, a1, a2} / a0 of Direct Form I.  Host only. */
int32_t cpq_meter_kweighting(double rate, double pre[5], double rlb[5]);
/* TruePeakDetector::prepareStage for stage 0 (63 taps) or 1 (31 taps), 100 dB: as cpq_os_design_stage.  Host only. */
int32_t cpq_meter_tp_design_stage(int32_t stage, cpq_os_stage_info* info, double* taps, int32_t capacity);
/* flags: 0 = off, or CPQ_METER_LOUDNESS | CPQ_METER_TRUE_PEAK.  Any change resets the meters.  The filters are designed for
 * the base rate sample_rate / factor; cpq_engine_prepare and cpq_engine_set_oversampling redesign them and reset the meters.
 * While true peak is on a call must be whole callbacks (else CPQ_ERR_UNSUPPORTED, before any state moves: the reference's
 * result then depends on stale memory) and a callback must hold at least 8 samples; loudness alone accepts the ragged calls
 * of CPQ_CALLS_ANY, the short last chunk being one callback of its own length. */
int32_t cpq_engine_set_metering(cpq_engine* e, int32_t flags);
/* LoudnessMeter::reset + TruePeakDetector::reset: filter states, histories, hold, block counter and the ring */
int32_t cpq_meter_reset(cpq_engine* e);
/* Meters caller rows [channel][n_samples] exactly as the engine's output would be, without running the chain.
 * CPQ_ERR_NOT_READY while metering is off. */
int32_t cpq_meter_process(cpq_engine* e, const double* in, int32_t n_samples);
int32_t cpq_meter_process_device(cpq_engine* e, const double* d_in, int32_t n_samples);
/* Synchronises the engine's stream and pops the oldest min(max_blocks, stored) records of every stream at once:
 * out[stream * max_blocks + i].  Every stream holds a ring of 4096 records; a record that finds it full is dropped (its
 * block_index is still consumed).  *n_blocks = records popped per stream, *n_dropped = records dropped per stream since the
 * last read (either may be NULL).  CPQ_ERR_NOT_READY while metering is off. */
int32_t cpq_meter_read_blocks(cpq_engine* e, cpq_meter_block* out, int32_t max_blocks, int32_t* n_blocks, int64_t* n_dropped);

/* ---------------------------------------------------------------- soft clipper */
/* The soft clipper DSPCore::processDouble runs between the output make-up gain and the oversampler's down stages
 * (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:471-503; softClipBlockAVX2 :133-224), memoryless, per channel.
 * With sat = (double)saturation_amount: threshold = 0.95 - 0.45 sat, knee = 0.05 + 0.35 sat, asymmetry = 0.10 sat.  A sample
 * with |x| <= threshold - knee (and a NaN) passes unchanged.  The reference clips callback by callback with two arithmetic paths,
 * and so does this stage, bit for bit: sample i of a callback of len samples takes the 4-wide body while i < len / 4 * 4
 * (reciprocals of the knee, three fused multiply-adds, the Pade tanh on an argument clamped to +-4.5) and the scalar tail after
 * that (true divisions, nothing fused, tanh = +-1 beyond 4.5).  An infinity becomes a NaN on either path.
 *   factor > 1   in place on the oversampled block, one callback = block_size samples at the processing rate
 *   factor 1     a local 2x pair around it (softClipOS: one half-band stage of 31 taps at 90 dB, the design of the third
 *                CPQ_OS_IIR stage, driven like the main oversampler: histories, guards, auto-clear and hard fallback -- a stream
 *                in hard fallback delivers silence -- and the 3/4 pass-band gain of an up / down pair), one callback =
 *                2 * block_size samples; the pair delays the stream by 15 base-rate samples
 * The ragged last chunk of a CPQ_CALLS_ANY call is a callback of its own length.  The stage runs inside
 * cpq_engine_process_block[_device] and the PCM calls, before the output stage, the meters, the dither stage and the pack.
 * Not built: the 1 Hz DC blocker on the oversampled block, the full-bypass dry blend, the fade-in, the fixed latency delay. */
/* threshold, knee and asymmetry of an amount; CPQ_ERR_INVALID_ARG for a null pointer or an amount that is not finite or
 * outside 0 .. 1, the range the reference's setSaturationAmount admits.  Host only. */
int32_t cpq_soft_clip_params(float saturation_amount, double* threshold, double* knee, double* asymmetry);
/* The reference's walk over one row in place on the host, sequentially: n_samples in callbacks of callback_len (the last one
 * shorter).  The statement the kernel is tested against.  Host only. */
int32_t cpq_soft_clip_host(double* data, int32_t n_samples, int32_t callback_len, float saturation_amount);
/* base-rate samples the stage adds: 15.0 at factor 1 (the local 2x pair), 0.0 at any other factor.  Host only. */
double  cpq_soft_clip_latency(int32_t factor);
/* One stream or CPQ_ALL_STREAMS: enabled != 0 clips with the amount, 0 lets the stream's rows pass untouched (the amount is
 * kept).  The default is off for every stream; while no stream clips nothing is launched or allocated and the engine's output
 * is what it was without this call.  CPQ_ERR_INVALID_ARG for a stream out of range or an amount that is not finite or outside
 * 0 .. 1, before any state moves.  A change of `enabled` of any stream clears the local 2x stage's histories and flags of every
 * stream, as do cpq_engine_prepare and cpq_engine_set_oversampling; a change of the amount alone does not.  Synchronises the
 * engine's stream. */
int32_t cpq_engine_set_soft_clip(cpq_engine* e, int32_t stream, int32_t enabled, float saturation_amount);
/* histories and flags of the local 2x stage to zero (its counters stay).  CPQ_ERR_NOT_READY while no stream clips (so for the
 * two calls below). */
int32_t cpq_soft_clip_reset(cpq_engine* e);
/* The kernel alone on caller rows [channel][n_samples] with the engine's table: n_samples is 1 .. block_size *
 * max_blocks_per_call, callback_len >= 1 is the callback length to walk them in (any value: the rows are at whatever rate the
 * caller says).  in and out may be the same buffer; both 16-byte aligned.  _device: device pointers, enqueued on the engine's
 * stream, no synchronisation.  The local 2x pair is not run.  Every refusal happens before anything is enqueued. */
int32_t cpq_soft_clip_process(cpq_engine* e, const double* in, double* out, int32_t n_samples, int32_t callback_len);
int32_t cpq_soft_clip_process_device(cpq_engine* e, const double* d_in, double* d_out, int32_t n_samples, int32_t callback_len);
/* cpq_os_read_telemetry for the local 2x stage: its own events, auto-clears and hard fallback; all zero before it first ran */
int32_t cpq_soft_clip_read_telemetry(cpq_engine* e, int32_t stream, cpq_os_telemetry* out);

/* ---------------------------------------------------------------- output stage */
/* The base-rate steps DSPCore::processOutputDouble runs on the chain's result when dither is off
 * (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:577-744), in its order:
 *   CPQ_OUT_DC_BLOCK   the 3 Hz output UltraHighRateDCBlocker (src/UltraHighRateDCBlocker.h): two one-pole sections at 2.7 and
 *                      3.3 Hz, s += alpha (x - s), x -= s; at the end of every callback a state that is not finite or not below
 *                      1e15 becomes 0
 *   CPQ_OUT_HEADROOM   x *= 0.8912509381337456 (kOutputHeadroom, -1 dBFS), then the scrub: not finite or |x| >= 1e300 becomes 0,
 *                      written into the delivered rows
 *   CPQ_OUT_LIMITER    SimplePeakLimiter (src/audioengine/SimplePeakLimiter.h): threshold 0.8413951287507587, knee 0.108748,
 *                      release 100 ms, one envelope per stream carried across callbacks and calls
 *   CPQ_OUT_CLAMP      min(max(x, -0.8912509381337456), 0.8912509381337456) as the reference's 4-wide body computes it (a NaN,
 *                      which only a stage without CPQ_OUT_HEADROOM can meet, becomes the lower limit)
 * The stage runs on the base-rate rows at the end of cpq_engine_process_block[_device] and of the PCM calls: after the
 * oversampler's down stages, before the pack, one callback = block_size / factor samples (the ragged last chunk of a
 * CPQ_CALLS_ANY call is a callback of its own length).  With the stage on the meters read where the reference's do: after the
 * scrub, before the limiter.  The soft clipper (the section above) runs before this stage.  Not built: the fade-in, the fixed
 * latency delay (dither: the next section). */
#define CPQ_OUT_DC_BLOCK 1
#define CPQ_OUT_HEADROOM 2
#define CPQ_OUT_LIMITER  4
#define CPQ_OUT_CLAMP    8
#define CPQ_OUT_ALL      15

/* UltraHighRateDCBlocker::init(rate, 3.0) -> alpha[2] and SimplePeakLimiter::prepare(rate, 100.0) -> *release_coeff, with the
 * reference's fallbacks for a rate that is not positive and finite (alpha 1e-6, release 0).  Host only. */
int32_t cpq_out_design(double rate, double alpha[2], double* release_coeff);
/* flags: 0 = off (the default: the rows leave the engine as they always did), or CPQ_OUT_* bits; any other bit is
 * CPQ_ERR_INVALID_ARG.  Applies to every stream.  The coefficients are designed for the base rate sample_rate / factor;
 * cpq_engine_prepare, cpq_engine_set_oversampling and any change of the flags redesign them, clear the DC states and set the
 * envelopes to 1.0. */
int32_t cpq_engine_set_output_stage(cpq_engine* e, int32_t flags);
/* DC states to 0, envelopes to 1.0.  CPQ_ERR_NOT_READY while the stage is off (so for the four calls below). */
int32_t cpq_out_reset(cpq_engine* e);
/* The stage alone on caller rows [channel][n_samples], exactly as the engine's output would pass it (the meters are not run):
 * n_samples is 1 .. block_size * max_blocks_per_call / factor, whole callbacks unless the engine takes CPQ_CALLS_ANY.  in and
 * out may be the same buffer.  _device: device pointers, enqueued on the engine's stream, no synchronisation.  Every refusal
 * happens before any state moves. */
int32_t cpq_out_process(cpq_engine* e, const double* in, double* out, int32_t n_samples);
int32_t cpq_out_process_device(cpq_engine* e, const double* d_in, double* d_out, int32_t n_samples);
/* synchronises the engine's stream; *envelope = the limiter's envelope of one stream */
int32_t cpq_out_read_envelope(cpq_engine* e, int32_t stream, double* envelope);

/* ---------------------------------------------------------------- dither stage */
/* processOutputDouble's ditherBitDepth > 0 branch (DSPCoreDouble.cpp:644-654) for the reference's three deterministic shapers:
 * the shaper's processStereoBlock(l, r, n, headroom) takes the place of the plain headroom multiply; scrub, meters, limiter and
 * clamp follow as without it, so the limiter acts after quantisation and a limited sample leaves the grid.
 *   CPQ_DITHER_FIXED4   FixedNoiseShaper (src/FixedNoiseShaper.h): 4 error taps, xoshiro256++ seeded with the header's constants
 *                       (channel 0 for L, channel 1 for R); its prepare() / reset() do not reseed
 *   CPQ_DITHER_FIXED15  Fixed15TapNoiseShaper (src/Fixed15TapNoiseShaper.h): ORDER 16 (the sixteenth coefficient is 0.0), seeded
 *                       by splitmix64 over (rate, bit depth) in every prepare()
 * Per sample and channel: x = in * headroom; fb = sum c[k] e[k] (e[0] the newest stored error; 4 taps: one expression, left to
 * right; 15 taps: fb = 0.0, fb += c[k] e[k]; no contraction); y = x - fb; v = clamp(y, -1, 1 - scale) + (u1 + u2 - 1) * scale
 * with u = (xoshiro256++ >> 11) * 2^-53, u1 drawn first; yq = rint(v * invScale) (ties to even) * scale; the stored error is
 * yq - y clamped to +-2 scale.  scale = 2^-(bits - 1).  Non-finite values: the 4-tap shaper replaces a non-finite y by 0 before
 * the clamp and a non-finite result by 0, its stored error passes std::clamp (a NaN stays) and then becomes 0 when not finite;
 * the 15-tap shaper has no such guards (a NaN in is a NaN out), clamps the rounded code to [-invScale, invScale - 1] with
 * std::clamp, and its stored error passes max_sd / min_sd, which turn a NaN into -2 scale.  The coefficients are prepare()'s: ten
 * presets (44.1 ... 768 kHz), linear interpolation in the rate between them, the first and the last preset outside.
 * Every stream is a DSPCore of its own: all streams draw the same two sequences (L, R).
 * Headroom is 0.8912509381337456 with CPQ_OUT_HEADROOM in the output-stage flags, else 1.0; the scrub runs only with that flag.
 *   CPQ_DITHER_ADAPTIVE9  LatticeNoiseShaper (src/LatticeNoiseShaper.h), NoiseShaperType::Adaptive9thOrder: a 9-stage lattice on
 *                       the stored error, the 4-tap header's two constant generator states (prepare() / reset() do not reseed),
 *                       and nine reflection coefficients of the stream's own
 * Per sample and channel, with states s[0..8] and the stream's coefficients c[0..8]: x = in * headroom;
 * p_j = fma(s[4+j], c[4+j], s[j] * c[j]) for j = 0..3 (computeFeedback's _mm256_fmadd_pd, a real fused multiply-add);
 * fb = ((p_0 + p_2) + (p_1 + p_3)) + s[8] * c[8] (nothing else contracted); y = x + fb; v = y clamped to [-1, 1 - scale] by two
 * comparisons (a NaN passes both), plus (u1 + u2 - 1) * scale; q = rint(v * invScale) clamped to [-invScale, invScale - 1] with
 * std::clamp (a NaN stays); yq = q * scale is the output; err = yq - y, 0 when not finite, clamped to +-2 scale; then f = err and
 * for i = 0..8: b = s[i], nf = f + c[i] * b, s[i] = clamp(c[i] * f + b, -2, 2), f = nf.  A NaN input is a NaN output for that
 * sample only, +-inf clamps to the rails, and in both cases the stored error is 0, so the states stay finite.
 * processStereoBlock's closing clampStateSIMD (+-1e12) cannot act on states already held to +-2 and is not built.
 * Coefficients: every stream starts from kDefaultAdaptiveNoiseShaperCoeffs (DSPCoreLifecycle.cpp:32-35);
 * cpq_dither_set_adaptive_coeffs is the learner's published set reaching the shaper (applyMatchedCoefficients at the start of a
 * callback, DSPCoreDouble.cpp:617-628).  Which set to publish -- the reference keeps one per sample-rate bank
 * (kAdaptiveNoiseShaperSampleRateBankCount = 10, 44.1 ... 768 kHz), bit depth and learning mode -- is the caller's lookup.
 * Not built: the psychoacoustic shaper (it draws from MKL's SFMT19937 stream), the learner itself, the shapers' diagnostics, the
 * 15-tap errorEnvelope / needsReset handshake (finite input cannot raise it). */
#define CPQ_DITHER_OFF       0
#define CPQ_DITHER_FIXED4    1
#define CPQ_DITHER_FIXED15   2
#define CPQ_DITHER_ADAPTIVE9 4  /* 3 stays unassigned and refused */
#define CPQ_DITHER_TILE    64   /* samples a workgroup of k_dither moves through LDS at a time (tests walk its edges) */
/* prepare(rate, bit_depth) of the shaper: coeffs[16] (the 4-tap shaper fills 4, the rest 0.0) and *scale.  bit_depth 1 .. 32.
 * CPQ_DITHER_ADAPTIVE9: the default set in coeffs[0..8], the rest 0.0; the rate is ignored, as its prepare(bitDepth) takes none.
 * Host only. */
int32_t cpq_dither_design(double rate, int32_t shaper, int32_t bit_depth, double coeffs[16], double* scale);
/* shaper CPQ_DITHER_OFF (the default: nothing is launched, bit_depth ignored) or one of the three shapers with bit_depth 1 .. 32;
 * anything else is CPQ_ERR_INVALID_ARG before any state moves.  The same arguments again change nothing; any change clears the
 * errors and reseeds, and gives every stream of the adaptive shaper the default set.  The rate is sample_rate / oversampling
 * factor: cpq_engine_prepare and cpq_engine_set_oversampling redesign the coefficients and clear the errors; they reseed the
 * 15-tap shaper only, as the reference's prepare() does.  The adaptive shaper keeps each stream's coefficients across them (the
 * reference applies the published set again at the first callback after DSPCore::prepare) and its states are cleared. */
int32_t cpq_engine_set_dither(cpq_engine* e, int32_t shaper, int32_t bit_depth);
/* the shaper's reset(): errors (the lattice's states) to 0, the generators run on, coefficients stay.  CPQ_ERR_NOT_READY while
 * dither is off (so for the calls below). */
int32_t cpq_dither_reset(cpq_engine* e);
/* applyMatchedCoefficients(k, n) for one stream or CPQ_ALL_STREAMS: the coefficients become clampCoeff(k[i]) (not finite -> 0,
 * else clamped to +-0.85) for i < n and 0 from n on, and those streams' states are cleared; other streams and every generator
 * are left alone.  Acts on the next call.  CPQ_ERR_NOT_READY unless the adaptive shaper is on; CPQ_ERR_INVALID_ARG for a stream
 * out of range, n outside 0 .. 9 or a null k with n > 0; every refusal happens before any state moves. */
int32_t cpq_dither_set_adaptive_coeffs(cpq_engine* e, int32_t stream, const double* k, int32_t n);
/* k[0..8] = the clamped coefficients stream `stream` (an index, not CPQ_ALL_STREAMS) runs with; refusals as above */
int32_t cpq_dither_get_adaptive_coeffs(const cpq_engine* e, int32_t stream, double k[9]);
/* The stage alone (headroom, shaper, scrub if flagged) on caller rows, with the argument rules of cpq_out_process. */
int32_t cpq_dither_process(cpq_engine* e, const double* in, double* out, int32_t n_samples);
int32_t cpq_dither_process_device(cpq_engine* e, const double* d_in, double* d_out, int32_t n_samples);

/* ------------------------------------------------------- packed PCM in and out */
/* The whole-chain call with a converter at each end: float32 or integer PCM, planar or interleaved, instead of fp64 rows.
 * What the reference does around its chain in float (DSPCore::processInput -> convertFloatToDoubleHighQuality,
 * src/InputBitDepthTransform.h:102-121; processOutput's final static_cast<float>,
 * src/audioengine/AudioEngine.Processing.DSPCoreIO.cpp:532-537) and what a file reader does before it.  All conversions are exact
 * statements, there is no tolerance:
 *   in,  F32          (double)x
 *   in,  S16/S24/S32  the JUCE reader's convention, as cpq_ir_load_wav decodes: left-justified to 32 bits, converted to float
 *                     (round to nearest), times 1.0f / (float)0x7fffffff (= 2^-31) in float arithmetic, widened to double.
 *                     S16 and S24 are therefore exact; S32 is rounded to 24 significant bits, as the reference's reader does.
 *   in,  F64          a copy (planar) or a de-interleave
 *   CPQ_PCM_SANITIZE  input_transform::applyHighQuality64BitTransform(gain = 1) on the widened input, per callback of
 *                     block_size / oversampling factor base-rate samples (the ragged last chunk of a CPQ_CALLS_ANY call is a
 *                     callback of its own length): NaN and |v| < 1e-20 become +0.0, the rest is clamped to [-1, 1]; an infinity
 *                     clamps to +-1 in the 4-wide body of a callback and becomes 0 in its scalar tail, the last len % 4 samples.
 *                     Without the flag the widened value goes in untouched, as the fp64 entry point takes it.
 *   out, F32          static_cast<float>: round to nearest even, overflow to +-inf, NaN stays NaN
 *   out, S24/S32      rint(x * 2^(b-1)), ties to even, saturated to [-2^(b-1), 2^(b-1) - 1], NaN -> 0; S24 as three
 *                     little-endian bytes
 *   out, F64          a copy or an interleave
 *   out, S16          only while the dither stage is on with bit_depth <= 16 (cpq_engine_set_dither): the S24 rule at 16 bits,
 *                     which is exact on rows the shaper quantised and the limiter left alone; otherwise CPQ_ERR_UNSUPPORTED
 *                     and the destination is untouched
 * Packed buffers are aligned to their element (S24: any byte), fp64 rows to 8 bytes; the buffers of
 * cpq_engine_process_block_pcm[_device] to 16 bytes like those of cpq_engine_process_block.  No byte outside
 * [base, base + bytes) of a buffer is read or written. */
typedef enum { CPQ_PCM_F64 = 0, CPQ_PCM_F32 = 1, CPQ_PCM_S16 = 2, CPQ_PCM_S24 = 3 /* packed, 3 bytes, LE */, CPQ_PCM_S32 = 4 } cpq_pcm_format;
typedef enum { CPQ_PCM_PLANAR = 0      /* [2 S][n], the existing row order */,
               CPQ_PCM_INTERLEAVED = 1 /* [S][n][2]: stereo frames per stream, as in a file */ } cpq_pcm_layout;
#define CPQ_PCM_SANITIZE 1u   /* flags bit */

int32_t cpq_pcm_bytes_per_sample(int32_t format);                 /* host only; -1 for an unknown format */
/* The converters alone on caller buffers (host pointers; _device: device pointers, enqueued on the engine's stream, no
 * synchronisation): pcm -> rows [2 S][n] and rows -> pcm.  n is 1 .. block_size * max_blocks_per_call. */
int32_t cpq_pcm_unpack(cpq_engine* e, const void* pcm, int32_t format, int32_t layout, uint32_t flags, double* rows, int32_t n);
int32_t cpq_pcm_unpack_device(cpq_engine* e, const void* d_pcm, int32_t format, int32_t layout, uint32_t flags, double* d_rows, int32_t n);
int32_t cpq_pcm_pack(cpq_engine* e, const double* rows, void* pcm, int32_t format, int32_t layout, int32_t n);
int32_t cpq_pcm_pack_device(cpq_engine* e, const double* d_rows, void* d_pcm, int32_t format, int32_t layout, int32_t n);
/* cpq_engine_process_block with the converters around it: the same routing, oversampling and metering (the meters read the
 * fp64 rows the chain delivered, before packing), the same n_samples rules (base-rate samples on both sides with
 * oversampling).  in and out may be the same buffer only when in_format == out_format; any other overlap of the two byte
 * ranges is CPQ_ERR_INVALID_ARG.  Every refusal happens before any state moves or anything is enqueued. */
int32_t cpq_engine_process_block_pcm(cpq_engine* e, const void* in, int32_t in_format, void* out, int32_t out_format,
                                     int32_t layout, uint32_t flags, int32_t n_samples);
int32_t cpq_engine_process_block_pcm_device(cpq_engine* e, const void* d_in, int32_t in_format, void* d_out, int32_t out_format,
                                            int32_t layout, uint32_t flags, int32_t n_samples);

/* ---------------------------------------------------------------- word-length reduction of delivered rows */
/* cpq_quantizer: the last step of a delivery -- engine -> cpq_loudness -> cpq_limiter -> cpq_quantizer -- as an object of its own
 * beside the engine: the stream's gain, a noise shaper and the PCM pack of fp64 rows in one pass, after every gain the chain
 * applies.  n_streams stereo programmes at once, rows planar float64 at (2 s + channel) * stride + i, as cpq_limiter writes
 * them.  Per call, channel and sample:
 *     u  = x * gains[s]                  one rounding, nothing scrubbed (cpq_loudness_apply_device's rule); gains default to 1.0
 *     yq = the shaper's processSample(u) exactly the text of "dither stage" above for CPQ_DITHER_FIXED4, CPQ_DITHER_FIXED15 or
 *                                        CPQ_DITHER_ADAPTIVE9 at bit_depth, headroom 1.0, no scrub
 *     b  = the "out, S24/S32" rule of "packed PCM in and out" at the width w of the container (16, 24 or 32):
 *          rint(yq * 2^(w-1)), ties to even, saturated to [-2^(w-1), 2^(w-1) - 1], NaN -> 0
 * and b is written as w / 8 little-endian bytes: CPQ_PCM_PLANAR, sample i of channel c at c * pcm_pitch_bytes + i * w / 8;
 * CPQ_PCM_INTERLEAVED, sample i of channel ch of stream s at s * pcm_pitch_bytes + (2 i + ch) * w / 8.  pcm_pitch_bytes is the
 * caller's, at least the width of a packed row (n_samples * w / 8, twice that interleaved); the bytes of a pitch gap are
 * neither read nor written, and none outside a row's [base, base + width).  With bit_depth <= w the pack is exact for every
 * value a shaper can emit with one exception: the 4-tap shaper does not clamp its code, so it can emit +1.0, which saturates to
 * 2^(w-1) - 1 at every bit_depth (and, where both draws are 0, -1 - 2^-(bit_depth-1), which saturates to -2^(w-1) at
 * bit_depth == w); the saturation is part of the definition.
 * Design and seeds are cpq_dither_design's and the dither stage's at sample_rate and bit_depth, and every stream draws the same
 * two sequences (L, R): at gain 1.0 the bytes equal what cpq_dither_process_device followed by cpq_pcm_pack_device give on an
 * engine with the same shaper, bit depth and rate.  Error taps or lattice states and the generator words are carried over
 * calls, so the bytes of a programme are the same for every split into calls, and equal from the object that computes on the
 * host (CPQ_QUANT_HOST, no GPU needed) and the one that computes on the device (CPQ_QUANT_DEVICE, one gfx950 kernel per call;
 * DESIGN.md 4.19).  Neither object ever stands in for the other.
 *
 * cpq_quantizer_create refuses, in this order: a null out, n_streams outside 1 ... 32767, unknown flags, both flags, a
 * sample_rate that is not finite and > 0, a shaper that is none of the three, a container_format that is not CPQ_PCM_S16,
 * CPQ_PCM_S24 or CPQ_PCM_S32, a bit_depth outside 1 ... 32 (all CPQ_ERR_INVALID_ARG); a bit_depth above the container's width,
 * then flags == 0 (the caller says where the bytes are computed; both CPQ_ERR_UNSUPPORTED); CPQ_QUANT_DEVICE without a gfx950
 * device (CPQ_ERR_NO_DEVICE).  The reason of a refused create is in cpq_last_error(NULL). */
#define CPQ_HAS_QUANTIZER 1
#define CPQ_QUANT_HOST   1u
#define CPQ_QUANT_DEVICE 2u
typedef struct cpq_quantizer cpq_quantizer;
int32_t cpq_quantizer_create(int32_t n_streams, double sample_rate, int32_t shaper, int32_t bit_depth, int32_t container_format,
                             uint32_t flags, cpq_quantizer** out);
void cpq_quantizer_destroy(cpq_quantizer* p);
const char* cpq_quantizer_last_error(const cpq_quantizer* p);
/* Device object only (a host object: CPQ_ERR_INVALID_ARG).  Synchronises the stream used so far, then later calls enqueue on
 * `stream` (a hipStream_t; NULL: the null stream). */
int32_t cpq_quantizer_set_stream(cpq_quantizer* p, void* stream);
/* The object is as new: errors (the lattice's states) cleared, generators reseeded, the sample count 0.  Gains and adaptive
 * coefficients stay.  On a device object it synchronises the stream. */
int32_t cpq_quantizer_reset(cpq_quantizer* p);
/* gains[n_streams] (default 1.0; they stay over reset).  Refused in this order: a null object (no message) or null gains, a
 * gain that is not finite or is negative (CPQ_ERR_INVALID_ARG), a programme that has started (CPQ_ERR_NOT_READY: reset first).
 * On a device object it synchronises the stream. */
int32_t cpq_quantizer_set_gains(cpq_quantizer* p, const double* gains);
/* cpq_dither_set_adaptive_coeffs / cpq_dither_get_adaptive_coeffs on this object, with their rules: the set a cpq_learner
 * publishes reaches a delivery.  One stream or CPQ_ALL_STREAMS takes clampCoeff(k[i]) for i < n and 0 from n on, and those
 * streams' states are cleared; other streams and every generator are left alone; allowed in the middle of a programme, acts on
 * the next call.  CPQ_ERR_NOT_READY unless the object runs CPQ_DITHER_ADAPTIVE9; CPQ_ERR_INVALID_ARG for a stream out of range,
 * n outside 0 .. 9 or a null k with n > 0; every refusal happens before any state moves.  On a device object set synchronises
 * the stream. */
int32_t cpq_quantizer_set_adaptive_coeffs(cpq_quantizer* p, int32_t stream, const double* k, int32_t n);
int32_t cpq_quantizer_get_adaptive_coeffs(const cpq_quantizer* p, int32_t stream, double k[9]);
/* n_samples more of every programme, device rows in and device bytes out, asynchronous on the object's stream: d_in must stay
 * as it is until that stream has reached the call.  layout is a cpq_pcm_layout.  Refused before any state moves, in this
 * order, all CPQ_ERR_INVALID_ARG: a null object (no message), a host object, a null buffer, n_samples outside 1 ... 2^30, an
 * unknown layout, in_stride below n_samples or pcm_pitch_bytes below the width of a packed row, d_in not 16-byte aligned, d_pcm
 * or pcm_pitch_bytes not aligned to the element (2 or 4 bytes; S24: any byte), the byte range of the rows and that of the
 * packed buffer overlapping.  CPQ_ERR_DEVICE: a launch failed. */
int32_t cpq_quantizer_process_device(cpq_quantizer* p, const double* d_in, int64_t in_stride, void* d_pcm, int64_t pcm_pitch_bytes,
                                     int32_t layout, int32_t n_samples);
/* The same on host buffers, on either object (the device object copies through buffers it owns and synchronises); the same
 * refusals in the same order without the host-object rule, and `in` on 8 bytes instead of 16. */
int32_t cpq_quantizer_process(cpq_quantizer* p, const double* in, int64_t in_stride, void* pcm, int64_t pcm_pitch_bytes, int32_t layout,
                              int32_t n_samples);
/* Device time of the launch of the last call of a device object, waiting for it; -1 on a host object or before a call. */
double cpq_quantizer_last_kernel_ms(cpq_quantizer* p);

/* ---------------------------------------------------------------- profiling */
/* Per-kernel HIP-event timing on the engine's stream (counterpart of the reference's CONV_TIME /
 * EQ_TIME diagnostics, src/convolver/ConvolverProcessor.Runtime.cpp:679-721). */
typedef enum {
    CPQ_K_RFFT_FWD = 0,   /* k_rfft_fwd_ols */
    CPQ_K_FDL_MAC  = 1,   /* k_fdl_mac      */
    CPQ_K_DCNYQ    = 2,   /* k_fdl_mac_dcnyq */
    CPQ_K_RFFT_INV = 3,   /* k_rfft_inv_ols */
    CPQ_K_SVF      = 4,   /* k_svf_cascade (lane-skewed sequential recurrence) */
    CPQ_K_SVF_TP   = 5,   /* the time-parallel cascade kernels (k_svf_cascade_tpv / _short; default) */
    CPQ_K_MIX      = 6,   /* k_convproc_mix (processor-level dry/wet stage) */
    CPQ_K_OUTFILT  = 7,   /* output-filter biquad cascade (k_svf_cascade_tp / k_svf_cascade running DF-II-T sections) */
    CPQ_K_OS       = 8,   /* half-band oversampler stages, up and down (k_os_interp / k_os_decim and their helpers) */
    CPQ_K_METER    = 9,   /* loudness and true-peak meters (k_meter_kweight / k_meter_true_peak / k_meter_finish) */
    CPQ_K_PCM      = 10,  /* packed PCM converters (k_pcm_unpack / k_pcm_pack) */
    CPQ_K_OUT      = 11,  /* output stage (k_out_pre / k_out_headroom / k_out_post) */
    CPQ_K_DITHER   = 12,  /* dither stage (k_dither, k_dither_lattice) */
    /* 13 stays unassigned: cpq_kernel_name(13) has answered "?" since the dither stage and keeps doing so; its counters read 0 */
    CPQ_K_SOFTCLIP = 14,  /* soft clipper (k_soft_clip); its local 2x pair at factor 1 counts under CPQ_K_OS */
    CPQ_K_COUNT    = 15
} cpq_kernel_id;
int32_t     cpq_profile_enable(cpq_engine* e, int32_t on);
int32_t     cpq_profile_reset(cpq_engine* e);
/* synchronises the stream, then returns launches and summed milliseconds of one kernel */
int32_t     cpq_profile_read(cpq_engine* e, int32_t kernel_id, int64_t* launches, double* total_ms);
const char* cpq_kernel_name(int32_t kernel_id);

/* ---------------------------------------------------------------- diagnostics (all defined in csrc/engine_diag.cpp) */
/* The partition FFT on its own (what replaces ProductionFft::forwardRealToCCS / inverseCCSToR, src/FFTBackend.cpp:123-150,
 * inside processLayerBlock): for n_channels x n_blocks blocks of `partition` samples (host, [channel][block][sample]; the
 * history before block 0 is silence) the forward transform of every overlap-save frame [previous block | block]
 * (2 * partition real points, unscaled) and the inverse transform of those spectra (scaled 1 / (2 * partition)), second half.
 * spectra: [channel][block][partition][2] in the kernels' own storage order -- element 0 = (DC, Nyquist), both real; element
 * e = bin e for partition <= 2048; for larger partitions element k1 * 512 + k2 = bin k1 + (partition / 512) * k2.
 * out: [channel][block][sample], equals the input up to rounding.  partition: a power of two in 64 ... 131072.
 * Needs a gfx950 device; no engine.  For tests of the FFT kernel families in isolation. */
int32_t     cpq_diag_partition_fft(int32_t partition, int32_t n_channels, int32_t n_blocks, const double* in,
                                   double* spectra, double* out);
/* The same with the work split of the partition = 4096 kernels chosen by the caller: `split` workgroups (1 ... n_blocks) walk
 * the blocks of a channel, each a contiguous range of ceil(n_blocks / split) blocks (the last ranges may be shorter or empty),
 * so that a small test decides how many consecutive frames one workgroup transforms.  split <= 0 or partition != 4096: the
 * engine's own choice, i.e. cpq_diag_partition_fft.  The results do not depend on split. */
int32_t     cpq_diag_partition_fft_split(int32_t partition, int32_t n_channels, int32_t n_blocks, int32_t split,
                                         const double* in, double* spectra, double* out);
/* The FDL multiply-accumulate on its own (what replaces the per-partition accumulateSplitComplex loop,
 * src/MKLNonUniformConvolver.cpp:150-195): exactly the launches an engine makes for one call, on buffers the caller fills.
 *   y[c][t][b] = sum_{k < k_parts} x[c][(head + t - k) & (ring_slots - 1)][b] * h[ir_slot[c]][k][b]     (complex, b >= 1)
 *   y[c][t][0] = ( sum_k Re x Re h , sum_k Im x Im h )              (element 0 packs DC and Nyquist, two real products)
 * x: [n_channels][ring_slots][partition][2], the whole delay-line ring; h: [n_ir_slots][h_rows][partition][2];
 * ir_slot: [n_channels]; y: [n_channels][n_blocks][partition][2]; all host memory.  The compact DC/Nyquist rows the 16- and
 * 32-row tiles read are formed from element 0 of x and h.
 * tile: 0 = automatic (by n_blocks), 4 / 8 / 16 / 32 = that register tile, -1 = the workgroup-cooperative kernel at any
 * n_blocks (no engine selects it below 48 blocks), -2 = the same kernel with 128-row workgroups at any n_blocks (no engine
 * selects it).  *variant_used = the kernel that ran: 4 / 8 / 16 / 32, 0 for the cooperative kernel, 128 for its 128-row
 * workgroups.  h_private != 0: no two channels share an IR slot (one-tile calls may then stream the IR rows).
 * Rows k_parts ... h_rows - 1 of a slot, IR slots no channel names and ring slots outside {head + t - k} may hold anything
 * finite: they may be loaded, never consumed.
 * CPQ_ERR_INVALID_ARG, before anything is launched, unless: partition is a power of two in 64 ... 4096; n_channels, k_parts,
 * n_blocks, n_ir_slots >= 1; tile is one of the values above; ring_slots is a power of two >= nextPow2(alignUp(k_parts, 32) +
 * 32 + n_blocks) (the engines' ring size); h_rows >= alignUp(k_parts, 32) + 16 (the engines' smallest slot); 0 <= head <
 * ring_slots; 0 <= ir_slot[c] < n_ir_slots; no buffer above 2^28 elements.
 * Needs a gfx950 device; no engine.  For tests of the MAC kernel variants in isolation. */
int32_t     cpq_diag_fdl_mac(int32_t partition, int32_t n_channels, int32_t k_parts, int32_t n_blocks, int32_t tile,
                             int32_t head, int32_t ring_slots, int32_t n_ir_slots, int32_t h_rows, int32_t h_private,
                             const double* x, const double* h, const int32_t* ir_slot, double* y, int32_t* variant_used);
/* The launch variants of the partition transforms on their own (tests/test_gpu_fft_variants.py): the launches an engine makes
 * around cpq_diag_partition_fft's plain rows -- a moving ring head and a carried history, the side copies of the 512-sample
 * forward transform, the three store modes of the inverse transform, the IR spectra and their spectral gain.  All pointers are
 * host memory; spectra are in the storage order described at cpq_diag_partition_fft.  Every buffer a kernel may write is
 * filled with 0xFF bytes (NaN; -1 in the table) before the launch, unless the caller supplies its contents, and is returned
 * whole, so that what a launch leaves alone can be told from what it stores.  Each entry returns CPQ_ERR_INVALID_ARG, before
 * anything is allocated or launched (and before a device is looked for), for every argument set with which a kernel would read
 * or write outside a buffer or a launcher's precondition would not hold.  "partition" below: a power of two in 64 ... 131072;
 * no buffer may exceed 2^28 elements.  Need a gfx950 device; no engine.
 *
 * Forward (launch_rfft_fwd_ols; side != 0: launch_rfft_fwd_ols_side).  in: [n_channels][n_blocks * partition + tail_len] (the
 * device rows are padded to an even length), hist_old: [n_channels][partition], the block in front of block 0.  Block t of
 * channel c is transformed as the frame [block t - 1 | block t] into slot (head + t) & (ring_slots - 1) of
 * ring: [n_channels][ring_slots][partition][2]; xdn: [n_channels][ring_slots][2] receives element 0 of every slot written;
 * hist_new: [n_channels][partition] the last block.
 *   side != 0 also: n_side <= 2 destinations side_out0 / side_out1: [n_channels][side_stride[a]], block t of channel c copied
 *   to [c][side_off[a] + t * partition ...); tab_out: [64] receives tab[0 .. n_tab); tail_out: [n_channels][tail_stride] receives
 *   the tail_len samples behind the blocks of every input row.
 * Refused unless: n_channels, n_blocks >= 1; ring_slots a power of two >= n_blocks; 0 <= head < ring_slots; side == 0:
 * tail_len == 0; side != 0: partition == 512, 0 <= n_side <= 2, side_stride[a] and side_off[a] even (the launcher's
 * rfft_fwd_can_carry_side), 0 <= side_off[a], side_off[a] + n_blocks * partition <= side_stride[a], 0 <= n_tab <= 64,
 * 0 <= tail_len <= tail_stride, tail_stride >= 1, every pointer that is used non-null. */
int32_t     cpq_diag_fft_forward(int32_t partition, int32_t n_channels, int32_t n_blocks, int32_t head, int32_t ring_slots,
                                 int32_t tail_len, const double* in, const double* hist_old, int32_t side, int32_t n_side,
                                 const int64_t* side_stride, const int64_t* side_off, const int64_t* tab, int32_t n_tab,
                                 int32_t tail_stride, double* ring, double* xdn, double* hist_new, double* side_out0,
                                 double* side_out1, int64_t* tab_out, double* tail_out);
/* Inverse transform of spectra: [n_channels][n_blocks][partition][2] (second half of every frame, scaled 1 / (2 * partition)),
 * stored by
 *   mode 1 (launch_rfft_inv_ols_ring): sample i of block t to ring_a[c][(p_t + i) & (ring_a_size - 1)], p_t = pos_a[t] (a
 *     negative entry drops the block) or pos0 + t * partition when pos_a is null.  ring_a: [n_channels][ring_a_size], in and out.
 *   mode 2 (launch_rfft_inv_ols_tail): to out: [n_channels][n_blocks * partition] plus what the delay-line reader of n_tail tail
 *     layers adds there: for sample n of the call, callback n / callback_size, layer l (gain g1, then g2): s = sched[l][callback];
 *     s >= 0 adds x (gain within 1e-12 of 1) or x * gain, x = layer_out[l][c][s + n % callback_size - g0] when that index is
 *     >= 0, else tail_ring[l][c][(s + n % callback_size) & (tail_ring_size - 1)]; g0 = tail_state[3].  layer_out: [n_tail]
 *     [n_channels][n_blocks * partition], tail_ring: [n_tail][n_channels][tail_ring_size], sched: [n_tail][n_blocks * partition
 *     / callback_size], tail_state: [4].
 *   mode 3 (launch_rfft_inv_ols_add, partition 512): to out plus, for block t, ring_a[c][(pos_a[t] + i) & mask] (gain g1) and then
 *     ring_b[c][(pos_b[t] + i) & mask] (gain g2; ring_b may be null); negative positions add nothing.  The rings come back as
 *     they are after the launch.
 * Refused unless: n_channels, n_blocks >= 1; mode 1: ring_a_size a power of two >= partition and >= 2, positions <= 2^62,
 * 0 <= pos0 when pos_a is null, the blocks that are written at least a partition apart on the ring (no element stored twice);
 * mode 2: partition <= 4096, n_tail 1 or 2, callback_size a power of two dividing n_blocks * partition, tail_ring_size a power
 * of two >= 2, 0 <= g0 <= 2^62, every entry s >= 0 of sched with s + callback_size <= g0 + n_blocks * partition; mode 3:
 * partition == 512, ring sizes powers of two >= partition, positions <= 2^62, pos_a non-null, pos_b non-null with ring_b. */
int32_t     cpq_diag_fft_inverse_store(int32_t mode, int32_t partition, int32_t n_channels, int32_t n_blocks, const double* spectra,
                                       double* ring_a, int32_t ring_a_size, const int64_t* pos_a, int64_t pos0, double* ring_b,
                                       int32_t ring_b_size, const int64_t* pos_b, const double* layer_out, const double* tail_ring,
                                       int32_t tail_ring_size, const int64_t* tail_state, const int64_t* sched,
                                       int32_t callback_size, int32_t n_tail, double g1, double g2, double* out);
/* launch_ir_spectra on heff[0 .. heff_len): h: [n_parts][partition][2] the spectra of the frames [heff[k * partition ..
 * (k + 1) * partition) | zeros] (zeros from heff_len on), hdn: [n_parts][2] their elements 0.  The device copy of heff holds
 * n_parts * partition elements, NaN from heff_len on.  gain: null, or [partition + 1] factors per bin: launch_spectrum_gain is
 * then applied and h_gain / hdn_gain receive both buffers again.
 * Refused unless: n_parts >= 1, 1 <= heff_len <= n_parts * partition, h_gain and hdn_gain non-null with gain. */
int32_t     cpq_diag_ir_spectra(int32_t partition, int32_t n_parts, const double* heff, int32_t heff_len, const double* gain,
                                double* h, double* hdn, double* h_gain, double* hdn_gain);
/* The launchers of mix_kernels.hip on their own (tests/test_gpu_mix_kernels.py): direct head, AGC, plan-group ring chunks,
 * processor-level mix with its delay ring, the delay-line reader's schedule, and the row helpers.  Conventions of the FFT
 * launch diagnostics above: all pointers are host memory; one stream, synchronised before the entry returns; every device row
 * is allocated at exactly the size stated here; every buffer a kernel may write is filled with 0xFF bytes (NaN; -1 for integers)
 * before the launch unless the caller supplies its contents ("in and out"), and is returned whole.  Each entry returns
 * CPQ_ERR_INVALID_ARG, before anything is allocated and before a device is looked for, unless the rules of its "Refused unless"
 * hold (and every pointer that is used is non-null); no buffer may exceed 2^28 elements.  Need a gfx950 device; no engine.
 *
 * cpq_diag_direct_head: launch_direct_head, then with out != null launch_rows_add of dout into out.
 *   in: [n_ch][in_stride] (n samples used per row), ir_rev: [n_slots][32] reversed taps, taps: [n_slots], ir_slot: [n_ch],
 *   hist_old: [n_ch][32], wet_on: [n_ch / 2] or null; dout: [n_ch][n] and hist_new: [n_ch][32] out; out: [n_ch][out_stride] in
 *   and out, or null.
 *   Refused unless: n_ch, n_slots >= 1; 1 <= n <= in_stride; 0 <= taps[s] <= 32; 0 <= ir_slot[c] < n_slots; n_ch even with
 *   wet_on; out_stride >= n with out. */
int32_t     cpq_diag_direct_head(int32_t n_ch, int32_t n, int64_t in_stride, int32_t n_slots, const double* in,
                                 const double* ir_rev, const int32_t* taps, const int32_t* ir_slot, const double* hist_old,
                                 const int32_t* wet_on, double* dout, double* hist_new, double* out, int64_t out_stride);
/* cpq_diag_agc on data: [n_ch][ch_stride] (in and out; callback t of a row is [t * B, (t + 1) * B)), S = n_ch / 2 streams:
 *   op 0 launch_agc_block_rms: rms: [n_ch][T] out.
 *   op 1 launch_agc_apply (gains, then ramp): rms_in, rms_out: [n_ch][T]; state: [S][3] = envIn, envOut, gain, in and out; on: [S]; gains: [S][T][2]
 *        out; b_att, b_rel, b_sm the per-callback coefficients.
 *   op 2 launch_gain_ramp: gains: [S][T][2] in; on: [S].
 *   op 3 launch_block_silence: silent: [S][T] out.
 *   Refused unless: op in 0 .. 3; n_ch, B, T >= 1; ch_stride >= B * T; ops 1 .. 3: n_ch even (S >= 1). */
int32_t     cpq_diag_agc(int32_t op, int32_t n_ch, int32_t B, int32_t T, int64_t ch_stride, double* data, const double* rms_in,
                         const double* rms_out, double* state, const int32_t* on, double* gains, double b_att, double b_rel,
                         double b_sm, double* rms, int32_t* silent);
/* cpq_diag_ring_chunks: the plan-group kernels on out: [rows][out_stride] (in and out), ch_map: [n_ch] (row of out per local
 * channel, -1 = unused slot), n samples in chunks of q (ceil(n / q) chunks, the last one possibly shorter):
 *   op 0 launch_rows_gather_multi: out is the source; n_dst destinations dst0 .. dst2: [n_ch][dst_stride[l]] (out), the n samples
 *        at dst_off[l] of every row; tab[0 .. n_tab) stored to tab_out: [64] (out).
 *   ops 1 .. 4 are launch_ring_chunks, with or without the read of layer 0's ring in front and with no, one or two tail taps:
 *   op 1 the read alone: ring0: [n_ch][size0], pos, cnt: [chunks].
 *   op 2 one tap added to out: ring_a: [n_ch][size_a], sched_a: [chunks] (negative: nothing added), gain_a.
 *   op 3 two taps added to out: ring_a and ring_b with their schedules and gains.
 *   op 4 the read, then the taps: ring0, pos, cnt, ring_a, sched_a, gain_a; ring_b may be null.
 *   Refused unless: op in 0 .. 4; rows, n_ch, n, q >= 1; out_stride >= n; every ch_map entry -1 or < rows and no row named
 *   twice; ring sizes powers of two >= 2; 0 <= cnt <= q; 0 <= pos <= 2^62; schedule entries <= 2^62; op 0: 1 <= n_dst <= 3,
 *   0 <= dst_off[l], dst_off[l] + n <= dst_stride[l], 0 <= n_tab <= 64 (the launcher would drop a longer table silently). */
int32_t     cpq_diag_ring_chunks(int32_t op, int32_t rows, int32_t n_ch, int32_t n, int32_t q, int64_t out_stride, double* out,
                                 const int32_t* ch_map, const double* ring0, int32_t size0, const int64_t* pos, const int64_t* cnt,
                                 const double* ring_a, int32_t size_a, const int64_t* sched_a, double gain_a, const double* ring_b,
                                 int32_t size_b, const int64_t* sched_b, double gain_b, int32_t n_dst, const int64_t* dst_stride,
                                 const int64_t* dst_off, double* dst0, double* dst1, double* dst2, const int64_t* tab,
                                 int32_t n_tab, int64_t* tab_out);
/* cpq_diag_convproc_mix: with old_ring != null launch_ring_regrow of old_ring: [n_ch][old_size] up to position regrow_end into a
 * zeroed ring (the contents of `ring` are then not read); with ring_in != null launch_ring_put of n_put samples of ring_in:
 * [n_ch][ring_in_stride] at pos0; then launch_convproc_mix over one range of n samples (n = 0: nothing is launched for it).
 *   wet, out: [n_ch][ch_stride]; in_place != 0: one device buffer, filled from wet and returned in out.  gains: [S][2] (wet, dry);
 *   ring: [n_ch][ring_size] in and out; d_new, d_old: [S]; x_len: [S] or null, x_gains: [S][x_cap]; ramp_len: [S] or null,
 *   ramp_gains: [S][ramp_cap][2]; wet_on: [S] or null.  S = n_ch / 2.
 *   Refused unless: n_ch even >= 2; 0 <= n <= ch_stride, ch_stride >= 1; ring_size a power of two >= 2; 0 <= pos0 <= 2^62;
 *   0 <= d_new[s], d_old[s] < ring_size; with x_len: x_cap >= 1 and 0 <= x_len[s] <= min(n, x_cap); with ramp_len: ramp_cap >= 1,
 *   ramp_off >= 0 and ramp_len[s] - ramp_off <= ramp_cap - ramp_off; with old_ring: old_size a power of two >= 2, ring_size >=
 *   old_size, 0 <= regrow_end <= 2^62; with ring_in: 1 <= n_put <= min(ring_in_stride, ring_size). */
int32_t     cpq_diag_convproc_mix(int32_t n_ch, int32_t n, int64_t ch_stride, const double* wet, double* out, int32_t in_place,
                                  const double* gains, double* ring, int32_t ring_size, int64_t pos0, const int32_t* d_new,
                                  const int32_t* d_old, const int32_t* x_len, const double* x_gains, int32_t x_cap,
                                  int32_t wet_valid, const int32_t* ramp_len, const double* ramp_gains, int32_t ramp_cap,
                                  int32_t ramp_off, const int32_t* wet_on, const double* old_ring, int32_t old_size,
                                  int64_t regrow_end, const double* ring_in, int64_t ring_in_stride, int32_t n_put);
/* cpq_diag_tail_reader: launch_tail_schedule for n_calls consecutive calls of T[i] callbacks of B samples, starting from
 * state_in: [4] = callbacks so far, read cursor of tail layer 1, of layer 2, first sample of the last call.  Layer l has
 * partition pl, outputDelaySamples ol and d callbacks between partition fill and delay-line write.  sched_out: the calls'
 * schedules one behind the other, call i as [n_tail][T[i]]; states_out: [n_calls][4] the state after every call.  With
 * layer_out != null launch_tail_append follows the last schedule: layer_out: [n_tail][n_ch][n_samples], ring: [n_tail][n_ch]
 * [ring_size] in and out.
 *   Refused unless: 1 <= n_calls <= 4096; T[i] >= 1, their sum <= 2^20; B >= 1; n_tail 1 or 2; per layer in use pl >= B,
 *   pl % B == 0, ol >= 0, d >= 0; 0 <= state_in[k] <= 2^62; with layer_out: n_ch, n_samples >= 1, ring_size a power of two >= 2. */
int32_t     cpq_diag_tail_reader(int32_t n_calls, const int32_t* T, int32_t B, int32_t n_tail, int32_t pl1, int32_t ol1, int32_t d1,
                                 int32_t pl2, int32_t ol2, int32_t d2, const int64_t* state_in, int64_t* sched_out,
                                 int64_t* states_out, int32_t n_ch, int32_t n_samples, const double* layer_out, double* ring,
                                 int32_t ring_size);
/* cpq_diag_rows on dst: [n_ch][dst_stride] (in and out):
 *   op 0 launch_rows_copy: dst[c][dst_off + i] = src[c][src_off + i], i < n; src: [n_ch][src_stride].
 *   op 1 launch_rows_scale: the first n samples of every row times gain[c / 2]; gain: [n_ch / 2].
 *   op 2 launch_bypass_blend: dst = out, src = dry; on, len, g_end: [n_ch / 2]; gains: [n_ch / 2][cap].
 *   Refused unless: op in 0 .. 2; n_ch, n >= 1; 0 <= offset and offset + n <= stride on both sides in use; ops 1, 2: n_ch even
 *   and both offsets 0; op 2: cap >= 1 and 0 <= len[s] <= cap. */
int32_t     cpq_diag_rows(int32_t op, int32_t n_ch, int32_t n, const double* src, int64_t src_stride, int64_t src_off, double* dst,
                          int64_t dst_stride, int64_t dst_off, const double* gain, const int32_t* on, const int32_t* len,
                          const double* g_end, const double* gains, int32_t cap);
/* Chained spans of the EQ / output-filter cascade (engines with fewer channels than the device holds workgroups of the span
 * kernel: the spans of a call are dealt to the workgroups and a band's state is handed from span to span inside the launch).
 * Synchronises the engine's stream; *launches = chained launches so far (0: this engine never chains), *gave_up != 0 when a
 * hand-over ever ran into its poll bound (a defect: results of that launch are not valid).  For tests. */
int32_t     cpq_diag_eq_chain_status(cpq_engine* e, uint32_t* launches, uint32_t* gave_up);

/* ------------------------------------------------------- shaper scorer: the fitness function of the adaptive shaper's learner */
/* cpq_scorer reproduces the deterministic part of NoiseShaperLearner (src/NoiseShaperLearner.cpp): configureForSampleRate,
 * buildTrainingSegments with precomputeMaskingThresholds, evaluateCandidate / evaluateCandidateMapped, and
 * MklFftEvaluator::evaluate / computeMaskingThreshold (src/MklFftEvaluator.h).  It is an object of its own, independent of
 * cpq_engine, with the same device rules: CPQ_ERR_NO_DEVICE without a gfx950 device, no CPU fallback.  One scorer serves
 * n_learners learners, each with its own training segments; one call scores every candidate of every learner.  The optimiser
 * (CMA-ES) is cpq_learner, further down, which drives a scorer generation after generation on the device; the capture queue and
 * AudioSegmentBuffer, elite re-evaluation (call score again) and persistence are the caller's.  A scored set reaches the shaper
 * through cpq_dither_set_adaptive_coeffs.
 *
 * Generator semantics.  reset() of the reference's shaper clears the lattice states and not the generator, so within one
 * EvaluationContext the dither stream runs on across segments and candidates, and which worker scores which candidate is a race:
 * the reference's population scores are not a function of their inputs.  Two deterministic modes are offered; segment s counts in
 * evaluation order (level-major, then bucket order), a segment draws 8192 words per channel, and rng_start is
 * LatticeNoiseShaper::rngState (src/LatticeNoiseShaper.h:297-300) unless cpq_scorer_set_rng_start changed it:
 *   CPQ_SCORE_RNG_FRESH    every candidate is scored by a freshly constructed context: candidate c, segment s starts from
 *                          rng_start advanced by 8192 * s words (the default)
 *   CPQ_SCORE_RNG_CHAINED  one context scores candidates 0 .. C - 1 in order, the reference with no auxiliary workers:
 *                          rng_start advanced by 8192 * (c' * n_segments + s) words, c' the number of candidates of that
 *                          learner before c that ran: a set the stability check refuses is not run and draws nothing, so
 *                          c' = c while every candidate is stable.
 * Nothing is carried from one score call to the next.
 * The 4096-point transform is the device's own (FFT parity unpinned: IPP's and the device's spectra differ by their own rounding
 * only); sums over bins are tree-shaped; every data-dependent decision is the reference's comparison on the reference's quantity. */
#define CPQ_HAS_SHAPER_SCORING 1
#define CPQ_SCORE_RNG_FRESH   0
#define CPQ_SCORE_RNG_CHAINED 1
#define CPQ_SCORE_SEGMENT_LEN  4096     /* AudioSegment::kLength */
#define CPQ_SCORE_MAX_SEGMENTS 16       /* kMaxTrainingSegments: 4 levels x 4 */
#define CPQ_SCORE_RECENT (4096 + 2048 * 15)     /* kRecentSampleRequest */
#define CPQ_SCORE_MAX_CANDIDATES 1024   /* per learner and call: the start-state table (16 entries of 8192 words a candidate,
                                         * stepped on the host at create and set_rng_start) stays below a second of host work */
#define CPQ_SCORE_UNSTABLE 1e18        /* evaluateCandidateMapped's penalty of a set isStable refuses */
typedef enum { CPQ_SEGMENT_BROADBAND = 0, CPQ_SEGMENT_TONAL = 1, CPQ_SEGMENT_TRANSIENT = 2 } cpq_segment_type;   /* SpectralType */
typedef struct cpq_scorer cpq_scorer;
typedef struct {
    int32_t n_learners;             /* >= 1 */
    int32_t max_candidates;         /* 1 .. CPQ_SCORE_MAX_CANDIDATES; the reference's population is 18 */
    double  sample_rate_hz;         /* finite, > 0: configureForSampleRate and precomputeMaskingThresholds */
    int32_t bit_depth;              /* evaluationBitDepth, 1 .. 32 */
    double  level_weights[4];       /* currentLevelWeights; reference default {0.4, 0.3, 0.2, 0.1}; finite, >= 0 */
    double  coeff_safety_margin;    /* settings.coeffSafetyMargin (0.85), in (0, 1]: cpq_scorer_score_raw only */
    int32_t stability_check;        /* settings.enableStabilityCheck (1) */
    int32_t rng_mode;               /* CPQ_SCORE_RNG_* */
} cpq_scorer_desc;
typedef struct {                    /* MklFftEvaluator::Result (src/MklFftEvaluator.h:40-47) */
    double noise_power, spectral_flatness_penalty, hf_penalty, time_domain_rms, composite_score;
} cpq_score_parts;
typedef struct {                    /* one LeveledSegment of a learner, in evaluation order */
    int32_t start;                  /* first sample of the window, counted from the first of the samples used */
    int32_t level;                  /* 0 .. 3: -40, -30, -20, -10 dBFS */
    int32_t type;                   /* cpq_segment_type (crest factor > 5: transient, < 1.6: tonal) */
    int32_t reserved;
    double  gain;                   /* appliedGain: targetRMS / rms, or 0.95 / peak where that is smaller */
} cpq_score_segment;
/* CPQ_ERR_INVALID_ARG for a desc outside the ranges above or a null argument; CPQ_ERR_NO_DEVICE; CPQ_ERR_OOM. */
int32_t cpq_scorer_create(const cpq_scorer_desc* desc, cpq_scorer** out);
void    cpq_scorer_destroy(cpq_scorer* s);
/* the text of the scorer's last refusal or failure ("" when there was none) */
const char* cpq_scorer_last_error(const cpq_scorer* s);
/* buildTrainingSegments (src/NoiseShaperLearner.cpp:1185-1270) of one learner on the most recent min(n, CPQ_SCORE_RECENT) of the
 * samples given, replacing what the learner held: hop 2048, windows with RMS below 1e-5 gated out, gain limited by the peak
 * headroom 0.95, targets -40 / -30 / -20 / -10 dBFS, a bucket full at 4.  The selection runs on the host in the reference's order;
 * the levelling multiply and precomputeMaskingThresholds (:1377-1398: transform of the levelled segment, computeMaskingThreshold
 * per bin) run on the device and stay there.  *n_segments (may be NULL) = segments held afterwards; n < 4096 gives 0 and CPQ_OK.
 * The _device variant takes device pointers (the selection reads a copy).  CPQ_ERR_INVALID_ARG: learner out of range, n < 0,
 * a null row with n > 0. */
int32_t cpq_scorer_set_audio(cpq_scorer* s, int32_t learner, const double* left, const double* right, int32_t n, int32_t* n_segments);
int32_t cpq_scorer_set_audio_device(cpq_scorer* s, int32_t learner, const double* d_left, const double* d_right, int32_t n, int32_t* n_segments);
/* segments[0 .. *n_segments - 1] of a learner (room for CPQ_SCORE_MAX_SEGMENTS) and counts[4] per level; either may be NULL */
int32_t cpq_scorer_get_segments(const cpq_scorer* s, int32_t learner, cpq_score_segment* segments, int32_t* n_segments, int32_t counts[4]);
/* thresholds[2049] = LeveledSegment::maskingThresholds of segment `segment` (evaluation order) of a learner.  Synchronises. */
int32_t cpq_scorer_read_thresholds(cpq_scorer* s, int32_t learner, int32_t segment, double* thresholds);
/* evaluateCandidateMapped (src/NoiseShaperLearner.cpp:1289-1375) for every learner and candidate: mapped [n_learners]
 * [n_candidates][9] reflection coefficients, scores [n_learners][n_candidates], parts (may be NULL) [n_learners][n_candidates]
 * [16] per segment in evaluation order, zero where nothing was evaluated.  1 <= n_candidates <= max_candidates.  Per candidate:
 * with the stability check on, a set isStable refuses (some |k| >= 1 - 1e-12) scores CPQ_SCORE_UNSTABLE and is not run; otherwise
 * a fresh shaper (prepare(bit_depth), setCoefficients: clampCoeff to +-0.85) runs every segment from cleared states with headroom
 * 0.8912509381337456, the error yq - x * headroom goes through evaluate() with the segment's masking thresholds, and the score is
 * sum_level(w_level * mean_segments(alpha * sqrt(composite / 4096) * 1000 + (1 - alpha) * rms * 1000)) / sum_level(w_level) over
 * the levels that hold segments, alpha 0.3 / 0.5 / 0.5 / 0.7.  A learner without segments (or with zero total weight) scores
 * DBL_MAX.  The lattice stage is bit-exact; the rest differs from the reference by rounding alone.  Host pointers; synchronises. */
int32_t cpq_scorer_score(cpq_scorer* s, const double* mapped, int32_t n_candidates, double* scores, cpq_score_parts* parts);
/* evaluateCandidate (:1272-1287): mapped = clampCoeff(tanh(raw), coeff_safety_margin) on the host with std::tanh, then the above.
 * The reference's population path maps with MKL's vdTanh, which may differ from std::tanh in the last place: cpq_scorer_score is
 * the exact entry point. */
int32_t cpq_scorer_score_raw(cpq_scorer* s, const double* raw, int32_t n_candidates, double* scores, cpq_score_parts* parts);
/* the two generator states (L, R) every evaluation counts from; rebuilds the start-state tables.  Acts on the next score call. */
int32_t cpq_scorer_set_rng_start(cpq_scorer* s, const uint64_t state[2][4]);
/* Diagnostic: the error rows (4096 doubles each; either may be NULL) the lattice stage of the last score call stored for one
 * (learner, candidate, segment).  CPQ_ERR_NOT_READY when that call did not run this chain (no call yet, candidate refused or
 * beyond its n_candidates, segment beyond the learner's). */
int32_t cpq_scorer_read_error(cpq_scorer* s, int32_t learner, int32_t candidate, int32_t segment, double* left, double* right);
/* Diagnostic: events around the two stages of the last score call, in milliseconds */
int32_t cpq_scorer_last_timing(cpq_scorer* s, double* lattice_ms, double* spectrum_ms);
/* configureForSampleRate on the host, for tests and tuning: any of the outputs may be NULL.  weight[2049] = weights[bin] *
 * jndWeight(bin), bark / ath_db / width (getBinWidth) [2049], band / range (binToBand, neighborRangeBins) [2049], bins[4] =
 * flatnessStartBin, flatnessEndBin, highBandStartBin, ultraHighStartBin, scalars[4] = expectedUltraHighShare,
 * flatnessPenaltyWeight, hfPenaltyWeight, sum of weight. */
int32_t cpq_score_design(double sample_rate_hz, double* weight, double* bark, double* ath_db, double* width, int32_t* band,
                         int32_t* range, int32_t bins[4], double scalars[4]);
/* buildTrainingSegments' selection alone, on the host: as cpq_scorer_get_segments after cpq_scorer_set_audio would report */
int32_t cpq_score_select_segments(const double* left, const double* right, int32_t n, cpq_score_segment* segments,
                                  int32_t* n_segments, int32_t counts[4]);
/* The scorer's three kernels on their own (csrc/engine_diag.cpp, tests/test_gpu_score_kernels.py), for inputs cpq_scorer_score
 * cannot produce: no scorer object.  Conventions of the other cpq_diag_* entries: all pointers are host memory; the null stream,
 * synchronised before the entry returns; every device buffer is allocated at exactly the size stated here; every buffer a kernel
 * may write is filled with 0xFF bytes (NaN) before the launch unless the caller supplies its contents ("in and out"), and is
 * returned whole.  Each entry returns CPQ_ERR_INVALID_ARG, with the reason in cpq_last_error(NULL), before anything is allocated
 * and before a device is looked for, unless the rules of its "Refused unless" hold and every pointer is non-null; no buffer may
 * exceed 2^28 elements.  Need a gfx950 device (CPQ_ERR_NO_DEVICE); an allocation or HIP failure is CPQ_ERR_DEVICE.  Like every
 * addition since revision 1 they leave CPQ_ABI_REVISION as it is (a caller that may meet an older library looks the symbols up),
 * and as diagnostics of kernels no engine profiles they add no cpq_kernel_id.
 *
 * cpq_diag_score_spectrum: launch_score_spectrum as cpq_scorer makes it, with the tables of sample_rate_hz (built and uploaded by
 *   the scorer's own function).  rows: [n_rows][2][4096] (L, R); thr: [n_thr][2049], in and out; evals: [n_evals], evaluation i
 *   reads row pair evals[i].row and, with thresholds_only == 0, the masking thresholds thr[evals[i].thr], and stores
 *   MklFftEvaluator::evaluate's members to parts[evals[i].slot] and alpha * sqrt(composite / 4096) * 1000 + (1 - alpha) * rms * 1000
 *   to blended[evals[i].slot]; thr comes back as given.  thresholds_only != 0: computeMaskingThreshold of every bin of 0.5 (|L|^2 +
 *   |R|^2) to thr[evals[i].thr]; parts and blended come back as the fill.  parts, blended: [n_slots], out.
 *   Refused unless: sample_rate_hz finite and > 0; n_rows, n_thr, n_evals, n_slots >= 1; 0 <= row < n_rows, 0 <= thr < n_thr,
 *   0 <= slot < n_slots for every evaluation; no slot named twice; with thresholds_only no thr named twice.
 * cpq_diag_score_lattice: launch_score_lattice with the shaper parameters cpq_scorer_create derives from bit_depth (one shared
 *   function).  seg: [n_src][4096]; err: [n_dst][4096], out; chains: [n_chains], chain i runs a fresh shaper with the clamped
 *   coefficients coef[chains[i].coef][9] and the generator words rng[chains[i].rng][4] over seg[chains[i].src] and stores
 *   yq - x * headroom to err[chains[i].dst]; coef: [n_coef][9]; rng: [n_rng][4].
 *   Refused unless: 1 <= bit_depth <= 32; n_src, n_dst, n_chains, n_coef, n_rng >= 1; every index of every chain inside its
 *   table; no dst named twice.
 * cpq_diag_score_reduce: launch_score_reduce.  counts: [n_learners][4] segments per level; state: [n_learners * n_cand] (1: the
 *   pair scores CPQ_SCORE_UNSTABLE); blended: [n_learners * n_cand][16], a pair's segments in evaluation order; weights: [4];
 *   scores: [n_learners * n_cand], out.  No level with segments, or no weight on those levels: DBL_MAX.
 *   Refused unless: n_learners, n_cand >= 1, n_learners * n_cand <= 2^20; every count >= 0 and a learner's counts sum to <= 16. */
typedef struct { int32_t row, thr, slot, reserved; double alpha; } cpq_diag_score_eval;
typedef struct { int32_t src, dst, coef, rng; } cpq_diag_score_chain;
int32_t cpq_diag_score_spectrum(double sample_rate_hz, int32_t n_rows, const double* rows, int32_t n_thr, double* thr,
                                int32_t n_evals, const cpq_diag_score_eval* evals, int32_t n_slots, int32_t thresholds_only,
                                cpq_score_parts* parts, double* blended);
int32_t cpq_diag_score_lattice(int32_t bit_depth, int32_t n_src, const double* seg, int32_t n_dst, double* err, int32_t n_chains,
                               const cpq_diag_score_chain* chains, int32_t n_coef, const double* coef, int32_t n_rng,
                               const uint64_t* rng);
int32_t cpq_diag_score_reduce(int32_t n_learners, int32_t n_cand, const int32_t* counts, const int32_t* state,
                              const double* blended, const double* weights, double* scores);

/* ------------------------------------------------------- shaper learner: the optimiser of the adaptive shaper, on the device */
/* cpq_learner is the reference's CmaEsOptimizer (src/CmaEsOptimizer.h: dimension 9, population 18, elite 6) with the generation
 * loop of NoiseShaperLearner (src/NoiseShaperLearner.cpp: evaluatePopulation and the best tracking at :716-729, :975-986) around a
 * cpq_scorer.  One learner object serves the scorer's n_learners learners; each has its own state on the device.  cpq_learner_run
 * builds and uploads the scorer's chain and evaluation tables once and enqueues, per generation, ask (k_learn_ask: normal
 * variates, Cholesky factor, 18 candidates, their mapping into the scorer's coefficient buffer), the scorer's three kernels and
 * tell (k_learn_tell: CmaEsOptimizer::update and the best tracking) on the scorer's stream; the host does nothing in between and
 * the call returns without waiting.  The arithmetic is stated once (csrc/learn_plan.hpp) for the kernels and for the
 * cpq_learn_*_host entries: they agree bit for bit except through log (normal variates) and tanh (mapping), which are each
 * side's math library.
 *
 * Where this differs from the reference, and why:
 *   normal variates   the reference seeds std::mt19937 from random_device and draws std::normal_distribution; neither stream is
 *                     reproduced.  A learner draws xoshiro256++ words w (the dither stage's generator), u = (w >> 11) 2^-53, and
 *                     pairs by Marsaglia's polar method: v = 2 u - 1, s = v1^2 + v2^2, accepted when 0 < s < 1,
 *                     m = sqrt(-2 log(s) / s), z = (v1 m, v2 m), filling z[candidate][dimension] in order.  After 32 refused
 *                     tries a pair is (0, 0) and rejected_pairs counts it: a generator state of four zero words cannot spin.
 *                     A seed becomes four successive splitmix64 outputs.
 *   the sort          ascending fitness, ties by the lower index, NaN after everything else (std::sort leaves ties open)
 *   re-evaluation     evaluatePopulation scores its top three again and averages (:700-714).  cpq_learner needs a scorer in
 *                     CPQ_SCORE_RNG_FRESH mode, where a second score of the same candidate is the same bits a, and
 *                     (a + a) * 0.5 == a for every score a run can produce (2 a does not overflow below DBL_MAX / 2, and
 *                     CPQ_SCORE_UNSTABLE and DBL_MAX themselves are not averaged into anything else): it is left out.
 *   unstable sets     a candidate the stability check refuses is run all the same and scores CPQ_SCORE_UNSTABLE in the
 *                     reduction, so that the tables of a run do not depend on its candidates
 *   inactive          a learner holding fewer than two segments when a run starts is left alone (the reference waits for
 *                     audio): neither its state nor its generation count moves
 * Not here: the capture queue and AudioSegmentBuffer, persistence, wall-clock pacing. */
#define CPQ_HAS_SHAPER_LEARNING 1
#define CPQ_LEARN_DIM 9                 /* CmaEsOptimizer::kDim */
#define CPQ_LEARN_POPULATION 18         /* kPopulation */
#define CPQ_LEARN_ELITE 6               /* kElite */
#define CPQ_LEARN_MAX_GENERATIONS 4096  /* of one cpq_learner_run */
#define CPQ_LEARN_MAX_TRIES 32          /* refused tries of the polar method before a pair becomes (0, 0) */
typedef struct cpq_learner cpq_learner;
typedef struct {                        /* CmaEsOptimizer::Params and NoiseShaperLearner::currentLevelWeights */
    double sigma_min, sigma_max, cov_retention_target, cov_retention_step, level_weights[4];
} cpq_learn_params;
typedef struct {
    double   mean[9], cov_upper[45];    /* serializeTo's layout: rows of the upper triangle */
    double   sigma, cov_retention;      /* covRetentionCurrent */
    uint64_t rng[4];                    /* xoshiro256++; four zero words are refused */
    double   best_score;                /* DBL_MAX until a generation's best is below it */
    double   best_raw[9];               /* the unconstrained candidate that earned best_score */
    double   best_scored[9];            /* its mapped set, the one that was scored: for cpq_dither_set_adaptive_coeffs */
    int32_t  generations, rejected_pairs;
} cpq_learn_state;
typedef enum { CPQ_LEARN_SHORTEST = 0, CPQ_LEARN_SHORT, CPQ_LEARN_MIDDLE, CPQ_LEARN_LONG, CPQ_LEARN_ULTRA, CPQ_LEARN_CONTINUOUS } cpq_learn_mode;
/* Borrows the scorer, its stream, its buffers and its segments: the scorer must outlive the learner, and a cpq_scorer_score call
 * between runs is allowed (a run rebuilds what it needs).  CPQ_ERR_INVALID_ARG: null argument, a scorer with max_candidates < 18
 * or a generator mode other than CPQ_SCORE_RNG_FRESH (the reason in cpq_last_error(NULL)); CPQ_ERR_OOM. */
int32_t cpq_learner_create(cpq_scorer* scorer, cpq_learner** out);
void    cpq_learner_destroy(cpq_learner* l);
const char* cpq_learner_last_error(const cpq_learner* l);
/* initFromParcor (src/CmaEsOptimizer.h:97-105) of one learner or of CPQ_ALL_STREAMS, with the generator seeded from `seed`
 * (every learner from seed + its index), best_score DBL_MAX, the counters 0.  Synchronises. */
int32_t cpq_learner_init(cpq_learner* l, int32_t learner, const double parcor[9], uint64_t seed);
/* Acts on the next run.  Defaults: 0.03, 0.30, 0.92, 0, the scorer's level weights.  Refused unless every value is finite,
 * 0 < sigma_min <= sigma_max, 0 <= cov_retention_target <= 1, cov_retention_step >= 0, the weights >= 0. */
int32_t cpq_learner_set_params(cpq_learner* l, const cpq_learn_params* p);
/* n_generations in 1 .. CPQ_LEARN_MAX_GENERATIONS; enqueues and returns.  CPQ_ERR_NOT_READY: a learner holding two or more
 * segments was never initialised.  cpq_scorer_read_error afterwards names the last generation's rows. */
int32_t cpq_learner_run(cpq_learner* l, int32_t n_generations);
/* One learner's state.  Both synchronise.  set_state refuses a non-finite mean, covariance, sigma or retention, a generator of
 * four zero words and negative counters. */
int32_t cpq_learner_get_state(cpq_learner* l, int32_t learner, cpq_learn_state* out);
int32_t cpq_learner_set_state(cpq_learner* l, int32_t learner, const cpq_learn_state* in);
/* The last generation a run made for this learner: z, candidates, mapped [18][9], scores [18], order [18] (the sort); any may be
 * NULL.  CPQ_ERR_NOT_READY before the learner's first generation.  Synchronises. */
int32_t cpq_learner_read_generation(cpq_learner* l, int32_t learner, double* z, double* candidates, double* mapped, double* scores,
                                    int32_t* order);
/* best_per_generation[0 .. *n - 1] (room for the last run's n_generations): every generation's lowest score, of the last run;
 * *n = 0 for a learner the run left alone.  Either may be NULL.  Synchronises. */
int32_t cpq_learner_read_history(cpq_learner* l, int32_t learner, double* best_per_generation, int32_t* n);
/* What the reference publishes: tanh(sanitize(tanh(best_raw))) -- toParcor at NoiseShaperLearner.cpp:975, then tanh again where
 * the published set is applied (:1465).  This is the reference's own double mapping, computed on the host with std::tanh; the
 * set that earned best_score is best_scored. */
int32_t cpq_learner_published(cpq_learner* l, int32_t learner, double k[9]);
/* Diagnostic: events around ask and around tell of the last run's last generation, in milliseconds.  Synchronises. */
int32_t cpq_learner_last_timing(cpq_learner* l, double* ask_ms, double* tell_ms);
/* The optimiser on the host (csrc/learn_plan.hpp), no device needed.  Null arguments are refused.
 * cpq_learn_init_host: initFromParcor (atanh of the set clamped to +-0.995, sigma 0.12, identity covariance, retention =
 *   params->cov_retention_target; params NULL: the defaults), the generator from `seed`.
 * cpq_learn_normals_host: the 162 variates of one generation from state->rng, which advances; *words (may be NULL) = generator
 *   words drawn; state->rejected_pairs counts the pairs given up.
 * cpq_learn_ask_host: CmaEsOptimizer::sample with the variates given: candidates [18][9].
 * cpq_learn_tell_host: CmaEsOptimizer::update, then the best tracking and generations + 1.  mapped [18][9] (may be NULL:
 *   best_scored stays) are the sets that were scored; order [18] (may be NULL) receives the sort.
 * cpq_learn_phase: computePhase (:227-258): 1, 2 or 3; CPQ_ERR_INVALID_ARG for an unknown mode or seconds not finite.
 * cpq_learn_phase_params: applyPhaseParams (:260-317): retention target and step and the level weights of (mode, phase 1..3),
 *   sigma_min / sigma_max at their defaults; *generation_interval_s (may be NULL) = generationIntervalSeconds. */
int32_t cpq_learn_init_host(const double parcor[9], uint64_t seed, const cpq_learn_params* params, cpq_learn_state* out);
int32_t cpq_learn_normals_host(cpq_learn_state* state, double z[162], int32_t* words);
int32_t cpq_learn_ask_host(const cpq_learn_state* state, const double z[162], double candidates[162]);
int32_t cpq_learn_tell_host(cpq_learn_state* state, const cpq_learn_params* params, const double candidates[162],
                            const double mapped[162], const double fitness[18], int32_t order[18]);
int32_t cpq_learn_phase(int32_t mode, double playback_seconds);
int32_t cpq_learn_phase_params(int32_t mode, int32_t phase, cpq_learn_params* out, double* generation_interval_s);
/* k_learn_tell alone, on the conventions of the cpq_diag_score_* entries above: states [n_learners], in and out; candidates,
 * mapped [n_learners][18][9]; fitness [n_learners][18].  Refused unless 1 <= n_learners <= 2^20. */
int32_t cpq_diag_learn_tell(int32_t n_learners, cpq_learn_state* states, const cpq_learn_params* params, const double* candidates,
                            const double* mapped, const double* fitness);
/* k_prog_finish alone (prog_kernels.hip), on the same conventions: hops [n_streams][max_hops] on the host, of which the kernel is
 * given the first n_hops of every row (what lies behind them must not matter); out [n_streams] as cpq_loudness_finish makes it.
 * What the kernel itself delivers, before any logarithm (csrc/prog_plan.hpp, ProgRecord), goes to z [n_streams][6]: the mean
 * squares zInt, zGate, zMomMax, zShortMax, zLo, zHi, and to counts [n_streams][4]: nAbs, nRel, nShortAbs, nShortKept; either
 * may be NULL.  Refused unless: hops and out not NULL, 1 <= n_streams <= 32767, max_hops >= 1, 0 <= n_hops <= max_hops,
 * sample_rate one cpq_loudness_create takes, at most 8192 short-term blocks at the 1 s step in n_hops, n_streams * max_hops
 * <= 2^28. */
int32_t cpq_diag_prog_finish(int32_t n_streams, int32_t n_hops, int32_t max_hops, double sample_rate, const double* hops,
                             cpq_loudness_result* out, double* z, int32_t* counts);

/* The complex fp64 transforms of the minimum-phase conversion alone (minphase_kernels.hip): `rows` transforms of 2^log2n points,
 * re_im and out [rows][2^log2n][2], natural order in and out, on the path the size selects (up to 4096 points the LDS transform,
 * above it the column and row passes); inverse != 0: the inverse transform with its 1 / N.  The four-step path keeps its spectra
 * as [k1][k2] on the device; the reordering to and from natural order is host work of this entry.
 * Refused unless: 1 <= log2n <= 23, rows >= 1, rows * 2^(log2n + 1) <= 2^28. */
int32_t cpq_diag_cfft(const double* re_im, int32_t log2n, int32_t rows, int32_t inverse, double* out);

#ifdef __cplusplus
}
#endif
#endif /* CONVOPEQ_MI355X_H */
