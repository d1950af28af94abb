// engine_internal.hpp -- the engine object behind the C ABI and the helpers its translation units share:
//   engine_core.cpp  create / destroy / prepare, status and profiling entry points, DSPCore routing (whole path); what the stage
//                    files below share: checkCall, checkBaseRows, hostRoundTrip, refreshBaseRateStages
//   engine_conv.cpp  kernel-level convolver: set_impulse, FilterSpec tail layers, the per-call kernel sequence
//   engine_native.cpp  plan groups: streams whose convolver runs on the reference's own layer plan; a call is carried out as
//                    nuc_replay.hpp plans it
//   engine_upload.cpp  the pinned staging ring behind every small host -> device upload of a call
//   engine_proc.cpp  processor-level stage: dry delay ring, mix ramp, latency cross-fade; a call is carried out step by step as
//                    host_replay.hpp plans it
//   engine_eq.cpp    EQ and output filter: design into one host image of a stream's tables, the one routine that uploads it,
//                    and the EQ call carried out piece by piece as host_replay.hpp plans it
//   engine_os.cpp    half-band oversampler around the routing: stage buffers, per-stream state machine
//   engine_softclip.cpp  soft clipper between the make-up gain and the down stages; at factor 1 with its local 2x pair
//   engine_pcm.cpp   packed PCM in and out: the converters around the whole-chain call
//   engine_out.cpp   output stage: DC blocker, headroom, limiter and clamp on the delivered rows
//   engine_dither.cpp  dither stage: the fixed 4- and 15-tap and the adaptive lattice noise shaper between the output stage's two halves
//   engine_meter.cpp  loudness and true-peak metering of the delivered rows
//   engine_diag.cpp  every cpq_diag_* entry point: single launchers on caller-filled buffers, no engine
//   engine_score.cpp  cpq_scorer, an object of its own: the fitness function of the adaptive shaper's learner; engine_learn.cpp,
//                    cpq_learner around it (score_internal.hpp; of this header they use fail, CPQ_TRY and the scorer's tables)
//   engine_resample.cpp  cpq_ir_resample / _batch: the device side of the IR sample-rate conversion, no engine (uses only fail,
//                    checkCurrentDevice and CPQ_TRY of this header; design, checks, host path and tail trim are resample_design.cpp's)
//   engine_minphase.cpp  cpq_ir_minimum_phase / _batch, cpq_ir_prepare_batch: the device side of the minimum-phase conversion, no
//                    engine; the plan of a call is minphase_plan.hpp's, the host steps around it are ir_ingest.hpp's
//   engine_src.cpp   cpq_src, an object of its own: streaming sample-rate conversion; the plan of a call is src_plan.hpp's, the
//                    host object src_host.hpp's
//   engine_prog.cpp  cpq_loudness, an object of its own: gated programme loudness per stream; the plan of a call and the
//                    definition are prog_plan.hpp's
//   engine_lim.cpp   cpq_limiter, an object of its own: look-ahead true-peak limiter per stream; the definition and the plan of a
//                    call are lim_plan.hpp's, the host object lim_host.hpp's
//   object_support.hpp  what four of those objects and the two loader calls share (engine_prog / lim / score / learn /
//                    resample / minphase.cpp; engine_src.cpp keeps its own copies): failTo, CPQ_OBJ_HIP, the owner of timing events, the row stage, setStream, guardAlloc.
//                    Of the helpers declared below, cpq_src, cpq_loudness and cpq_limiter use only checkCurrentDevice and CPQ_TRY.
// The per-stream ramps and fades those files replay on the host (total gain, EQ bypass, mix, latency) are the structs of
// host_replay.hpp, and so are the EQ's plan of a call (gain segments, bypass classes, band resets, pieces) and the processor-level
// stage's (who rests, mix prefixes, latency ranges): HIP-free steppers and planners that return plain data; the engine files
// allocate, upload and launch.  The plan groups' integer state (the
// reference's Add / Get bookkeeping per layer) and the plan of one of their calls are nuc_replay.hpp's, in the same way.
// Device memory is owned (device_buffers.hpp): the arena for what every engine needs, one buffer or group of buffers per
// feature allocated on first use, all of it freed with the engine.
#pragma once

#include "convopeq_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "device_buffers.hpp"
#include "host_design.hpp"
#include "host_replay.hpp"
#include "nuc_replay.hpp"
#include "resample_design.hpp"
#include "softclip_design.hpp"
#include "kernels.hpp"

using cpq::kBands;

struct ProfileSlot {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> freeList;
    int64_t launches = 0;
    double totalMs = 0.0;
};


// One layer of a plan group (engine_native.cpp), run at the reference's OWN partition size: the HC/LC gains (and the
// air-absorption damping) multiply every partition spectrum of a layer at that layer's FFT size, which folds time-aliased
// energy into the frame (src/MKLNonUniformConvolver.cpp:336-443) -- only reproducible with the same partitioning; and the
// reference's Add / Get bookkeeping (input fill, distributed tail MAC, delay-line reader) runs per layer.
// What a layer carries over when its group is resized or a member is moved to a group of its own is its LayerState
// (nuc_replay.hpp): plain host state.
struct NativeLayer : cpqi::LayerState {
    int P = 0, K = 0, kPad = 0, hRows = 0, ringSlots = 0, nbMax = 0, accCap = 0, outRing = 0;
    double gain = 1.0;          // tail-layer gain applied by the delay-line reader
    int ppc = 1, outputDelay = 0;       // partsPerCallback (:988-994), outputDelaySamples (:1005-1024)
    cpqi::DeviceBuffer<char> mem;       // one allocation; the pointers below are carved out of it
    double2 *X = nullptr, *XDN = nullptr, *H = nullptr, *HDN = nullptr, *Y = nullptr, *tw = nullptr, *tw2 = nullptr, *twCol = nullptr, *twSplit = nullptr;
    double *hist[2] = { nullptr, nullptr }, *acc[2] = { nullptr, nullptr }, *ring = nullptr, *gainDev = nullptr;
    double2* scratch = nullptr;   // four-step FFT workspace (P > 4096): [max(nCh * nbMax, K)][P]
    cpq::FftTables tables() const { return cpq::FftTables{ tw, tw2, twCol, twSplit }; }
};

// Streams that share one layer plan and one phase (loaded while the group was fresh); see engine_native.cpp
struct PlanGroup {
    cpq_nuc_plan plan{};
    bool hasSpec = false, shared = false;       // shared: CPQ_ALL_STREAMS (one stereo IR for every member)
    bool frozen = false;                        // processor-level bypass / dry-only of its (single) member: not processed
    cpq_filter_spec spec{};
    int capCh = 0, usedCh = 0;                  // allocated / launched local channels (2 per pair slot)
    bool identityMap = false;                   // chMap[i] == i for every launched channel (layer 0 may then write the output rows itself)
    std::vector<int> streamOfPair;              // pair slot -> stream, -1 = free
    std::vector<NativeLayer> layers;
    cpqi::DeviceBuffer<int> chMapDev;                // [capCh] local channel -> row of the call's buffers (-1 = free slot)
    cpqi::DeviceBuffer<int> irSlotDev;               // [capCh] local channel -> IR slot
    cpqi::DeviceBuffer<long long> tabDev;            // the call's chunk tables
    int tabCap = 0;
    cpqi::NucCallPlan call;                     // the call in flight: built by groupsAppend, carried out by groupsRunLayer0 / groupsRunTails
    long long samplesSinceReset = 0;
    int lastGot = 0, lastCall = 0;              // Get()'s return value summed over the chunks of the last call
    // tail layer l's delay line as Get() reads it in the call in flight (its schedule: call.offs[2 l]); empty when the plan has no layer l
    cpq::RingTap tap(size_t l) const
    {
        if (l >= layers.size()) return cpq::RingTap{};
        return cpq::RingTap{ layers[l].ring, layers[l].outRing, tabDev + call.offs[2 * l], layers[l].gain };
    }
};

// pinned staging for the small host -> device tables of a call (chunk schedules, per-stream gains and flags): a byte ring;
// a region is reused only after the copy that read it has run (one event per upload)
struct PinnedRing {
    struct Pending { size_t begin, end; hipEvent_t ev; };
    cpqi::PinnedBuffer<char> host;
    size_t cap = 0, head = 0;
    std::vector<Pending> pending;       // in issue order
    std::vector<hipEvent_t> freeEvents;
};

struct cpq_engine {
    cpq_engine_desc desc{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copyIn = nullptr, copyOut = nullptr;      // host-pointer entry points: upload / download beside the kernels
    hipEvent_t evIn[4] = {}, evDone[4] = {};
    std::string lastError;

    // geometry
    int nCh = 0;          // 2 * streams
    int B = 0;            // caller's block size (the reference's blockSize / callQuantum: layer plan, chunking)
    int P0 = 0;           // the reference's layer-0 partition = getLatency(): nextPow2(max(B, 64))
    int P = 0;            // internal partition size (samples) == complex bins per packed spectrum; multiple of B
    int kCap = 0;         // partition capacity per IR slot (multiple of kMacMaxTile)
    int hRows = 0;        // kCap + prefetch rows allocated per IR slot
    int ringSlots = 0;    // FDL ring slots per channel (power of two)
    int tMax = 0;
    int macTile = 16;
    bool anyCalls = false;  // CPQ_CALLS_ANY: any call quantum, ragged calls; every stream runs in a plan group
    int maxCall = 0;        // samples per call the engine is sized for (max_blocks_per_call * block_size)

    // device arena
    cpqi::DeviceBuffer<char> arena;
    int64_t arenaBytes = 0;
    double2* X = nullptr;       // [nCh][ringSlots][e->P]       FDL ring of packed spectra
    double2* XDN = nullptr;     // [nCh][ringSlots]           (DC, Nyquist) of every FDL slot
    double2* H = nullptr;       // [nCh][hRows][e->P]           IR partition spectra per IR slot
    double2* HDN = nullptr;     // [nCh][hRows]
    double2* Y = nullptr;       // [nCh][tMax][e->P]            accumulated output spectra of the call
    double* hist[2] = { nullptr, nullptr };   // [nCh][e->P]    overlap history, ping-pong
    cpqi::DeviceBuffer<double> stageIn;  // [nCh][tMax*e->P]             staging for the host-pointer entry points (allocated on first use)
    cpqi::DeviceBuffer<double> stageOut;
    cpqi::DeviceBuffer<double> mid;      // [nCh][tMax*e->P]             conv <-> EQ hand-off (not used when in place)
    double* heffDev = nullptr;  // staging for one h_eff upload
    double* gainDev = nullptr;  // [P+1] spectral gains of a FilterSpec
    bool directHead = false;    // last set_impulse enabled the direct head (affects the processor-level dry delay)
    // direct head (allocated on first use): reversed, scaled head taps and tap count per IR slot, input history, output
    cpqi::DeviceBuffer<double> directIr;         // [nCh slots][32]
    cpqi::DeviceBuffer<int> directTaps;          // [nCh slots]
    cpqi::DeviceBuffer<double> directHist[2];   // [nCh][32] last input samples, ping-pong
    cpqi::DeviceBuffer<double> directOut;        // [nCh][tMax * P]
    int directSel = 0;
    std::vector<int> directTapsHost;    // per IR slot
    bool anyDirect = false;
    int64_t heffCap = 0;
    double2* tw512 = nullptr;
    double2* tw1024 = nullptr;
    int* irSlot = nullptr;      // [nCh] device
    cpq::CascadeTables eqTab;   // the EQ's 20 SVF bands (layouts: kernels.hpp)
    cpq::CascadeTables ofTab;   // output filter (N2): the same cascade kernels running DF-II-T sections in band slots 0..2
    void* svfChain = nullptr;   // scheduling words of the time-parallel cascade: header, arrival counters of the CUs, and (chained spans
                                // only: svfChainSpans > 0) the [channels][svfChainSpans][20][4] hand-over granules
    int svfChainSpans = 0;
    int svfChainGrid = 0;       // workgroups of the span kernel the device holds at once (2 per CU)
    unsigned long long uploadSeq = 0;   // staged uploads so far (they are ordered on the engine's stream only)
    bool ofSet = false, ofTpSafe = true, ofInPath = false;

    // run-time state
    int head = 0;               // ring slot of the next block
    int histSel = 0;
    int kActive = 0;            // max partitions over the loaded IRs (multiple of kMacMaxTile)
    int kMaxReal = 0;           // max real partition count (DC/Nyquist loop bound)
    std::vector<int> irSlotHost;
    bool irPrivate = true;      // every channel reads its own IR rows (no shared slot)
    std::vector<char> irLoaded; // per channel
    std::vector<int> irParts;   // per IR slot: partitions in use
    std::vector<char> slotSpecTail;   // per IR slot: loaded with a FilterSpec plan that has tail layers
    cpq_nuc_plan plan{};        // plan of the most recent set_impulse
    bool planValid = false;
    bool eqSet = false;
    std::vector<char> eqTpSafe; // per stream: time-parallel kernel proven guard-free
    std::vector<char> eqMidSide; // per stream: some active band filters the Mid or Side component
    // last parameters per stream, re-designed when prepare() changes the sample rate (EQProcessor::prepareToPlay rebuilds
    // its band nodes on a rate change, src/eqprocessor/EQProcessor.Core.cpp:679-826; OutputFilter::prepare likewise)
    std::vector<cpq_eq_params> eqParamsHost;
    std::vector<char> eqParamsSet;
    struct OfModes { int convIsLast, hc, lc, lp; };
    std::vector<OfModes> ofModesHost;
    std::vector<char> ofModesSet;
    int eqMode = CPQ_EQ_MODE_AUTO;
    int order = CPQ_ORDER_CONV_THEN_EQ;
    double sampleRate = 48000.0;

    // total-gain LinearRamp per stream (src/DspNumericPolicy.h:319-421; 50 ms, EQProcessor.h SMOOTHING_TIME_SEC)
    std::vector<cpqi::GainRamp> gainRamp;     // per stream
    bool eqProcessed = false;           // a process call has consumed EQ parameters since prepare
    // EQ bypass per stream (EQProcessor::setBypassFromRT + the fade of the basic process(block),
    // src/eqprocessor/EQProcessor.Processing.cpp:499-526, 977-1015): LinearRamp bypassFadeGain over 5 ms
    std::vector<cpqi::EqBypass> eqBypass;
    // requestBandReset (EQProcessor.h; Processing.cpp:595-624): bands whose state is cleared at the first callback where
    // that is safe -- the block is silent, or a bypass fade is running
    std::vector<uint32_t> eqResetPending;
    std::vector<char> agcResetPending;  // requestAgcReset: envelopes and gain back to their initial values at the next processed block
    bool anyEqReset = false;
    cpqi::DeviceBuffer<int> silentDev;           // [streams][callbacks]
    cpqi::PinnedBuffer<int> silentHost;          // pinned
    bool anyEqBypass = false;           // some stream is not in the plain "never bypassed" state
    // DSPCore block routing (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:384-470)
    std::vector<double> trimHost, makeupHost;   // per stream: convolverInputTrimGain (EQ -> conv order), outputMakeupGain
    cpqi::DeviceBuffer<double> trimDev;
    cpqi::DeviceBuffer<double> makeupDev;
    bool anyTrim = false, anyMakeup = false;
    bool convBypassed = false;          // state.convBypassed: the convolver stage is not called
    std::vector<char> ofPass;           // per stream: output filter tables hold pass-through flags (nothing active)
    cpqi::DeviceBuffer<double> eqDry;            // [nCh][tMax * P] dry copy for the bypass cross-fade (allocated on first use)
    cpqi::DeviceBuffer<int> blendOn;             // [streams]
    cpqi::DeviceBuffer<int> blendLen;            // [streams] samples with their own fade gain
    cpqi::DeviceBuffer<double> blendEnd;         // [streams] gain after those
    cpqi::DeviceBuffer<double> blendGains;       // [streams][fade steps]
    int blendCap = 0;
    cpqi::DeviceBuffer<int> rampOn;              // [streams] device
    cpqi::DeviceBuffer<double> rampGains;        // [streams][callbacks][2] device

    // EQ AGC (allocated on first use)
    std::vector<int> agcOnHost;
    bool anyAgc = false;
    cpqi::DeviceBuffer<int> agcOn;           // [streams]
    cpqi::DeviceBuffer<double> agcState;     // [streams][3]
    cpqi::DeviceBuffer<double> agcRmsIn;     // [nCh][callbacks]
    cpqi::DeviceBuffer<double> agcRmsOut;
    cpqi::DeviceBuffer<double> agcGains;     // [streams][callbacks][2]

    // layered (time-varying) reference semantics: per-layer convolutions + replay of the tail delay-line reader
    bool layered = false;
    cpq_nuc_plan layerPlan{};
    int layerRow[3] = { 0, 0, 0 };      // first IR row of each layer inside a channel's slot
    int layerK[3] = { 0, 0, 0 };        // partitions per layer
    cpqi::DeviceBuffer<double> layerOut;         // [nTail][nCh][tMax*P]
    cpqi::DeviceBuffer<double> tailRing;         // [nTail][nCh][tailRingSlots]
    int tailRingSlots = 0;
    cpqi::DeviceBuffer<long long> tailState;          // device: callback counter + read cursors
    cpqi::DeviceBuffer<long long> tailSched;     // device: [nTail][tMax]

    // plan groups (engine_native.cpp): streams run on the reference's own layer plan with its Add / Get bookkeeping
    std::vector<std::unique_ptr<PlanGroup>> groups;
    std::vector<int> groupOf;           // per stream: index into groups, -1 = main (uniform) path
    bool mainActive = false;            // some loaded stream runs on the main path
    int lastCallSamples = 0;
    PinnedRing pinned;                  // small per-call host -> device tables

    // processor-level wrapper (N1)
    int convLevel = CPQ_LEVEL_NUC;
    std::vector<cpq_convproc_params> procParams;   // per stream
    std::vector<char> procBypass, procDryOnly;      // per stream: bypassed / mix <= 0.001 (the convolver is not called)
    std::vector<int> procWetOnHost;                 // per stream: what the device flags hold
    cpqi::DeviceBuffer<int> procWetOn;                       // [streams] device: 0 = the stream's output is the delayed dry signal
    bool honourFrozen = false;                      // set around the convolver call of enqueueConvProc: frozen plan groups (and their direct heads) rest
    // mix smoothing (LinearRamp mixSmoother, src/ConvolverProcessor.h:945; Runtime.cpp:340-375, 591-607): per stream
    std::vector<cpqi::MixRamp> mixRamp;
    bool procProcessed = false;         // a processor-level call has run since create / prepare: parameter changes ramp
    cpqi::DeviceBuffer<int> mixRampLen;             // [streams] device: leading samples of the call with per-sample gains
    cpqi::DeviceBuffer<double> mixRampGains;     // [streams][mixRampCap][2] device (allocated when a ramp first runs)
    int mixRampCap = 0;
    cpqi::DeviceBuffer<double> procGains;    // [streams][2] device
    cpqi::DeviceBuffer<int> procDelay;       // [streams] device
    // dry delay line: a ring per channel (the reference's 4 Mi-sample delayBuffer, Runtime.cpp:378-391), sized for the
    // longest delay an IR of max_ir_len can ask for plus one call; every call's input is written before anything reads
    cpqi::DeviceBuffer<double> dryRing;      // [nCh][dryRingSize] device, allocated on first use
    int dryRingSize = 0;
    long long dryPos = 0;           // absolute position of the next input sample
    // latency compensation (Runtime.cpp:263-290, 394-540): latencySmoother is only ever snapped, crossfadeGain runs 20 ms
    std::vector<cpqi::LatencyFade> latFade;
    cpqi::DeviceBuffer<int> latNew;          // [streams] device: delay of the dry read
    cpqi::DeviceBuffer<int> latOld;          // [streams] delay faded out
    std::vector<int> latNewHost, latOldHost;    // what the two device arrays hold
    cpqi::DeviceBuffer<int> latLen;          // [streams] samples of the range that are cross-faded
    cpqi::DeviceBuffer<double> latGains;     // [streams][latCap]
    int latCap = 0;

    // half-band oversampler (engine_os.cpp): CustomInputOversampler around the routing
    struct OsStageDev {
        int convCount = 0, upKeep = 0, downKeep = 0, centerTap = 0, centerDelay = 0;
        double centerCoeff = 0.5;
        double* coef = nullptr;                 // [convCount] device
        double* up[2] = { nullptr, nullptr };   // [nCh][upKeep] ping-pong
        double* down[2] = { nullptr, nullptr }; // [nCh][downKeep] ping-pong
        int upSel = 0, downSel = 0;             // the current history of each direction
    };
    int osFactor = 1, osType = CPQ_OS_IIR, osStages = 0;
    OsStageDev osStage[3];
    cpqi::DeviceBuffer<char> osMem;                      // coefficients and histories of the stages
    cpqi::DeviceBuffer<int> osFlags;                     // [streams][4] device (os_kernels.hip)
    cpqi::DeviceBuffer<unsigned long long> osCounts;     // [streams][2] device
    cpqi::DeviceBuffer<int> osNonSilent;                 // [3][nCh] device: silence test of each down stage
    cpqi::DeviceBuffer<double> osTmp[2];    // [nCh][maxCall / 2] stage-to-stage buffers (allocated on first use)
    cpqi::DeviceBuffer<double> osWork;                   // [nCh][tMax * P] the routing's block at the internal rate

    // soft clipper (engine_softclip.cpp): a table row per stream; at factor 1 its local 2x pair, a second oversampler instance of
    // one stage with state of its own (one group, allocated by the first call that runs it) and the pair's 2n-sample rows
    std::vector<char> scOnHost;                         // per stream
    std::vector<float> scAmountHost;
    bool anySoftClip = false;                           // some stream clips; false: nothing is launched
    cpqi::DeviceBuffer<double> scTab;                   // [streams][kSoftClipTabDoubles]
    OsStageDev scStage;                                 // 31 taps, 90 dB: the design of the third IIR-like stage
    cpqi::DeviceBuffer<double> scCoef, scUp[2], scDown[2];   // [convCount], [nCh][upKeep], [nCh][downKeep]
    cpqi::DeviceBuffer<int> scFlags, scNonSilent;       // [streams][4], [nCh]
    cpqi::DeviceBuffer<unsigned long long> scCounts;    // [streams][2]
    cpqi::DeviceBuffer<double> scWork;                  // [nCh][2 maxCall] the block at twice the rate

    // meters (engine_meter.cpp): LoudnessMeter and TruePeakDetector on the base-rate output rows, one record per callback
    int meterFlags = 0;                                // CPQ_METER_*; 0 = off
    cpqi::DeviceBuffer<double> meterTab;                // K-weighting section tables, then the two stages' FIR branches
    cpqi::DeviceBuffer<double> meterState;              // [nCh][8] x1 x2 | pre y1 y2 | rlb y1 y2
    cpqi::DeviceBuffer<double> meterHist[2];            // [nCh][32] last scrubbed inputs (true peak), ping-pong
    cpqi::DeviceBuffer<double> meterHold;               // [streams] peakHold
    cpqi::DeviceBuffer<double> meterChSum, meterChPeak; // [nCh][meterCbCap] of the call in flight
    cpqi::DeviceBuffer<unsigned long long> meterTp;     // [streams][meterCbCap]
    cpqi::DeviceBuffer<cpq_meter_block> meterRing;      // [streams][kMeterRing]
    int meterHistSel = 0, meterCbCap = 0;
    // every stream sees the same callbacks: one pair of ring counters, one block counter (LockFreeRingBuffer, blockCounter)
    unsigned long long meterWrite = 0, meterRead = 0, meterIndex = 0, meterDropped = 0;

    // output stage (engine_out.cpp): DC blocker, headroom + scrub, limiter, clamp on the base-rate output rows; one group
    int outFlags = 0;                                   // CPQ_OUT_*; 0 = off
    cpqi::DeviceBuffer<double> outTab;                  // the two DC sections' tables (kOutSectionDoubles each)
    cpqi::DeviceBuffer<double> outDc;                   // [nCh][2] one-pole states
    cpqi::DeviceBuffer<double> outEnv;                  // [streams] limiter envelopes
    double outRelease = 0.0;                            // SimplePeakLimiter::releaseCoeff at the base rate

    // dither stage (engine_dither.cpp): per channel the shaper's error taps and its generator's words; one group
    int ditherShaper = CPQ_DITHER_OFF, ditherBits = 0;
    cpq::DitherParams ditherParams{};                   // coefficients and scales at the present base rate
    cpqi::DeviceBuffer<double> ditherErr;               // [kDitherMaxOrder][nCh]
    cpqi::DeviceBuffer<unsigned long long> ditherRng;   // [4][nCh]
    cpqi::DeviceBuffer<double> ditherCoef;              // [kLatticeOrder][nCh] adaptive shaper: the stream's set in both of its channels
    std::vector<double> ditherCoefHost;                 // what ditherCoef holds

    // packed PCM entry points (engine_pcm.cpp): the call's packed input and output on the device, one group
    cpqi::DeviceBuffer<char> pcmIn, pcmOut;
    size_t pcmInCap = 0, pcmOutCap = 0;

    // profiling
    bool profiling = false;
    ProfileSlot prof[CPQ_K_COUNT];
};

namespace cpqi {

int fail(cpq_engine* e, int code, const char* fmt, ...);
// what runs without an engine (cpq_ir_resample, cpq_ir_minimum_phase, the device object of cpq_src) asks before its first HIP call:
// CPQ_OK where the current device is a gfx950, else CPQ_ERR_NO_DEVICE with the reason in cpq_last_error(NULL)
int checkCurrentDevice();

#define CPQ_HIP(e, call)                                                                            \
    do {                                                                                             \
        hipError_t err__ = (call);                                                                   \
        if (err__ != hipSuccess)                                                                     \
            return fail((e), CPQ_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(err__));      \
    } while (0)

// a step that reports a status: anything but CPQ_OK ends the calling function with it
#define CPQ_TRY(expr)                                                                                \
    do {                                                                                             \
        const int rc__ = (expr);                                                                     \
        if (rc__ != CPQ_OK) return rc__;                                                             \
    } while (0)

// the scorer's tables on the device (engine_score.cpp; cpq_scorer_create and cpq_diag_score_spectrum): the eight per-bin double
// tables and the twiddles in tabD, band / range / bandStart in tabI, dev pointing into both.  CPQ_OK, or CPQ_ERR_OOM /
// CPQ_ERR_DEVICE with the reason in `error`
struct ScoreTableBuffers {
    DeviceBuffer<double> tabD;
    DeviceBuffer<int> tabI;
    cpq::ScoreDeviceTables dev{};
};
int uploadScoreTables(const cpq::ScoreTables& t, ScoreTableBuffers& b, std::string& error);
// the scorer's shaper at `bits` (LatticeNoiseShaper::prepare) with the output stage's headroom: scale, invScale, maxV, headroom
cpq::DitherParams scoreDitherParams(int bits);

// the stream argument of an entry point, one stream or CPQ_ALL_STREAMS, as the range [s0, s1); refuses any other value
int streamRange(cpq_engine* e, int stream, int& s0, int& s1);

// AGC state [envIn, envOut, gain] of streams s0 .. s0 + n - 1 back to 0, 0, 1 on the engine's stream (agcState must exist)
int agcStateReset(cpq_engine* e, int s0, int n);

int nextPow2(int v);
int64_t alignUp(int64_t v, int64_t a);
cpq::FftTables tables(const cpq_engine* e);

// the engine's launches go to another stream while one of these is alive (declare it BEFORE the ProfScope it should cover)
struct StreamOverride {
    cpq_engine* e; hipStream_t saved;
    StreamOverride(cpq_engine* eng, hipStream_t s) : e(eng), saved(eng->stream) { e->stream = s; }
    ~StreamOverride() { e->stream = saved; }
};

struct ProfScope {
    cpq_engine* e;
    int id;
    hipEvent_t stop = nullptr;
    ProfScope(cpq_engine* eng, int kid) : e(eng), id(kid)
    {
        if (!e->profiling) return;
        ProfileSlot& s = e->prof[id];
        std::pair<hipEvent_t, hipEvent_t> ev;
        if (!s.freeList.empty()) { ev = s.freeList.back(); s.freeList.pop_back(); }
        else { (void)hipEventCreate(&ev.first); (void)hipEventCreate(&ev.second); }
        (void)hipEventRecord(ev.first, e->stream);
        stop = ev.second;
        s.pending.push_back(ev);
    }
    ~ProfScope() { if (stop) (void)hipEventRecord(stop, e->stream); }
};


int checkCall(cpq_engine* e, const void* in, const void* out, int nSamples);
int ensureCallBuffer(cpq_engine* e, DeviceBuffer<double>& buf, const char* what);

// The stages after the routing (meters, output stage, dither, PCM sanitise) run at the base rate, one callback of block_size /
// factor samples at a time.  The quotient is never 0: cpq_engine_create wants block_size >= 64 outside CPQ_CALLS_ANY, and
// cpq_engine_set_oversampling refuses a factor that does not divide block_size inside it.
inline int callbackLen(const cpq_engine* e) { return e->B / e->osFactor; }
inline double baseRate(const cpq_engine* e) { return e->sampleRate / e->osFactor; }
// what follows the base rate, redesigned and reset after it changed: meters, output stage, dither (each nothing while it is off)
int refreshBaseRateStages(cpq_engine* e);
// The refusals of a stage's own entry point on base-rate rows [nCh][n], in this order: null handle (no message), stage off
// (CPQ_ERR_NOT_READY with offText), null buffer, n outside 1..maxCall / factor, part callbacks outside CPQ_CALLS_ANY (only
// with wholeCallbacks: the oversampler's calls have no such rule), 16-byte alignment.  One buffer: pass it for both.
int checkBaseRows(cpq_engine* e, const void* in, const void* out, int n, bool on, const char* offText, bool wholeCallbacks);
// The host-pointer call of one stage, on the engine's stream: inLen samples per channel up into stageIn, body(src, dst), outLen
// samples per channel down from dst (0: nothing comes back), synchronise.  inPlace: dst is stageIn and stageOut is not allocated.
int hostRoundTrip(cpq_engine* e, const double* in, size_t inLen, double* out, size_t outLen, bool inPlace,
                  const std::function<int(const double*, double*)>& body);
// exp(-2 pi i m / P) and exp(-2 pi i m / 2P), m < P: extended precision on the host, rounded once (SURVEY.md section 7 "hard parts")
void hostTwiddles(int P, std::vector<double2>& w1, std::vector<double2>& w2);
int zeroRuntimeState(cpq_engine* e, bool conv, bool eq);

// engine_upload.cpp
int stageUpload(cpq_engine* e, void* dst, const void* src, size_t bytes);
void freePinnedRing(cpq_engine* e);
// engine_native.cpp
int resetGroups(cpq_engine* e);
int nativeSetImpulse(cpq_engine* e, int stream, const double* irL, const double* irR, int irLen, double scale, int headTaps,
                     const cpq_filter_spec* spec, const cpq_nuc_plan& pl);
int leaveNativeGroup(cpq_engine* e, int stream);
int setStreamFrozen(cpq_engine* e, int stream, bool frozen);
void clearFrozen(cpq_engine* e);           // no plan group rests any more (conv level change, reset, prepare)
int groupsAppend(cpq_engine* e, const double* dIn, int n);
int groupsRunLayer0(cpq_engine* e, double* dOut, int n);
int groupsRunTails(cpq_engine* e, double* dOut, int n);
// engine_conv.cpp
int enqueueConv(cpq_engine* e, const double* dIn, double* dOut, int n);
// seg = taps[0 .. len) times scale (a scale within 1e-12 of 1 is not applied) with the first headTaps taps zeroed: they leave the FFT
// path for the direct head.  zeroThenScale: the order of the two steps, which decides the sign of the zeroed taps at a negative
// scale -- plan groups zero first (-0.0), layered mode scales first (+0.0), and each keeps its order: the spectra's bits depend on it.
void prepareSegment(const double* taps, int len, double scale, int headTaps, bool zeroThenScale, std::vector<double>& seg);
void zeroHead(std::vector<double>& seg, int headTaps);      // the second step alone, for a segment that arrives scaled (buildHeff)
// Host taps -> partition spectra of one IR slot, the one way an IR reaches the device: rows H / HDN of nParts partitions of P
// samples, transformed with tw (and scratch where P > 4096); gainDev: P + 1 doubles for a gain table in flight.
struct SpectraRows { double2* H; double2* HDN; cpq::FftTables tw; int P, nParts; double2* scratch; double* gainDev; };
// Refuses a segment above the staging capacity (layer: for the message), clears the first clearRows rows (0: none), uploads seg,
// transforms it, multiplies the spectra by gainsA and then gainsB (FilterSpec gains, air absorption; null or empty: none), checks
// the launches and synchronises: the staging buffers and the caller's vectors are free when it returns.
int loadSpectra(cpq_engine* e, int layer, const std::vector<double>& seg, const SpectraRows& r, int clearRows,
                const std::vector<double>* gainsA, const std::vector<double>* gainsB);
// engine_proc.cpp
int uploadProcParams(cpq_engine* e);
int enqueueConvProc(cpq_engine* e, const double* dIn, double* dOut, int n);
// engine_os.cpp
void freeOversampler(cpq_engine* e);
int resetOversampler(cpq_engine* e);            // reset(): histories and flags, not the counters
int enqueueOsChain(cpq_engine* e, const double* dIn, double* dOut, int nBase);
// One CustomInputOversampler as the stage kernels are to drive it: its stages, its per-stream flags [4] and counts [2], the
// silence tests [stage][nCh of the instance], and the channels ch0 .. ch0 + nCh - 1 of it that take part (whole streams; a part
// of an instance only where it has a single stage).  Rows are the engine's [channel][stride]; channel ch0 is at ch0 * stride.
struct OsView {
    cpq_engine::OsStageDev* stage;
    int nStages;
    int* flags;
    unsigned long long* counts;
    int* nonSilent;
    int ch0, nCh;
};
// processUp / processDown of the view's channels, under CPQ_K_OS.  Neither moves the ping-pong selectors: the caller flips a
// direction once every channel of the instance has run it, and flips up before any down (whose prologue tests the new histories)
int enqueueOsUp(cpq_engine* e, const OsView& v, const double* in, int64_t inStride, double* out, int64_t outStride, int nBase);
int enqueueOsDown(cpq_engine* e, const OsView& v, const double* in, int64_t inStride, double* out, int64_t outStride, int nBase);
void flipOsUp(const OsView& v);
void flipOsDown(const OsView& v);
// engine_softclip.cpp
// the clipper in place on rows at the processing rate, callbacks of cb samples; launches nothing while no stream clips
int enqueueSoftClipRows(cpq_engine* e, double* rows, int64_t stride, int n, int cb);
// factor 1: softClipOS.processUp, the clipper on 2 n samples, softClipOS.processDown back into the rows, for the streams that clip
int ensureSoftClipStage(cpq_engine* e);
int enqueueSoftClipLocal(cpq_engine* e, double* rows, int n);
int resetSoftClipStage(cpq_engine* e);          // histories and flags of the local stage, not its counters; nothing before it exists
// engine_meter.cpp
constexpr int kMeterRing = 4096;                // LockFreeRingBuffer<BlockPower, 4096>
int refreshMeters(cpq_engine* e);               // redesign for the present base rate and reset; nothing while metering is off
int checkMeterCall(cpq_engine* e, int nBase);   // true peak's own refusals, before anything is enqueued
int enqueueMeters(cpq_engine* e, const double* rows, int64_t stride, int nBase);
// engine_out.cpp
int refreshOutStage(cpq_engine* e);             // redesign for the present base rate and reset; nothing while the stage is off
// the steps before the meters (DC blocker, headroom + scrub) and after them (limiter, clamp); in == out allowed.  A half whose
// flags are off launches nothing and leaves out untouched
// headroom = false: the DC blocker alone (the whole-chain call with dither on, where the shaper applies headroom and scrub)
int enqueueOutPre(cpq_engine* e, const double* in, int64_t inStride, double* out, int64_t outStride, int nBase, bool headroom = true);
int enqueueOutPost(cpq_engine* e, const double* in, int64_t inStride, double* out, int64_t outStride, int nBase);
// engine_dither.cpp
// prepare() at the present base rate: coefficients, errors cleared, the 15-tap shaper reseeded; the adaptive shaper's per-stream
// coefficients stay
int refreshDither(cpq_engine* e);
// headroom, shaper and (with CPQ_OUT_HEADROOM) the scrub; launches nothing while dither is off
int enqueueDither(cpq_engine* e, const double* in, int64_t inStride, double* out, int64_t outStride, int nBase);
// engine_core.cpp: DSPCore's routing of one block (conv / EQ in the configured order, output filter, makeup)
int enqueueBoth(cpq_engine* e, const double* a, double* b, int n);
// the whole-chain call behind cpq_engine_process_block: oversampling around the routing, then the output stage with the meters
// between its two halves; and its refusals
int meteredChain(cpq_engine* e, const double* a, double* b, int n);
int checkBlockCall(cpq_engine* e, const void* in, const void* out, int nSamples);
// engine_eq.cpp
void syncEqBypass(cpq_engine* e);
int enqueueEq(cpq_engine* e, const double* dIn, double* dOut, int n);
int enqueueOutFilter(cpq_engine* e, const double* dIn, double* dOut, int n);
// output filter tables of stream s to pass-through flags (nothing active) or back to its three sections, on the engine's stream
int setOutFilterPass(cpq_engine* e, int s, bool pass);

// Host-pointer entry points: H2D, the kernel sequence and D2H.  Long calls are cut into four time chunks (each a complete
// engine call: the state carries over on the engine's stream) so that the upload of chunk i+1 and the download of chunk
// i-1 run on two copy streams beside the kernels of chunk i.  With pinned caller buffers (cpq_host_register) the three
// overlap; pageable buffers take the plain upload / kernels / download sequence.
// factor > 1 (oversampled routing): the caller's nSamples are base-rate samples, checked and partitioned at nSamples * factor,
// so every chunk is whole internal partitions; body receives base-rate chunk lengths.
// What crosses the bus is the Io's business -- fp64 rows (RowsHostIo, viaStaging) or packed PCM (engine_pcm.cpp) -- the cut of
// the call, the streams and the events are this one loop's: body always sees chunk i at stageIn / stageOut + i * nCh * chunkLen.
//   hostIn() / hostOut()                         the caller's two buffers (checked, asked for pinnedness)
//   uploadAll(n) / downloadAll(n)                the whole call, on the engine's stream
//   uploadChunk(i, len, n) / downloadChunk(..)   time chunk i of len samples per channel, on e->copyIn / e->copyOut
template <typename Io, typename F>
int stagedCall(cpq_engine* e, Io& io, int nSamples, F&& body, int factor = 1)
{
    CPQ_TRY(checkCall(e, io.hostIn(), io.hostOut(), nSamples * factor));
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_TRY(ensureCallBuffer(e, e->stageIn, "upload staging"));
    CPQ_TRY(ensureCallBuffer(e, e->stageOut, "download staging"));
    constexpr int kChunks = 4;
    const int T = nSamples * factor / e->P;                             // partitions in the call (whole ones outside CPQ_CALLS_ANY)
    auto pinned = [](const void* p) {
        hipPointerAttribute_t a{};
        if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // plain malloc'd memory
        return a.type == hipMemoryTypeHost;
    };
    // pageable buffers: the runtime stages every copy and blocks the host, so chunking only adds strided copies
    // (measured 1157 vs 1230 M samples/s); one upload, one download
    if (e->anyCalls || T < 32 || T % kChunks != 0 || !pinned(io.hostIn()) || !pinned(io.hostOut())) {
        CPQ_TRY(io.uploadAll(e, nSamples));
        CPQ_TRY(body(e->stageIn, e->stageOut, nSamples));
        CPQ_TRY(io.downloadAll(e, nSamples));
        CPQ_HIP(e, hipStreamSynchronize(e->stream));
        return CPQ_OK;
    }
    if (!e->copyIn) {
        CPQ_HIP(e, hipStreamCreateWithFlags(&e->copyIn, hipStreamNonBlocking));
        CPQ_HIP(e, hipStreamCreateWithFlags(&e->copyOut, hipStreamNonBlocking));
        for (int i = 0; i < kChunks; ++i) {
            CPQ_HIP(e, hipEventCreateWithFlags(&e->evIn[i], hipEventDisableTiming));
            CPQ_HIP(e, hipEventCreateWithFlags(&e->evDone[i], hipEventDisableTiming));
        }
    }
    const int chunkT = T / kChunks;
    const size_t chunkLen = (size_t)chunkT * e->P / factor;              // samples per channel and chunk
    auto download = [&](int i) -> int {
        CPQ_HIP(e, hipStreamWaitEvent(e->copyOut, e->evDone[i], 0));
        return io.downloadChunk(e, i, chunkLen, nSamples);
    };
    for (int i = 0; i < kChunks; ++i) {
        double* dIn = e->stageIn + (size_t)i * e->nCh * chunkLen;
        double* dOut = e->stageOut + (size_t)i * e->nCh * chunkLen;
        CPQ_TRY(io.uploadChunk(e, i, chunkLen, nSamples));
        CPQ_HIP(e, hipEventRecord(e->evIn[i], e->copyIn));
        CPQ_HIP(e, hipStreamWaitEvent(e->stream, e->evIn[i], 0));
        const int rc = body(dIn, dOut, (int)chunkLen);
        if (rc != CPQ_OK) { (void)hipDeviceSynchronize(); return rc; }      // nothing of the other chunks stays in flight
        CPQ_HIP(e, hipEventRecord(e->evDone[i], e->stream));
        if (i > 0) CPQ_TRY(download(i - 1));
    }
    CPQ_TRY(download(kChunks - 1));
    CPQ_HIP(e, hipStreamSynchronize(e->copyOut));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

// fp64 rows [nCh][nSamples] on both sides: the copies land in, and leave from, the staging rows themselves
struct RowsHostIo {
    const double* in;
    double* out;
    const void* hostIn() const { return in; }
    const void* hostOut() const { return out; }
    int uploadAll(cpq_engine* e, int n) const
    {
        CPQ_HIP(e, hipMemcpyAsync(e->stageIn, in, (size_t)e->nCh * n * sizeof(double), hipMemcpyHostToDevice, e->stream));
        return CPQ_OK;
    }
    int downloadAll(cpq_engine* e, int n) const
    {
        CPQ_HIP(e, hipMemcpyAsync(out, e->stageOut, (size_t)e->nCh * n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        return CPQ_OK;
    }
    int uploadChunk(cpq_engine* e, int i, size_t chunkLen, int n) const
    {
        const size_t hostPitch = (size_t)n * sizeof(double), devPitch = chunkLen * sizeof(double);
        CPQ_HIP(e, hipMemcpy2DAsync(e->stageIn + (size_t)i * e->nCh * chunkLen, devPitch, in + i * chunkLen, hostPitch, devPitch,
                                    (size_t)e->nCh, hipMemcpyHostToDevice, e->copyIn));
        return CPQ_OK;
    }
    int downloadChunk(cpq_engine* e, int i, size_t chunkLen, int n) const
    {
        const size_t hostPitch = (size_t)n * sizeof(double), devPitch = chunkLen * sizeof(double);
        CPQ_HIP(e, hipMemcpy2DAsync(out + i * chunkLen, hostPitch, e->stageOut + (size_t)i * e->nCh * chunkLen, devPitch, devPitch,
                                    (size_t)e->nCh, hipMemcpyDeviceToHost, e->copyOut));
        return CPQ_OK;
    }
};

template <typename F>
int viaStaging(cpq_engine* e, const double* in, double* out, int nSamples, F&& body, int factor = 1)
{
    RowsHostIo io{ in, out };
    return stagedCall(e, io, nSamples, body, factor);
}

}  // namespace cpqi
