// convopeq_mi355x.hpp -- header-only C++20 adapter over the C ABI (convopeq_mi355x.h).
//
// Gives reference-style callers the member-function names of the reference's hot-path surface, batched over
// S stereo streams:
//   cpq::BatchedConvolver  ::SetImpulse / Add / Get / Reset / isReady / getLatency
//        <- convo::MKLNonUniformConvolver (src/MKLNonUniformConvolver.h:197-242), one instance per mono channel
//           in the reference, here one object for every channel of every stream
//   cpq::BatchedMeters      ::prepare / processBlock / readBlocks / reset          <- LoudnessMeter + TruePeakDetector (src/LoudnessMeter.h, src/TruePeakDetector.h)
//   cpq::BatchedOutputStage ::prepare / process / envelope / reset                 <- DSPCore::processOutputDouble, dither off
//   cpq::BatchedOversampler ::prepare / processUp / processDown / reset   <- CustomInputOversampler (src/CustomInputOversampler.h)
//   cpq::BatchedProcessor  ::prepareToPlay / process / setEqParameters / loadImpulse
//        <- ConvolverProcessor::{prepareToPlay,process} (src/ConvolverProcessor.h:226,259) and
//           EQProcessor::{prepareToPlay,process(block, params, cache)} (src/eqprocessor/EQProcessor.h:189-205)
// Same argument meaning and error behaviour as the reference: bool / sample-count returns, never throws on the
// processing path, a failed call leaves the output zeroed (the reference's fail-closed FFT policy,
// src/MKLNonUniformConvolver.cpp:75-82) -- and, unlike the reference's void returns, every call that can fail also reports
// it: Add / process / prepareToPlay return false, lastStatus() / lastError() say why.
// Call sizes: a power-of-two block (64..4096) runs the throughput path (calls of whole blocks); any other block size
// (480, 441, 96 ...) or CallMode::Any selects CPQ_CALLS_ANY, where every call length is accepted and the reference's
// inputPos accumulation / ring zero-fill are reproduced chunk by chunk.
#pragma once

#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "convopeq_mi355x.h"

namespace cpq {

// planar block of all streams: channels()[c] points at numSamples doubles (juce::dsp::AudioBlock<double> is
// `double* const* channels, numChannels, numSamples`; here numChannels = 2 * streams)
struct AudioBlockBatch {
    double* const* channels;
    int numChannels;
    int numSamples;
};

// RAII pin of a caller-owned PCM buffer (cpq_host_register): the host-pointer entry points pipeline upload, kernels and
// download only for pinned memory.
class PinnedRegion {
public:
    PinnedRegion(void* ptr, size_t bytes) : ptr_(cpq_host_register(ptr, bytes) == CPQ_OK ? ptr : nullptr) {}
    ~PinnedRegion() { if (ptr_) (void)cpq_host_unregister(ptr_); }
    PinnedRegion(const PinnedRegion&) = delete;
    PinnedRegion& operator=(const PinnedRegion&) = delete;
    bool ok() const { return ptr_ != nullptr; }
private:
    void* ptr_;
};

enum class CallMode { Auto, WholeBlocks, Any };      // Auto: whole blocks for a power-of-two block size, else any

class Engine {
public:
    Engine(int streams, int blockSize, int maxIrLen, int maxBlocksPerCall, double sampleRate = 48000.0,
           cpq_semantics semantics = CPQ_SEM_REFERENCE, int device = 0, int partitionSize = 0,
           cpq_schedule schedule = CPQ_SCHED_UNIFORM, CallMode calls = CallMode::Auto)
    {
        const bool pow2 = blockSize >= 64 && blockSize <= 4096 && (blockSize & (blockSize - 1)) == 0;
        anyCalls_ = calls == CallMode::Any || (calls == CallMode::Auto && !pow2);
        cpq_engine_desc d{};
        d.struct_size = static_cast<int32_t>(sizeof(d));
        d.device = device;
        d.n_streams = streams;
        d.block_size = blockSize;
        d.max_ir_len = maxIrLen;
        d.max_blocks_per_call = maxBlocksPerCall;
        d.semantics = semantics;
        d.mac_tile = 0;
        d.sample_rate = sampleRate;
        d.partition_size = partitionSize;
        d.schedule = schedule;
        d.call_mode = anyCalls_ ? CPQ_CALLS_ANY : CPQ_CALLS_WHOLE_BLOCKS;
        cpq_engine* raw = nullptr;
        const int rc = cpq_engine_create(&d, &raw);
        if (rc != CPQ_OK) throw std::runtime_error(std::string("cpq_engine_create: ") + cpq_last_error(nullptr));
        h_.reset(raw);
        streams_ = streams;
        block_ = blockSize;
        maxCall_ = blockSize * maxBlocksPerCall;
    }
    cpq_engine* get() const noexcept { return h_.get(); }
    int streams() const noexcept { return streams_; }
    int channels() const noexcept { return 2 * streams_; }
    int blockSize() const noexcept { return block_; }
    int maxSamplesPerCall() const noexcept { return maxCall_; }
    bool acceptsAnyCallSize() const noexcept { return anyCalls_; }
    const char* lastError() const noexcept { return cpq_last_error(h_.get()); }

private:
    struct Deleter { void operator()(cpq_engine* e) const noexcept { cpq_engine_destroy(e); } };
    std::unique_ptr<cpq_engine, Deleter> h_;
    int streams_ = 0, block_ = 0, maxCall_ = 0;
    bool anyCalls_ = false;
};

// ---------------------------------------------------------------------------------------------------------------
class BatchedConvolver {
public:
    explicit BatchedConvolver(Engine& e) : e_(e), pending_(static_cast<size_t>(e.channels()) * e.maxSamplesPerCall()),
                                           result_(pending_.size()) {}

    // one shared stereo IR for every stream (CPQ_ALL_STREAMS) or one stream's IR; arguments as
    // MKLNonUniformConvolver::SetImpulse(impulse, irLen, blockSize, scale, enableDirectHead, filterSpec)
    bool SetImpulse(int stream, const double* impulseL, const double* impulseR, int irLen, int blockSize,
                    double scale = 1.0, bool enableDirectHead = false, const cpq_filter_spec* filterSpec = nullptr)
    {
        if (blockSize != e_.blockSize()) return false;
        return cpq_conv_set_impulse(e_.get(), stream, impulseL, impulseR, irLen, scale, enableDirectHead ? 1 : 0,
                                    filterSpec) == CPQ_OK;
    }

    // Add: input planar [channel][numSamples]; nullptr = silence (reference :205-208).  false (and lastStatus() != CPQ_OK)
    // when the engine refused the call -- e.g. a call that is not whole blocks on a CallMode::WholeBlocks engine
    bool Add(const double* input, int numSamples)
    {
        have_ = 0;
        status_ = CPQ_ERR_INVALID_ARG;
        if (numSamples <= 0 || numSamples > e_.maxSamplesPerCall()) return false;
        const size_t n = static_cast<size_t>(e_.channels()) * numSamples;
        if (input) std::memcpy(pending_.data(), input, n * sizeof(double));
        else std::memset(pending_.data(), 0, n * sizeof(double));
        status_ = cpq_conv_process(e_.get(), pending_.data(), result_.data(), numSamples);
        if (status_ == CPQ_OK) have_ = numSamples;
        return status_ == CPQ_OK;
    }

    // Get: the block of the preceding Add.  Returns the samples layer 0's ring delivered (the smallest count over the
    // streams; short reads are zero-filled at the end of every chunk exactly as ringRead does, :1376-1402), 0 and a zeroed
    // output when nothing is available (reference :1560-1562)
    int Get(double* output, int numSamples)
    {
        if (numSamples <= 0) return 0;
        const size_t n = static_cast<size_t>(e_.channels()) * numSamples;
        if (have_ != numSamples) {
            if (output) std::memset(output, 0, n * sizeof(double));
            return 0;
        }
        if (output) std::memcpy(output, result_.data(), n * sizeof(double));
        have_ = 0;
        int got = numSamples;
        for (int s = 0; s < e_.streams(); ++s) {
            const int g = cpq_conv_last_got(e_.get(), s);
            if (g >= 0 && g < got) got = g;
        }
        return got;
    }

    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return e_.lastError(); }

    void Reset() { cpq_conv_reset(e_.get()); }
    bool isReady() const noexcept { return cpq_conv_is_ready(e_.get()) != 0; }
    int getLatency() const noexcept { return cpq_conv_latency(e_.get()); }

private:
    Engine& e_;
    std::vector<double> pending_, result_;
    int have_ = 0, status_ = CPQ_OK;
};

// ---------------------------------------------------------------------------------------------------------------
class BatchedProcessor {
public:
    explicit BatchedProcessor(Engine& e) : e_(e), scratch_(static_cast<size_t>(e.channels()) * e.maxSamplesPerCall()) {}

    bool prepareToPlay(double sampleRate, int samplesPerBlock)
    {
        status_ = cpq_engine_prepare(e_.get(), sampleRate, samplesPerBlock);
        return status_ == CPQ_OK;
    }

    bool loadImpulse(int stream, const double* irL, const double* irR, int irLen, double scale = 1.0)
    {
        return cpq_conv_set_impulse(e_.get(), stream, irL, irR, irLen, scale, 0, nullptr) == CPQ_OK;
    }

    // IR file -> conditioned IR -> SetImpulse + peak latency, as the reference's loader thread does for one processor
    // (LoaderThread::doLoadStep .. buildConvolverFromTrimmed); a mono file feeds both channels
    bool loadImpulseFile(int stream, const char* wavPath, double sampleRate, float targetIrLengthSec = 1.0f,
                         cpq_phase_mode phase = CPQ_PHASE_AS_IS, const cpq_filter_spec* spec = nullptr, float mix = 1.0f)
    {
        cpq_ir_buffer file{};
        if (cpq_ir_load_wav(wavPath, &file) != CPQ_OK) return false;
        cpq_ir_prepared prep{};
        const bool ok = cpq_ir_prepare(&file, sampleRate, targetIrLengthSec, phase, nullptr, 1.0, &prep) == CPQ_OK;
        cpq_ir_buffer_free(&file);
        if (!ok) return false;
        const double* l = prep.ir.data;
        const double* r = prep.ir.n_channels > 1 ? prep.ir.data + prep.ir.n_samples : l;
        bool done = cpq_conv_set_impulse(e_.get(), stream, l, r, prep.ir.n_samples, prep.scale.scale_factor, 0, spec) == CPQ_OK;
        const cpq_convproc_params pp{ mix, 0, prep.ir_peak_latency, 0.0f };
        done = done && cpq_convproc_set_params(e_.get(), stream, &pp) == CPQ_OK;
        cpq_ir_prepared_free(&prep);
        return done;
    }

    bool setEqParameters(int stream, const cpq_eq_params& p) { return cpq_eq_set_params(e_.get(), stream, &p) == CPQ_OK; }
    void setProcessingOrder(cpq_order o) { cpq_engine_set_order(e_.get(), o); }
    // EQProcessor::setBypassFromRT / requestBandReset, per stream
    void setBypassFromRT(int stream, bool bypassed) { cpq_eq_set_bypass(e_.get(), stream, bypassed ? 1 : 0); }
    void requestBandReset(int stream, uint32_t mask) { cpq_eq_request_band_reset(e_.get(), stream, mask); }
    void requestAgcReset(int stream) { cpq_eq_request_agc_reset(e_.get(), stream); }
    // DSPCore's remaining per-block routing values
    void setConvolverBypassed(bool bypassed) { cpq_engine_set_conv_bypass(e_.get(), bypassed ? 1 : 0); }
    void setGains(int stream, double convolverInputTrimGain, double outputMakeupGain)
    {
        cpq_engine_set_gains(e_.get(), stream, convolverInputTrimGain, outputMakeupGain);
    }

    // in-place on the planar block, like ConvolverProcessor::process / EQProcessor::process; a refused or failed call
    // clears the block (fail closed) AND returns false with the reason in lastStatus() / lastError()
    bool process(AudioBlockBatch& block)
    {
        const int n = block.numSamples;
        status_ = CPQ_ERR_INVALID_ARG;
        if (n <= 0 || block.numChannels != e_.channels() || n > e_.maxSamplesPerCall()) { clear(block); return false; }
        for (int c = 0; c < block.numChannels; ++c)
            std::memcpy(scratch_.data() + static_cast<size_t>(c) * n, block.channels[c], sizeof(double) * n);
        status_ = cpq_engine_process_block(e_.get(), scratch_.data(), scratch_.data(), n);
        if (status_ != CPQ_OK) { clear(block); return false; }
        for (int c = 0; c < block.numChannels; ++c)
            std::memcpy(block.channels[c], scratch_.data() + static_cast<size_t>(c) * n, sizeof(double) * n);
        return true;
    }

    // float in, float out, as DSPCore::processInput / processOutput hand the chain its blocks: planar rows
    // [channel][numSamples] of float32 on both sides (16-byte aligned; the same buffer, or two that do not overlap), widened
    // and narrowed on the device.  A refused or failed call zeroes `out` and returns false.
    bool process(const float* in, float* out, int numSamples)
    {
        status_ = cpq_engine_process_block_pcm(e_.get(), in, CPQ_PCM_F32, out, CPQ_PCM_F32, CPQ_PCM_PLANAR, 0u, numSamples);
        if (status_ == CPQ_OK) return true;
        if (out && numSamples > 0) std::memset(out, 0, sizeof(float) * static_cast<size_t>(e_.channels()) * numSamples);
        return false;
    }

    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return e_.lastError(); }

private:
    static void clear(AudioBlockBatch& b)
    {
        for (int c = 0; c < b.numChannels; ++c) std::memset(b.channels[c], 0, sizeof(double) * b.numSamples);
    }
    Engine& e_;
    std::vector<double> scratch_;
    int status_ = CPQ_OK;
};

// ---------------------------------------------------------------------------------------------------------------
// CustomInputOversampler (src/CustomInputOversampler.h) for every stream of an engine: prepare / processUp / processDown /
// reset.  The engine keeps describing the processing (oversampled) domain, as DSPCore prepares conv and EQ at
// sampleRate * factor; processUp takes base-rate blocks, processDown returns them.  Host buffers, staged per call.
class BatchedOversampler {
public:
    enum class Preset { IIRLike = CPQ_OS_IIR, LinearPhase = CPQ_OS_LINEAR_PHASE };
    explicit BatchedOversampler(Engine& e) : e_(e) {}

    // CustomInputOversampler::prepare(maxInputBlockSize, ratio, preset): ratio 1, 2, 4 or 8
    bool prepare(int ratio, Preset preset = Preset::IIRLike)
    {
        status_ = cpq_engine_set_oversampling(e_.get(), ratio, static_cast<int32_t>(preset));
        if (status_ == CPQ_OK) ratio_ = ratio;
        return status_ == CPQ_OK;
    }
    int getOversamplingFactor() const noexcept { return ratio_; }
    // in: numSamples base-rate samples per channel; out: numSamples * factor.  false (out zeroed) on failure
    bool processUp(const AudioBlockBatch& in, AudioBlockBatch& out) { return run(in, out, true); }
    // in: numSamples * factor per channel; out: numSamples (= in.numSamples / factor)
    bool processDown(const AudioBlockBatch& in, AudioBlockBatch& out) { return run(in, out, false); }
    void reset() { status_ = cpq_os_reset(e_.get()); }
    bool telemetry(int stream, cpq_os_telemetry& t) { return (status_ = cpq_os_read_telemetry(e_.get(), stream, &t)) == CPQ_OK; }
    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return e_.lastError(); }

private:
    bool run(const AudioBlockBatch& in, AudioBlockBatch& out, bool up)
    {
        const int nBase = up ? in.numSamples : out.numSamples;
        const int nIn = in.numSamples, nOut = out.numSamples;
        if (in.numChannels != e_.channels() || out.numChannels != e_.channels() || nBase <= 0 ||
            (up ? nOut != nIn * ratio_ : nIn != nOut * ratio_)) {
            status_ = CPQ_ERR_INVALID_ARG;
            clear(out);
            return false;
        }
        scratchIn_.resize(static_cast<size_t>(e_.channels()) * nIn);
        scratchOut_.resize(static_cast<size_t>(e_.channels()) * nOut);
        for (int c = 0; c < in.numChannels; ++c) std::memcpy(scratchIn_.data() + static_cast<size_t>(c) * nIn, in.channels[c], sizeof(double) * nIn);
        status_ = up ? cpq_os_up(e_.get(), scratchIn_.data(), scratchOut_.data(), nBase)
                     : cpq_os_down(e_.get(), scratchIn_.data(), scratchOut_.data(), nBase);
        if (status_ != CPQ_OK) { clear(out); return false; }
        for (int c = 0; c < out.numChannels; ++c) std::memcpy(out.channels[c], scratchOut_.data() + static_cast<size_t>(c) * nOut, sizeof(double) * nOut);
        return true;
    }
    static void clear(AudioBlockBatch& b)
    {
        for (int c = 0; c < b.numChannels; ++c) std::memset(b.channels[c], 0, sizeof(double) * b.numSamples);
    }
    Engine& e_;
    std::vector<double> scratchIn_, scratchOut_;
    int ratio_ = 1;
    int status_ = CPQ_OK;
};

// ---------------------------------------------------------------------------------------------------------------
// LoudnessMeter + TruePeakDetector (src/LoudnessMeter.h, src/TruePeakDetector.h) for every stream of an engine.  Once
// prepared, cpq_engine_process_block meters its own output; processBlock meters caller blocks without running the chain.
class BatchedMeters {
public:
    explicit BatchedMeters(Engine& e) : e_(e) {}
    // loudness and / or truePeak; both false switches metering off
    bool prepare(bool loudness = true, bool truePeak = true)
    {
        status_ = cpq_engine_set_metering(e_.get(), (loudness ? CPQ_METER_LOUDNESS : 0) | (truePeak ? CPQ_METER_TRUE_PEAK : 0));
        return status_ == CPQ_OK;
    }
    bool processBlock(const AudioBlockBatch& in)
    {
        if (in.numChannels != e_.channels() || in.numSamples <= 0) { status_ = CPQ_ERR_INVALID_ARG; return false; }
        scratch_.resize(static_cast<size_t>(e_.channels()) * in.numSamples);
        for (int c = 0; c < in.numChannels; ++c)
            std::memcpy(scratch_.data() + static_cast<size_t>(c) * in.numSamples, in.channels[c], sizeof(double) * in.numSamples);
        return (status_ = cpq_meter_process(e_.get(), scratch_.data(), in.numSamples)) == CPQ_OK;
    }
    // pops up to maxBlocks records per stream into out[stream * maxBlocks + i]; returns the count per stream, -1 on failure
    int readBlocks(cpq_meter_block* out, int maxBlocks, int64_t* dropped = nullptr)
    {
        int32_t n = 0;
        status_ = cpq_meter_read_blocks(e_.get(), out, maxBlocks, &n, dropped);
        return status_ == CPQ_OK ? n : -1;
    }
    void reset() { status_ = cpq_meter_reset(e_.get()); }
    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return e_.lastError(); }

private:
    Engine& e_;
    std::vector<double> scratch_;
    int status_ = CPQ_OK;
};

// ---------------------------------------------------------------------------------------------------------------
// DSPCore's soft clipper (state.softClipEnabled / state.saturationAmount) for the streams of an engine.  Once enabled,
// cpq_engine_process_block clips between the make-up gain and the oversampler's down stages -- at factor 1 inside a local 2x
// pair that adds latency() base-rate samples.
class BatchedSoftClip {
public:
    explicit BatchedSoftClip(Engine& e) : e_(e) {}
    // stream: an index or CPQ_ALL_STREAMS; saturationAmount in 0 .. 1
    bool set(int stream, bool enabled, float saturationAmount)
    {
        return (status_ = cpq_engine_set_soft_clip(e_.get(), stream, enabled ? 1 : 0, saturationAmount)) == CPQ_OK;
    }
    static double latency(int oversamplingFactor) { return cpq_soft_clip_latency(oversamplingFactor); }
    void reset() { status_ = cpq_soft_clip_reset(e_.get()); }
    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return e_.lastError(); }

private:
    Engine& e_;
    int status_ = CPQ_OK;
};

// ---------------------------------------------------------------------------------------------------------------
// DSPCore's output stage (processOutputDouble with dither off: DC blocker, headroom + scrub, SimplePeakLimiter, clamp) for
// every stream of an engine.  Once prepared, cpq_engine_process_block passes its own output through it; process runs it on
// caller blocks, in place, without the chain.
class BatchedOutputStage {
public:
    explicit BatchedOutputStage(Engine& e) : e_(e) {}
    // flags: CPQ_OUT_* bits; 0 switches the stage off
    bool prepare(int flags = CPQ_OUT_ALL) { return (status_ = cpq_engine_set_output_stage(e_.get(), flags)) == CPQ_OK; }
    bool process(AudioBlockBatch& io)
    {
        if (io.numChannels != e_.channels() || io.numSamples <= 0) { status_ = CPQ_ERR_INVALID_ARG; return false; }
        scratch_.resize(static_cast<size_t>(e_.channels()) * io.numSamples);
        for (int c = 0; c < io.numChannels; ++c)
            std::memcpy(scratch_.data() + static_cast<size_t>(c) * io.numSamples, io.channels[c], sizeof(double) * io.numSamples);
        status_ = cpq_out_process(e_.get(), scratch_.data(), scratch_.data(), io.numSamples);
        if (status_ != CPQ_OK) return false;
        for (int c = 0; c < io.numChannels; ++c)
            std::memcpy(io.channels[c], scratch_.data() + static_cast<size_t>(c) * io.numSamples, sizeof(double) * io.numSamples);
        return true;
    }
    // SimplePeakLimiter::getCurrentEnvelope of one stream; 1.0 when it cannot be read
    double envelope(int stream)
    {
        double v = 1.0;
        status_ = cpq_out_read_envelope(e_.get(), stream, &v);
        return v;
    }
    void reset() { status_ = cpq_out_reset(e_.get()); }
    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return e_.lastError(); }

private:
    Engine& e_;
    std::vector<double> scratch_;
    int status_ = CPQ_OK;
};

// ---------------------------------------------------------------------------------------------------------------
// The reference's deterministic noise shapers (FixedNoiseShaper, Fixed15TapNoiseShaper, LatticeNoiseShaper) for every stream of
// an engine: once prepared,
// cpq_engine_process_block quantises its output to bitDepth bits between the output stage's DC blocker and its limiter, and
// the PCM calls accept CPQ_PCM_S16 output when bitDepth <= 16.
class BatchedDither {
public:
    explicit BatchedDither(Engine& e) : e_(e) {}
    // shaper: CPQ_DITHER_FIXED4 / CPQ_DITHER_FIXED15 / CPQ_DITHER_ADAPTIVE9; CPQ_DITHER_OFF switches the stage off
    bool prepare(int shaper, int bitDepth) { return (status_ = cpq_engine_set_dither(e_.get(), shaper, bitDepth)) == CPQ_OK; }
    void reset() { status_ = cpq_dither_reset(e_.get()); }
    // LatticeNoiseShaper::applyMatchedCoefficients for one stream or CPQ_ALL_STREAMS: the learner's published set (its
    // sample-rate bank, bit depth and mode chosen by the caller), numCoeffs 0 .. 9; those streams' states are cleared
    bool applyMatchedCoefficients(int stream, const double* coeffs, int numCoeffs)
    {
        return (status_ = cpq_dither_set_adaptive_coeffs(e_.get(), stream, coeffs, numCoeffs)) == CPQ_OK;
    }
    // LatticeNoiseShaper::getCoefficients of one stream: the nine clamped values in use
    bool getCoefficients(int stream, double coeffs[9]) { return (status_ = cpq_dither_get_adaptive_coeffs(e_.get(), stream, coeffs)) == CPQ_OK; }
    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return e_.lastError(); }

private:
    Engine& e_;
    int status_ = CPQ_OK;
};

// ---------------------------------------------------------------------------------------------------------------
// The fitness function of the adaptive shaper's learner (NoiseShaperLearner::buildTrainingSegments, evaluateCandidate,
// evaluateCandidateMapped; MklFftEvaluator::evaluate) for nLearners learners at once; independent of Engine.  The optimiser,
// the capture queue and persistence are the caller's.
class ShaperScorer {
public:
    explicit ShaperScorer(const cpq_scorer_desc& desc) { status_ = cpq_scorer_create(&desc, &s_); }
    // the reference's settings: 18 candidates, level weights {0.4, 0.3, 0.2, 0.1}, margin 0.85, stability check on
    static cpq_scorer_desc defaults(int nLearners, double sampleRateHz, int evaluationBitDepth)
    {
        return cpq_scorer_desc{ nLearners, 18, sampleRateHz, evaluationBitDepth, { 0.4, 0.3, 0.2, 0.1 }, 0.85, 1, CPQ_SCORE_RNG_FRESH };
    }
    ~ShaperScorer() { cpq_scorer_destroy(s_); }
    ShaperScorer(const ShaperScorer&) = delete;
    ShaperScorer& operator=(const ShaperScorer&) = delete;
    bool valid() const noexcept { return s_ != nullptr; }
    // the learner's segments from the most recent samples (what AudioSegmentBuffer::copyLatest returns); returns their number
    int buildTrainingSegments(int learner, const double* left, const double* right, int numSamples)
    {
        int32_t n = 0;
        status_ = cpq_scorer_set_audio(s_, learner, left, right, numSamples, &n);
        return status_ == CPQ_OK ? n : 0;
    }
    // mapped [nLearners][numCandidates][9] -> scores [nLearners][numCandidates]; parts may be null
    bool evaluateCandidateMapped(const double* mapped, int numCandidates, double* scores, cpq_score_parts* parts = nullptr)
    {
        return (status_ = cpq_scorer_score(s_, mapped, numCandidates, scores, parts)) == CPQ_OK;
    }
    // the same from raw optimiser coordinates: tanh and clampCoeff(k, coeffSafetyMargin) first
    bool evaluateCandidate(const double* raw, int numCandidates, double* scores, cpq_score_parts* parts = nullptr)
    {
        return (status_ = cpq_scorer_score_raw(s_, raw, numCandidates, scores, parts)) == CPQ_OK;
    }
    bool setRngStart(const uint64_t state[2][4]) { return (status_ = cpq_scorer_set_rng_start(s_, state)) == CPQ_OK; }
    cpq_scorer* get() const noexcept { return s_; }
    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return cpq_scorer_last_error(s_); }

private:
    cpq_scorer* s_ = nullptr;
    int status_ = CPQ_OK;
};

// ---------------------------------------------------------------------------------------------------------------
// The reference's CMA-ES over a ShaperScorer's learners (cpq_learner): whole generations on the device.  The scorer is borrowed
// and must outlive the learner.
class ShaperLearner {
public:
    explicit ShaperLearner(ShaperScorer& scorer) { status_ = cpq_learner_create(scorer.get(), &l_); }
    ~ShaperLearner() { cpq_learner_destroy(l_); }
    ShaperLearner(const ShaperLearner&) = delete;
    ShaperLearner& operator=(const ShaperLearner&) = delete;
    bool valid() const noexcept { return l_ != nullptr; }
    // initFromParcor of one learner or CPQ_ALL_STREAMS; learner i draws from seed + i
    bool init(int learner, const double parcor[9], uint64_t seed) { return (status_ = cpq_learner_init(l_, learner, parcor, seed)) == CPQ_OK; }
    bool setParams(const cpq_learn_params& p) { return (status_ = cpq_learner_set_params(l_, &p)) == CPQ_OK; }
    // applyPhaseParams(mode, computePhase(mode, playbackSeconds)); *generationIntervalSeconds may be null
    bool applyPhase(cpq_learn_mode mode, double playbackSeconds, double* generationIntervalSeconds = nullptr)
    {
        cpq_learn_params p;
        const int phase = cpq_learn_phase(mode, playbackSeconds);
        if (phase < 1) { status_ = phase; return false; }
        if ((status_ = cpq_learn_phase_params(mode, phase, &p, generationIntervalSeconds)) != CPQ_OK) return false;
        return setParams(p);
    }
    // enqueues numGenerations of ask, score, tell and returns; the getters below wait
    bool run(int numGenerations) { return (status_ = cpq_learner_run(l_, numGenerations)) == CPQ_OK; }
    bool getState(int learner, cpq_learn_state& out) { return (status_ = cpq_learner_get_state(l_, learner, &out)) == CPQ_OK; }
    bool setState(int learner, const cpq_learn_state& in) { return (status_ = cpq_learner_set_state(l_, learner, &in)) == CPQ_OK; }
    // best_per_generation has room for the last run's generations; returns how many were written, or -1
    int history(int learner, double* bestPerGeneration)
    {
        int32_t n = 0;
        status_ = cpq_learner_read_history(l_, learner, bestPerGeneration, &n);
        return status_ == CPQ_OK ? n : -1;
    }
    // the reference's published set, tanh(toParcor(best)); the set that was scored is cpq_learn_state::best_scored
    bool published(int learner, double k[9]) { return (status_ = cpq_learner_published(l_, learner, k)) == CPQ_OK; }
    cpq_learner* get() const noexcept { return l_; }
    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return cpq_learner_last_error(l_); }

private:
    cpq_learner* l_ = nullptr;
    int status_ = CPQ_OK;
};

// ---------------------------------------------------------------------------------------------------------------
// Streaming sample-rate conversion of nChannels planar rows (cpq_src): one object per source rate in front of an Engine, computing
// on the host (CPQ_SRC_HOST) or on the device (CPQ_SRC_DEVICE), with equal bits.
class StreamResampler {
public:
    explicit StreamResampler(const cpq_src_desc& desc) { status_ = cpq_src_create(&desc, &s_); }
    // flags: CPQ_SRC_HOST or CPQ_SRC_DEVICE; 0 is CPQ_ERR_UNSUPPORTED, both CPQ_ERR_INVALID_ARG
    StreamResampler(int nChannels, double inRate, double outRate, int maxIn, uint32_t flags)
    {
        const cpq_src_desc d{ nChannels, inRate, outRate, maxIn, CPQ_RESAMPLE_LINEAR_PHASE, flags, 0 };
        status_ = cpq_src_create(&d, &s_);
    }
    ~StreamResampler() { cpq_src_destroy(s_); }
    StreamResampler(const StreamResampler&) = delete;
    StreamResampler& operator=(const StreamResampler&) = delete;
    bool valid() const noexcept { return s_ != nullptr; }
    int latency() const noexcept { return cpq_src_latency(s_); }
    int outCount(int numSamples, bool flush = false) const noexcept { return cpq_src_out_count(s_, numSamples, flush ? 1 : 0); }
    int maxOut() const noexcept { return cpq_src_max_out(s_); }
    bool reset() { return (status_ = cpq_src_reset(s_)) == CPQ_OK; }
    // rows [channel][stride]; returns the samples written per channel, or -1 with lastStatus() set
    int process(const double* in, int64_t inStride, int numSamples, double* out, int64_t outStride, int outCapacity, bool flush = false)
    {
        int32_t n = 0;
        status_ = cpq_src_process(s_, in, inStride, numSamples, out, outStride, outCapacity, flush ? 1 : 0, &n);
        return status_ == CPQ_OK ? n : -1;
    }
    // device object: device rows, asynchronous on the object's stream; dIn and dOut stay valid until the stream has reached the call
    int processDevice(const double* dIn, int64_t inStride, int numSamples, double* dOut, int64_t outStride, int outCapacity, bool flush = false)
    {
        int32_t n = 0;
        status_ = cpq_src_process_device(s_, dIn, inStride, numSamples, dOut, outStride, outCapacity, flush ? 1 : 0, &n);
        return status_ == CPQ_OK ? n : -1;
    }
    // device object: a hipStream_t (nullptr: the null stream); the stream used so far is synchronised first
    bool setStream(void* stream) { return (status_ = cpq_src_set_stream(s_, stream)) == CPQ_OK; }
    // device time of the launches of the last process() on a device object; -1 otherwise
    double lastKernelMs() const noexcept { return cpq_src_last_kernel_ms(s_); }
    cpq_src* get() const noexcept { return s_; }
    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return cpq_src_last_error(s_); }

private:
    cpq_src* s_ = nullptr;
    int status_ = CPQ_OK;
};

// ---------------------------------------------------------------------------------------------------------------
// Gated programme loudness (EBU R 128) of nStreams stereo programmes on the device (cpq_loudness): rows L0 R0 L1 R1 ... as an
// Engine delivers them, calls of any length, the figures readable at any time.
class ProgrammeLoudness {
public:
    ProgrammeLoudness(int nStreams, double sampleRate, double maxSeconds)
    {
        const cpq_loudness_desc d{ nStreams, sampleRate, maxSeconds, 0 };
        status_ = cpq_loudness_create(&d, &p_);
    }
    ~ProgrammeLoudness() { cpq_loudness_destroy(p_); }
    ProgrammeLoudness(const ProgrammeLoudness&) = delete;
    ProgrammeLoudness& operator=(const ProgrammeLoudness&) = delete;
    bool valid() const noexcept { return p_ != nullptr; }
    bool reset() { return (status_ = cpq_loudness_reset(p_)) == CPQ_OK; }
    // a hipStream_t (nullptr: the null stream); the stream used so far is synchronised first
    bool setStream(void* stream) { return (status_ = cpq_loudness_set_stream(p_, stream)) == CPQ_OK; }
    // host rows [2 nStreams][rowStride], synchronous
    bool process(const double* rows, int64_t rowStride, int numSamples) { return (status_ = cpq_loudness_process(p_, rows, rowStride, numSamples)) == CPQ_OK; }
    // device rows, asynchronous on the object's stream
    bool processDevice(const double* dRows, int64_t rowStride, int numSamples) { return (status_ = cpq_loudness_process_device(p_, dRows, rowStride, numSamples)) == CPQ_OK; }
    // out[nStreams]; may be called repeatedly, the programmes go on
    bool finish(cpq_loudness_result* out) { return (status_ = cpq_loudness_finish(p_, out)) == CPQ_OK; }
    // the linear gain to targetLufs, or 0 where nothing passed the gates
    static double gain(const cpq_loudness_result& r, double targetLufs)
    {
        double g = 0.0;
        return cpq_loudness_gain(&r, targetLufs, &g) == CPQ_OK ? g : 0.0;
    }
    // true peak per programme (BS.1770-4 Annex 2): switched at the start of a programme only; out[nStreams], linear
    bool setTruePeak(bool on) { return (status_ = cpq_loudness_set_true_peak(p_, on ? 1 : 0)) == CPQ_OK; }
    bool readPeaks(cpq_loudness_peaks* out) { return (status_ = cpq_loudness_read_peaks(p_, out)) == CPQ_OK; }
    // the smaller of the gain to targetLufs and the gain that brings the largest peak to maxDbtp (limited: the ceiling won), or 0
    // where nothing passed the gates
    static double gainLimited(const cpq_loudness_result& r, const cpq_loudness_peaks& pk, double targetLufs, double maxDbtp, bool* limited = nullptr)
    {
        double g = 0.0;
        int32_t lim = 0;
        if (cpq_loudness_gain_limited(&r, &pk, targetLufs, maxDbtp, &g, &lim) != CPQ_OK) return 0.0;
        if (limited) *limited = lim != 0;
        return g;
    }
    // dOut = dIn * gains[stream] on device rows, asynchronous on the object's stream; in place with the same pointer and stride
    bool applyDevice(const double* gains, const double* dIn, int64_t inStride, double* dOut, int64_t outStride, int numSamples)
    {
        return (status_ = cpq_loudness_apply_device(p_, gains, dIn, inStride, dOut, outStride, numSamples)) == CPQ_OK;
    }
    cpq_loudness* get() const noexcept { return p_; }
    int lastStatus() const noexcept { return status_; }
    const char* lastError() const noexcept { return cpq_loudness_last_error(p_); }

private:
    cpq_loudness* p_ = nullptr;
    int status_ = CPQ_OK;
};

}  // namespace cpq
