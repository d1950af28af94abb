// engine_proc.cpp -- processor-level convolver stage: dry delay ring, mix ramp, latency cross-fade, cpq_convproc_* (see engine_internal.hpp, include/convopeq_mi355x.h).
// The plan of a call (who rests, the mix ramp's prefix, the latency fade's ranges) and the stage's arithmetic are host_replay.hpp's.
#include "engine_internal.hpp"

using namespace cpqi;

// ----------------------------------------------------------------- convolver, processor level (N1)
namespace cpqi {

static int procDelayOf(const cpq_engine* e, int s) { return procDelay(e->directHead, e->P0, (int)e->procParams[s].ir_peak_latency); }

int uploadProcParams(cpq_engine* e)
{
    const int S = e->desc.n_streams;
    std::vector<double> g((size_t)S * 2);
    std::vector<int> d(S);
    int maxDelay = 0;
    for (int s = 0; s < S; ++s) {
        const MixGains mg = staticMixGains((double)e->procParams[s].mix);
        g[2 * s] = mg.wet;
        g[2 * s + 1] = mg.dry;
        d[s] = procDelayOf(e, s);
        maxDelay = std::max(maxDelay, d[s]);
    }
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    if (!e->procGains) {
        CPQ_TRY(allocAll(e, { { e->procGains, (size_t)2 * S }, { e->procDelay, (size_t)S } }, "processor-level gain buffers could not be allocated"));
    }
    // delay ring: the longest delay in sight (any IR that fits the engine: irPeakLatency < irLen) plus one call; a larger
    // request later grows it, keeping what it holds
    const int64_t need = (int64_t)std::max(maxDelay, e->P0 + e->desc.max_ir_len) + (int64_t)e->tMax * e->P + 1;
    if (need > e->dryRingSize) {
        const int size = nextPow2((int)std::min<int64_t>(need, (int64_t)1 << 30));
        DeviceBuffer<double> ring;
        CPQ_TRY(allocAll(e, { { ring, (size_t)e->nCh * size, true } }, "dry delay line of %d samples per channel could not be allocated", size));
        if (e->dryRing) {
            cpq::launch_ring_regrow(e->stream, e->dryRing, e->dryRingSize, ring, size, e->dryPos, e->nCh);
            CPQ_HIP(e, hipStreamSynchronize(e->stream));
        }
        e->dryRing = std::move(ring);       // frees the old ring
        e->dryRingSize = size;
    }
    if (!e->latNew) {
        CPQ_TRY(allocAll(e, { { e->latNew, (size_t)S }, { e->latOld, (size_t)S }, { e->latLen, (size_t)S } }, "latency buffers could not be allocated"));
    }
    CPQ_HIP(e, hipMemcpy(e->procGains, g.data(), sizeof(double) * g.size(), hipMemcpyHostToDevice));
    CPQ_HIP(e, hipMemcpy(e->procDelay, d.data(), sizeof(int) * d.size(), hipMemcpyHostToDevice));
    return CPQ_OK;
}

// The steps of enqueueConvProc, in its order.

// resting ONE convolver needs that stream in a plan group: refused before any ramp moves
static int checkRestFeasible(cpq_engine* e, const ProcRest& r)
{
    if (!r.anyRest || r.allRest) return CPQ_OK;
    for (int s = 0; s < e->desc.n_streams; ++s)
        if (r.rest[(size_t)s] && e->groupOf[(size_t)s] < 0)
            return fail(e, CPQ_ERR_UNSUPPORTED, "stream %d: a per-stream bypass / dry-only needs the stream on the reference's own "
                        "layer plan (CPQ_CALLS_ANY, CPQ_SCHED_REFERENCE_NUC or a FilterSpec plan with tail layers); on the "
                        "uniform path set it for CPQ_ALL_STREAMS", s);
    return CPQ_OK;
}

static int uploadMixPlan(cpq_engine* e, const ProcMixPlan& m)
{
    if (!m.anyRamp) return CPQ_OK;
    const int S = e->desc.n_streams;
    if (!e->mixRampLen) {
        CPQ_TRY(allocAll(e, { { e->mixRampLen, (size_t)S } }, "mix-ramp buffers could not be allocated"));
    }
    CPQ_TRY(grow(e, e->mixRampGains, e->mixRampCap, m.rampStride, (size_t)2 * S, "mix-ramp buffers could not be allocated"));
    CPQ_TRY(stageUpload(e, e->mixRampLen, m.len.data(), sizeof(int) * S));
    return stageUpload(e, e->mixRampGains, m.gains.data(), sizeof(double) * m.gains.size());
}

// A stream whose convolver rests while others run is moved to a plan group of its own and that group is not processed; the
// device flags say whose output is the delayed dry signal alone.
static int applyRest(cpq_engine* e, const ProcRest& r)
{
    const int S = e->desc.n_streams;
    if (!r.allRest && (r.anyRest || !e->groups.empty()))
        for (int s = 0; s < S; ++s) {
            if (e->groupOf[(size_t)s] < 0) { if (r.rest[(size_t)s]) return setStreamFrozen(e, s, true); continue; }     // reports why not
            CPQ_TRY(setStreamFrozen(e, s, r.rest[(size_t)s] != 0));
        }
    std::vector<int> wetOn((size_t)S);
    for (int s = 0; s < S; ++s) wetOn[(size_t)s] = r.rest[(size_t)s] ? 0 : 1;
    if (wetOn == e->procWetOnHost) return CPQ_OK;
    if (!e->procWetOn)
        CPQ_TRY(allocAll(e, { { e->procWetOn, (size_t)S } }, "processor-level flags could not be allocated"));
    CPQ_TRY(stageUpload(e, e->procWetOn, wetOn.data(), sizeof(int) * S));
    e->procWetOnHost = wetOn;
    return CPQ_OK;
}

// one launch per range of the latency plan; latNewHost / latOldHost: what the device holds
static int launchMixRanges(cpq_engine* e, double* dOut, int n, long long pos0, const ProcLatPlan& lat, const ProcMixPlan& mix, bool skipConv)
{
    const int S = e->desc.n_streams;
    if (lat.anyFade) {
        CPQ_TRY(grow(e, e->latGains, e->latCap, lat.xStride, (size_t)S, "latency cross-fade buffer could not be allocated"));
    }
    for (const ProcLatRange& r : lat.ranges) {
        const int off = r.c0 * e->B, len = std::min(r.c1 * e->B, n) - off;
        if (r.dNew != e->latNewHost) {
            CPQ_TRY(stageUpload(e, e->latNew, r.dNew.data(), sizeof(int) * S));
            e->latNewHost = r.dNew;
        }
        if (r.dOld != e->latOldHost) {
            CPQ_TRY(stageUpload(e, e->latOld, r.dOld.data(), sizeof(int) * S));
            e->latOldHost = r.dOld;
        }
        if (r.fade()) {
            CPQ_TRY(stageUpload(e, e->latLen, r.xLen.data(), sizeof(int) * S));
            CPQ_TRY(stageUpload(e, e->latGains, r.gains.data(), sizeof(double) * r.gains.size()));
        }
        ProfScope p(e, CPQ_K_MIX);
        cpq::launch_convproc_mix(e->stream, dOut + off, dOut + off, (int64_t)n, e->nCh, len, e->procGains, e->dryRing,
                                 e->dryRingSize, pos0 + off, e->latNew, e->latOld, r.fade() ? e->latLen : nullptr, e->latGains,
                                 e->latCap, skipConv ? 0 : 1, mix.anyRamp ? e->mixRampLen : nullptr, e->mixRampGains, mix.rampStride,
                                 off, e->procWetOn);
    }
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

// What a failure leaves behind: the refusal of a per-stream rest moves nothing; the mix ramps have moved, and procProcessed is
// set, before freezing, the ring put or the convolver can fail; the latency fades move only behind a convolver that was enqueued.
int enqueueConvProc(cpq_engine* e, const double* dIn, double* dOut, int n)
{
    if (!e->procGains) CPQ_TRY(uploadProcParams(e));
    const int S = e->desc.n_streams;
    std::vector<double> mixOf((size_t)S);
    std::vector<int> peakOf((size_t)S);
    for (int s = 0; s < S; ++s) {
        mixOf[(size_t)s] = (double)e->procParams[s].mix;
        peakOf[(size_t)s] = (int)e->procParams[s].ir_peak_latency;
    }
    const ProcRest rest = planProcRest(e->mixRamp.data(), e->procBypass.data(), e->procDryOnly.data(), mixOf.data(), S, n, e->B);
    CPQ_TRY(checkRestFeasible(e, rest));
    const ProcMixPlan mix = planProcMix(e->mixRamp.data(), e->procBypass.data(), mixOf.data(), S, n, e->B);
    CPQ_TRY(uploadMixPlan(e, mix));
    const bool firstCall = !e->procProcessed;
    e->procProcessed = true;
    CPQ_TRY(applyRest(e, rest));
    // the call's input goes into the delay ring before the convolver may overwrite it (in-place calls)
    const long long pos0 = e->dryPos;
    {
        ProfScope p(e, CPQ_K_MIX);
        cpq::launch_ring_put(e->stream, dIn, (int64_t)n, n, e->dryRing, e->dryRingSize, pos0, e->nCh);
    }
    e->dryPos += n;
    const bool skipConv = rest.allRest;
    if (!skipConv) {
        e->honourFrozen = true;               // resting streams: their plan groups and direct heads are not run
        const int rc = enqueueConv(e, dIn, dOut, n);
        e->honourFrozen = false;
        if (rc != CPQ_OK) return rc;
    }
    const ProcLatPlan lat = planProcLatency(e->latFade.data(), e->procBypass.data(), peakOf.data(), S, e->directHead, e->P0, firstCall,
                                            n, e->B, LinearRamp::stepsFor(e->sampleRate, 0.02));
    return launchMixRanges(e, dOut, n, pos0, lat, mix, skipConv);
}

}  // namespace cpqi

extern "C" {

int32_t cpq_convproc_set_params(cpq_engine* e, int32_t stream, const cpq_convproc_params* p)
{
    if (!e || !p) return CPQ_ERR_INVALID_ARG;
    int s0 = 0, s1 = 0;
    CPQ_TRY(streamRange(e, stream, s0, s1));
    if (!(p->mix >= 0.0f && p->mix <= 1.0f)) return fail(e, CPQ_ERR_INVALID_ARG, "mix must be in [0, 1]");
    if (p->ir_peak_latency < 0) return fail(e, CPQ_ERR_INVALID_ARG, "ir_peak_latency must be >= 0");
    const bool dryOnly = !((double)p->mix > 0.001);        // needsConvolution, :374
    if (stream != CPQ_ALL_STREAMS && (p->bypassed || dryOnly) && e->groupOf[(size_t)stream] < 0 && e->irLoaded[2 * (size_t)stream])
        return fail(e, CPQ_ERR_UNSUPPORTED, "a per-stream bypass / dry-only rests ONE convolver: the stream must run on the reference's own "
                    "layer plan (CPQ_CALLS_ANY, CPQ_SCHED_REFERENCE_NUC or a FilterSpec plan with tail layers); on the uniform path set it "
                    "for CPQ_ALL_STREAMS");
    if (p->smoothing_time_sec != 0.0f && !(p->smoothing_time_sec >= 0.01f && p->smoothing_time_sec <= 0.5f))
        return fail(e, CPQ_ERR_INVALID_ARG, "smoothing_time_sec must be 0 (default 0.1 s) or in [0.01, 0.5]");
    for (int s = s0; s < s1; ++s) {
        e->procParams[s] = *p;
        LinearRamp& r = e->mixRamp[s].ramp;
        const double t = p->smoothing_time_sec != 0.0f ? (double)p->smoothing_time_sec : 0.1;     // SMOOTHING_TIME_DEFAULT_SEC
        r.totalSteps = LinearRamp::stepsFor(e->sampleRate, t);
        // before the first processor-level call (the reference's prepareToPlay: setCurrentAndTargetValue, Lifecycle.cpp:370)
        // the mix applies at once; afterwards it is the ramp's new target
        if (!e->procProcessed) r.setCurrentAndTargetValue((double)p->mix);
    }
    for (int s = s0; s < s1; ++s) { e->procBypass[s] = p->bypassed != 0; e->procDryOnly[s] = dryOnly; }
    return uploadProcParams(e);
}

int32_t cpq_convproc_delay(const cpq_engine* e, int32_t stream)
{
    if (!e || stream < 0 || stream >= e->desc.n_streams) return CPQ_ERR_INVALID_ARG;
    return procDelayOf(e, stream);
}

int32_t cpq_engine_set_conv_level(cpq_engine* e, int32_t level)
{
    if (!e || (level != CPQ_LEVEL_NUC && level != CPQ_LEVEL_PROCESSOR)) return CPQ_ERR_INVALID_ARG;
    e->convLevel = level;
    if (level == CPQ_LEVEL_NUC) clearFrozen(e);      // resting a stream is processor-level state
    return CPQ_OK;
}

int32_t cpq_convproc_process_device(cpq_engine* e, const double* dIn, double* dOut, int32_t nSamples)
{
    CPQ_TRY(checkCall(e, dIn, dOut, nSamples));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueConvProc(e, dIn, dOut, nSamples);
}

int32_t cpq_convproc_process(cpq_engine* e, const double* in, double* out, int32_t nSamples)
{
    return viaStaging(e, in, out, nSamples, [e](const double* a, double* b, int n) { return enqueueConvProc(e, a, b, n); });
}

}  // extern "C"
