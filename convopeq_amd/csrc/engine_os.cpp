// engine_os.cpp -- the half-band oversampler around the routing (CustomInputOversampler, src/CustomInputOversampler.cpp, as
// DSPCore::processDouble runs it: processUp, the chain at F x the rate, processDown; DSPCoreDouble.cpp:359-376, :477-531).
// The stage kernels, guards and per-stream state machine are in os_kernels.hip; the host sizes the buffers, uploads the
// coefficients and flips the history ping-pong selectors.  cpq_os_up / cpq_os_down take the refusals of checkBaseRows (any
// call length) and the two-buffer hostRoundTrip; a new factor ends in refreshBaseRateStages (all three: engine_core.cpp).
// enqueueOsUp / enqueueOsDown take the instance they drive as an OsView: the engine's own stages, or the single 31-tap stage of
// the soft clipper's local 2x pair (engine_softclip.cpp), over all of its channels or a run of them.
#include "engine_internal.hpp"

namespace cpqi {

void freeOversampler(cpq_engine* e)
{
    e->osMem.reset();
    for (auto& s : e->osStage) s = cpq_engine::OsStageDev{};
    e->osStages = 0;
}

int resetOversampler(cpq_engine* e)
{
    if (!e->osFlags) return CPQ_OK;
    CPQ_HIP(e, hipSetDevice(e->device));
    for (int i = 0; i < e->osStages; ++i) {
        auto& s = e->osStage[i];
        for (int b = 0; b < 2; ++b) {
            CPQ_HIP(e, hipMemsetAsync(s.up[b], 0, sizeof(double) * (size_t)e->nCh * s.upKeep, e->stream));
            CPQ_HIP(e, hipMemsetAsync(s.down[b], 0, sizeof(double) * (size_t)e->nCh * s.downKeep, e->stream));
        }
        s.upSel = s.downSel = 0;
    }
    CPQ_HIP(e, hipMemsetAsync(e->osFlags, 0, sizeof(int) * 4 * (size_t)e->desc.n_streams, e->stream));
    return CPQ_OK;
}

static int ensureOsTmp(cpq_engine* e)
{
    for (auto& b : e->osTmp) {
        if (b) continue;
        const size_t count = (size_t)e->nCh * (size_t)(e->maxCall / 2);
        CPQ_TRY(allocAll(e, { { b, count } }, "oversampler stage buffer of %zu bytes could not be allocated", count * sizeof(double)));
    }
    return CPQ_OK;
}

static cpq::OsStageArgs stageArgs(const OsView& v, int i)
{
    const auto& s = v.stage[i];
    cpq::OsStageArgs a{};
    a.coef = s.coef;
    a.convCount = s.convCount;
    a.centerCoeff = s.centerCoeff;
    a.nCh = v.nCh;
    a.flags = v.flags + 4 * (v.ch0 / 2);
    a.counts = v.counts + 2 * (v.ch0 / 2);
    return a;
}

static OsView mainView(cpq_engine* e)
{
    return OsView{ e->osStage, e->osStages, e->osFlags, e->osCounts, e->osNonSilent, 0, e->nCh };
}

void flipOsUp(const OsView& v) { for (int i = 0; i < v.nStages; ++i) v.stage[i].upSel ^= 1; }
void flipOsDown(const OsView& v) { for (int i = 0; i < v.nStages; ++i) v.stage[i].downSel ^= 1; }

// processUp: in [nCh][inStride] (nBase samples) -> out [nCh][outStride] (nBase * F samples)
int enqueueOsUp(cpq_engine* e, const OsView& v, const double* in, int64_t inStride, double* out, int64_t outStride, int nBase)
{
    if (v.nStages > 1) CPQ_TRY(ensureOsTmp(e));
    ProfScope p(e, CPQ_K_OS);
    const double* src = in + v.ch0 * inStride;
    int64_t srcStride = inStride;
    int n = nBase;
    for (int i = 0; i < v.nStages; ++i) {
        const auto& s = v.stage[i];
        const bool last = i == v.nStages - 1;
        double* dst = last ? out + v.ch0 * outStride : e->osTmp[i & 1];
        const int64_t dstStride = last ? outStride : 2 * (int64_t)n;
        cpq::OsStageArgs a = stageArgs(v, i);
        a.in = src; a.inStride = srcStride; a.out = dst; a.outStride = dstStride;
        a.histOld = s.up[s.upSel] + (int64_t)v.ch0 * s.upKeep; a.histNew = s.up[s.upSel ^ 1] + (int64_t)v.ch0 * s.upKeep; a.keep = s.upKeep;
        a.centerOffset = s.centerDelay;
        a.n = n;
        cpq::launch_os_interp(e->stream, a);
        src = dst; srcStride = dstStride; n *= 2;
    }
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

// processDown: in [nCh][inStride] (nBase * F samples) -> out [nCh][outStride] (nBase samples)
int enqueueOsDown(cpq_engine* e, const OsView& v, const double* in, int64_t inStride, double* out, int64_t outStride, int nBase)
{
    if (v.nStages > 1) CPQ_TRY(ensureOsTmp(e));
    ProfScope p(e, CPQ_K_OS);
    cpq::OsHistories hs{};
    for (int i = 0; i < v.nStages; ++i) {
        const auto& s = v.stage[i];
        hs.up[i] = s.up[s.upSel] + (int64_t)v.ch0 * s.upKeep;
        hs.down[i] = s.down[s.downSel] + (int64_t)v.ch0 * s.downKeep;
        hs.upKeep[i] = s.upKeep;
        hs.downKeep[i] = s.downKeep;
    }
    int* nonSilent = v.nonSilent + v.ch0;
    cpq::launch_os_down_state(e->stream, hs, v.nStages, v.nCh / 2, v.flags + 4 * (v.ch0 / 2), v.counts + 2 * (v.ch0 / 2), nonSilent);
    const int top = v.nStages - 1;
    int n = nBase << top;                                   // outputs of the top stage
    const double* src = in + v.ch0 * inStride;
    cpq::launch_os_scan(e->stream, src, inStride, 2 * n, v.nCh, nonSilent + (size_t)top * v.nCh);
    int64_t srcStride = inStride;
    for (int i = top; i >= 0; --i) {
        const auto& s = v.stage[i];
        double* dst = i == 0 ? out + v.ch0 * outStride : e->osTmp[i & 1];
        const int64_t dstStride = i == 0 ? outStride : (int64_t)n;
        cpq::OsStageArgs a = stageArgs(v, i);
        a.in = src; a.inStride = srcStride; a.out = dst; a.outStride = dstStride;
        a.histOld = s.down[s.downSel] + (int64_t)v.ch0 * s.downKeep; a.histNew = s.down[s.downSel ^ 1] + (int64_t)v.ch0 * s.downKeep; a.keep = s.downKeep;
        a.centerOffset = s.centerTap;
        a.n = n;
        cpq::launch_os_decim(e->stream, a, nonSilent + (size_t)i * v.nCh,
                             i > 0 ? nonSilent + (size_t)(i - 1) * v.nCh : nullptr);
        src = dst; srcStride = dstStride; n /= 2;
    }
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

// the engine's own instance: one call of each direction, then the histories it wrote become the current ones
static int enqueueUp(cpq_engine* e, const double* in, int64_t inStride, double* out, int64_t outStride, int nBase)
{
    const OsView v = mainView(e);
    const int rc = enqueueOsUp(e, v, in, inStride, out, outStride, nBase);
    if (rc == CPQ_OK) flipOsUp(v);
    return rc;
}

static int enqueueDown(cpq_engine* e, const double* in, int64_t inStride, double* out, int64_t outStride, int nBase)
{
    const OsView v = mainView(e);
    const int rc = enqueueOsDown(e, v, in, inStride, out, outStride, nBase);
    if (rc == CPQ_OK) flipOsDown(v);
    return rc;
}

// whole path with factor > 1: up -> routing on nBase * F samples in the internal work buffer (in place) -> down
int enqueueOsChain(cpq_engine* e, const double* dIn, double* dOut, int nBase)
{
    CPQ_TRY(ensureCallBuffer(e, e->osWork, "oversampled block"));
    const int n = nBase * e->osFactor;
    CPQ_TRY(enqueueUp(e, dIn, nBase, e->osWork, n, nBase));
    CPQ_TRY(enqueueBoth(e, e->osWork, e->osWork, n));
    CPQ_TRY(enqueueSoftClipRows(e, e->osWork, n, n, e->B));     // after the make-up gain, before processDown (:479-488)
    return enqueueDown(e, e->osWork, n, dOut, nBase, nBase);
}

}  // namespace cpqi

using namespace cpqi;

// the stand-alone entry points: nBase * F within the engine's call limit, 16-byte aligned buffers; any call length
static int checkOsCall(cpq_engine* e, const void* in, const void* out, int nBase)
{
    return checkBaseRows(e, in, out, nBase, e && e->osFactor > 1, "oversampling is not set (factor 1)", false);
}

extern "C" {

int32_t cpq_engine_set_oversampling(cpq_engine* e, int32_t factor, int32_t type)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    const int nStages = cpq::osStagesFor(factor);
    if (nStages < 0) return fail(e, CPQ_ERR_INVALID_ARG, "oversampling factor %d is not 1, 2, 4 or 8", factor);
    if (type != CPQ_OS_IIR && type != CPQ_OS_LINEAR_PHASE) return fail(e, CPQ_ERR_INVALID_ARG, "oversampling type %d", type);
    if (factor > 1 && e->anyCalls && e->B % factor != 0)
        return fail(e, CPQ_ERR_INVALID_ARG, "block_size %d is not a multiple of the oversampling factor %d", e->B, factor);
    if (factor > 1 && e->sampleRate > 768000.0)
        return fail(e, CPQ_ERR_INVALID_ARG, "processing rate %.1f Hz above 768 kHz (OversamplingPolicy::kMaxInternalRate)", e->sampleRate);
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    freeOversampler(e);
    CPQ_TRY(resetSoftClipStage(e));     // DSPCore::prepare designs softClipOS again: its histories and flags start clear
    const int S = e->desc.n_streams;
    if (!e->osFlags) {
        CPQ_TRY(allocAll(e, { { e->osFlags, (size_t)4 * S }, { e->osCounts, (size_t)2 * S }, { e->osNonSilent, (size_t)3 * e->nCh } },
                         "oversampler state could not be allocated"));
    }
    CPQ_HIP(e, hipMemset(e->osCounts, 0, sizeof(unsigned long long) * 2 * S));
    CPQ_HIP(e, hipMemset(e->osFlags, 0, sizeof(int) * 4 * S));
    e->osFactor = factor;
    e->osType = type;
    if (nStages == 0) return refreshBaseRateStages(e);
    cpq::OsStage st[3];
    size_t bytes = 0;
    for (int i = 0; i < nStages; ++i) {
        cpq::osDesignStage(i, type, st[i]);
        if (!cpq::os_conv_count_supported(st[i].convCount) || st[i].convParity != 0 || st[i].historyUpKeep < st[i].convCount - 1 ||
            st[i].historyDownKeep < 2 * (st[i].convCount - 1) || st[i].historyDownKeep < st[i].centerTap) {
            e->osFactor = 1;
            return fail(e, CPQ_ERR_UNSUPPORTED, "stage %d geometry not supported by the kernels", i);
        }
        bytes += (size_t)alignUp(st[i].convCount, 32) + 2 * (size_t)e->nCh * (alignUp(st[i].historyUpKeep, 32) + alignUp(st[i].historyDownKeep, 32));
    }
    if (!e->osMem.alloc(bytes * sizeof(double))) {
        e->osFactor = 1;
        return fail(e, CPQ_ERR_OOM, "oversampler histories of %zu bytes could not be allocated", bytes * sizeof(double));
    }
    double* p = reinterpret_cast<double*>(e->osMem.get());
    for (int i = 0; i < nStages; ++i) {
        auto& d = e->osStage[i];
        d.convCount = st[i].convCount;
        d.upKeep = st[i].historyUpKeep;
        d.downKeep = st[i].historyDownKeep;
        d.centerTap = st[i].centerTap;
        d.centerDelay = st[i].centerDelayInput;
        d.centerCoeff = st[i].centerCoeff;
        d.coef = p; p += alignUp(d.convCount, 32);
        CPQ_HIP(e, hipMemcpy(d.coef, st[i].conv.data(), sizeof(double) * d.convCount, hipMemcpyHostToDevice));
        for (int b = 0; b < 2; ++b) { d.up[b] = p; p += (size_t)e->nCh * alignUp(d.upKeep, 32); }
        for (int b = 0; b < 2; ++b) { d.down[b] = p; p += (size_t)e->nCh * alignUp(d.downKeep, 32); }
    }
    e->osStages = nStages;
    CPQ_TRY(resetOversampler(e));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return refreshBaseRateStages(e);
}

int32_t cpq_os_up_device(cpq_engine* e, const double* dIn, double* dOut, int32_t nBase)
{
    CPQ_TRY(checkOsCall(e, dIn, dOut, nBase));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueUp(e, dIn, nBase, dOut, (int64_t)nBase * e->osFactor, nBase);
}

int32_t cpq_os_down_device(cpq_engine* e, const double* dIn, double* dOut, int32_t nBase)
{
    CPQ_TRY(checkOsCall(e, dIn, dOut, nBase));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueDown(e, dIn, (int64_t)nBase * e->osFactor, dOut, nBase, nBase);
}

int32_t cpq_os_up(cpq_engine* e, const double* in, double* out, int32_t nBase)
{
    CPQ_TRY(checkOsCall(e, in, out, nBase));
    const size_t nOut = (size_t)nBase * e->osFactor;
    return hostRoundTrip(e, in, (size_t)nBase, out, nOut, false,
                         [&](const double* a, double* b) { return enqueueUp(e, a, nBase, b, (int64_t)nOut, nBase); });
}

int32_t cpq_os_down(cpq_engine* e, const double* in, double* out, int32_t nBase)
{
    CPQ_TRY(checkOsCall(e, in, out, nBase));
    const size_t nIn = (size_t)nBase * e->osFactor;
    return hostRoundTrip(e, in, nIn, out, (size_t)nBase, false,
                         [&](const double* a, double* b) { return enqueueDown(e, a, (int64_t)nIn, b, nBase, nBase); });
}

int32_t cpq_os_reset(cpq_engine* e)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(resetOversampler(e));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

int32_t cpq_os_read_telemetry(cpq_engine* e, int32_t stream, cpq_os_telemetry* out)
{
    if (!e || !out) return CPQ_ERR_INVALID_ARG;
    if (stream < 0 || stream >= e->desc.n_streams) return fail(e, CPQ_ERR_INVALID_ARG, "stream %d out of range", stream);
    *out = cpq_os_telemetry{};
    if (!e->osFlags) return CPQ_OK;
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    unsigned long long c[2];
    int f[4];
    CPQ_HIP(e, hipMemcpy(c, e->osCounts + 2 * stream, sizeof(c), hipMemcpyDeviceToHost));
    CPQ_HIP(e, hipMemcpy(f, e->osFlags + 4 * stream, sizeof(f), hipMemcpyDeviceToHost));
    out->corruption_events = c[0];
    out->auto_clears = c[1];
    out->corruption_pending = f[0];
    out->consecutive_auto_clears = f[1];
    out->hard_fallback = f[2];
    return CPQ_OK;
}

}  // extern "C"
