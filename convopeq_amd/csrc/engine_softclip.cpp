// engine_softclip.cpp -- DSPCore's soft clipper (DSPCoreDouble.cpp:471-503), between the output make-up gain and the
// oversampler's down stages.  The kernel is softclip_kernels.hip, the arithmetic and the table row softclip_design.hpp's.
//   factor > 1   one launch in place on the oversampled block, callbacks of block_size samples (enqueueOsChain, engine_os.cpp)
//   factor 1     softClipOS, a CustomInputOversampler of one 31-tap / 90 dB stage (DSPCoreLifecycle.cpp:188): processUp, the
//                clipper on 2 n samples in callbacks of 2 block_size, processDown back into the rows; before the output stage
//                (meteredChain, engine_core.cpp).  The stage is the design of the main oversampler's third IIR-like stage and runs
//                through the same kernels as a second instance (OsView) with histories, flags and counters of its own: the same
//                guards, the same auto-clear / hard-fallback prologue, the same 3/4 gain of an up / down pair, 15 base-rate
//                samples of latency.
// Every stream has its own amount and may rest: its table row is flagged off and, at factor 1, the local pair runs over the
// runs of neighbouring streams that clip, so a resting stream's rows are not touched.  While no stream clips nothing is
// launched and nothing is allocated.
#include "engine_internal.hpp"

namespace cpqi {

namespace {

constexpr const char* kOffText = "the soft clipper is off (cpq_engine_set_soft_clip)";

OsView localView(cpq_engine* e, int s0, int s1)
{
    return OsView{ &e->scStage, 1, e->scFlags, e->scCounts, e->scNonSilent, 2 * s0, 2 * (s1 - s0) };
}

// fn(s0, s1) for every maximal run [s0, s1) of streams that clip
template <typename F>
int forClippingRuns(cpq_engine* e, F&& fn)
{
    const int S = e->desc.n_streams;
    for (int s = 0; s < S;) {
        if (!e->scOnHost[s]) { ++s; continue; }
        int t = s;
        while (t < S && e->scOnHost[t]) ++t;
        CPQ_TRY(fn(s, t));
        s = t;
    }
    return CPQ_OK;
}

// rows [nCh][n] at the processing rate: null handle (no message), clipper off, null buffer, n outside 1..maxCall, a callback
// length below 1, 16-byte alignment
int checkRows(cpq_engine* e, const void* in, const void* out, int n, int cb)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!e->anySoftClip) return fail(e, CPQ_ERR_NOT_READY, "%s", kOffText);
    if (!in || !out) return fail(e, CPQ_ERR_INVALID_ARG, "null buffer");
    if (n <= 0 || n > e->maxCall) return fail(e, CPQ_ERR_INVALID_ARG, "n_samples=%d outside 1..%d", n, e->maxCall);
    if (cb <= 0) return fail(e, CPQ_ERR_INVALID_ARG, "callback_len=%d is not positive", cb);
    if ((reinterpret_cast<uintptr_t>(in) & 15u) || (reinterpret_cast<uintptr_t>(out) & 15u))
        return fail(e, CPQ_ERR_INVALID_ARG, "buffers must be 16-byte aligned");
    return CPQ_OK;
}

int enqueueAlone(cpq_engine* e, const double* in, double* out, int n, int cb)
{
    if (in != out) cpq::launch_rows_copy(e->stream, in, n, 0, out, n, 0, n, e->nCh);
    return enqueueSoftClipRows(e, out, n, n, cb);
}

}  // namespace

int enqueueSoftClipRows(cpq_engine* e, double* rows, int64_t stride, int n, int cb)
{
    if (!e->anySoftClip) return CPQ_OK;
    ProfScope p(e, CPQ_K_SOFTCLIP);
    cpq::launch_soft_clip(e->stream, rows, stride, n, cb, e->nCh, e->scTab);
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

int ensureSoftClipStage(cpq_engine* e)
{
    const size_t S = (size_t)e->desc.n_streams, nCh = (size_t)e->nCh;
    if (!e->scCoef) {
        cpq::OsStage st;
        cpq::osDesignStage(2, CPQ_OS_IIR, st);          // tapsForStage / attenuationForStage of stage 2: 31 taps, 90 dB
        if (st.taps != 31 || !cpq::os_conv_count_supported(st.convCount) || st.convParity != 0 || st.historyUpKeep < st.convCount - 1 ||
            st.historyDownKeep < 2 * (st.convCount - 1) || st.historyDownKeep < st.centerTap)
            return fail(e, CPQ_ERR_UNSUPPORTED, "the soft clipper's 2x stage has a geometry the kernels do not support");
        const size_t up = nCh * (size_t)st.historyUpKeep, down = nCh * (size_t)st.historyDownKeep;
        CPQ_HIP(e, hipStreamSynchronize(e->stream));
        CPQ_TRY(allocAll(e, { { e->scCoef, (size_t)st.convCount }, { e->scUp[0], up, true }, { e->scUp[1], up, true },
                              { e->scDown[0], down, true }, { e->scDown[1], down, true }, { e->scFlags, 4 * S, true },
                              { e->scCounts, 2 * S, true }, { e->scNonSilent, nCh, true } },
                         "the soft clipper's 2x stage could not be allocated"));
        CPQ_HIP(e, hipMemcpy(e->scCoef, st.conv.data(), sizeof(double) * (size_t)st.convCount, hipMemcpyHostToDevice));
        auto& d = e->scStage;
        d = cpq_engine::OsStageDev{};
        d.convCount = st.convCount;
        d.upKeep = st.historyUpKeep;
        d.downKeep = st.historyDownKeep;
        d.centerTap = st.centerTap;
        d.centerDelay = st.centerDelayInput;
        d.centerCoeff = st.centerCoeff;
        d.coef = e->scCoef;
        for (int b = 0; b < 2; ++b) { d.up[b] = e->scUp[b]; d.down[b] = e->scDown[b]; }
    }
    if (!e->scWork) {
        const size_t count = nCh * 2 * (size_t)e->maxCall;
        CPQ_TRY(allocAll(e, { { e->scWork, count } }, "the soft clipper's 2x block of %zu bytes could not be allocated", count * sizeof(double)));
    }
    return CPQ_OK;
}

int resetSoftClipStage(cpq_engine* e)
{
    if (!e->scCoef) return CPQ_OK;
    auto& s = e->scStage;
    CPQ_HIP(e, hipSetDevice(e->device));
    for (int b = 0; b < 2; ++b) {
        CPQ_HIP(e, hipMemsetAsync(s.up[b], 0, sizeof(double) * (size_t)e->nCh * s.upKeep, e->stream));
        CPQ_HIP(e, hipMemsetAsync(s.down[b], 0, sizeof(double) * (size_t)e->nCh * s.downKeep, e->stream));
    }
    s.upSel = s.downSel = 0;
    CPQ_HIP(e, hipMemsetAsync(e->scFlags, 0, sizeof(int) * 4 * (size_t)e->desc.n_streams, e->stream));
    return CPQ_OK;
}

int enqueueSoftClipLocal(cpq_engine* e, double* rows, int n)
{
    const int64_t n2 = 2 * (int64_t)n;
    CPQ_TRY(forClippingRuns(e, [&](int s0, int s1) { return enqueueOsUp(e, localView(e, s0, s1), rows, n, e->scWork, n2, n); }));
    flipOsUp(localView(e, 0, 0));
    CPQ_TRY(enqueueSoftClipRows(e, e->scWork, n2, 2 * n, 2 * e->B));
    CPQ_TRY(forClippingRuns(e, [&](int s0, int s1) { return enqueueOsDown(e, localView(e, s0, s1), e->scWork, n2, rows, n, n); }));
    flipOsDown(localView(e, 0, 0));
    return CPQ_OK;
}

}  // namespace cpqi

using namespace cpqi;

extern "C" {

int32_t cpq_engine_set_soft_clip(cpq_engine* e, int32_t stream, int32_t enabled, float saturationAmount)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    int s0 = 0, s1 = 0;
    CPQ_TRY(streamRange(e, stream, s0, s1));
    if (!cpq::softClipAmountValid(saturationAmount))
        return fail(e, CPQ_ERR_INVALID_ARG, "saturation amount %g is not in 0..1", (double)saturationAmount);
    const int S = e->desc.n_streams;
    const char on = enabled != 0;
    bool onChanged = false;
    for (int s = s0; s < s1; ++s) onChanged = onChanged || e->scOnHost[s] != on;
    if (!on && !e->scTab) {         // nothing clips and nothing ever did: the amount is kept for a later call, nothing is allocated
        for (int s = s0; s < s1; ++s) e->scAmountHost[s] = saturationAmount;
        return CPQ_OK;
    }
    CPQ_HIP(e, hipSetDevice(e->device));
    if (!e->scTab)
        CPQ_TRY(allocAll(e, { { e->scTab, (size_t)S * cpq::kSoftClipTabDoubles } }, "the soft clipper's table could not be allocated"));
    for (int s = s0; s < s1; ++s) { e->scOnHost[s] = on; e->scAmountHost[s] = saturationAmount; }
    std::vector<double> tab((size_t)S * cpq::kSoftClipTabDoubles);
    e->anySoftClip = false;
    for (int s = 0; s < S; ++s) {
        cpq::softClipTableRow(e->scOnHost[s] != 0, e->scAmountHost[s], &tab[(size_t)s * cpq::kSoftClipTabDoubles]);
        e->anySoftClip = e->anySoftClip || e->scOnHost[s];
    }
    CPQ_HIP(e, hipStreamSynchronize(e->stream));        // nothing in flight reads the table
    CPQ_HIP(e, hipMemcpy(e->scTab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    if (onChanged) {                                    // a stream that starts or stops clipping: the local stage starts clear
        CPQ_TRY(resetSoftClipStage(e));
        CPQ_HIP(e, hipStreamSynchronize(e->stream));
    }
    return CPQ_OK;
}

int32_t cpq_soft_clip_reset(cpq_engine* e)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!e->anySoftClip) return fail(e, CPQ_ERR_NOT_READY, "%s", kOffText);
    CPQ_TRY(resetSoftClipStage(e));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

int32_t cpq_soft_clip_process_device(cpq_engine* e, const double* dIn, double* dOut, int32_t nSamples, int32_t callbackLen)
{
    CPQ_TRY(checkRows(e, dIn, dOut, nSamples, callbackLen));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueAlone(e, dIn, dOut, nSamples, callbackLen);
}

int32_t cpq_soft_clip_process(cpq_engine* e, const double* in, double* out, int32_t nSamples, int32_t callbackLen)
{
    CPQ_TRY(checkRows(e, in, out, nSamples, callbackLen));
    return hostRoundTrip(e, in, (size_t)nSamples, out, (size_t)nSamples, true,
                         [&](const double* a, double* b) { return enqueueAlone(e, a, b, nSamples, callbackLen); });
}

int32_t cpq_soft_clip_read_telemetry(cpq_engine* e, int32_t stream, cpq_os_telemetry* out)
{
    if (!e || !out) return CPQ_ERR_INVALID_ARG;
    if (stream < 0 || stream >= e->desc.n_streams) return fail(e, CPQ_ERR_INVALID_ARG, "stream %d out of range", stream);
    *out = cpq_os_telemetry{};
    if (!e->scFlags) return CPQ_OK;
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    unsigned long long c[2];
    int f[4];
    CPQ_HIP(e, hipMemcpy(c, e->scCounts + 2 * stream, sizeof(c), hipMemcpyDeviceToHost));
    CPQ_HIP(e, hipMemcpy(f, e->scFlags + 4 * stream, sizeof(f), hipMemcpyDeviceToHost));
    out->corruption_events = c[0];
    out->auto_clears = c[1];
    out->corruption_pending = f[0];
    out->consecutive_auto_clears = f[1];
    out->hard_fallback = f[2];
    return CPQ_OK;
}

}  // extern "C"
