// engine_meter.cpp -- loudness and true-peak metering of the base-rate output rows (LoudnessMeter, src/LoudnessMeter.{h,cpp};
// TruePeakDetector, src/TruePeakDetector.{h,cpp}; run at the end of DSPCore::processOutputDouble, DSPCoreDouble.cpp:695-701).
// The kernels are in meter_kernels.hip; the host designs the filters for the base rate, owns the buffers and keeps the ring's
// counters: every stream sees the same callbacks, so one write / read pair and one block counter serve all of them.
// cpq_meter_process takes the refusals of checkBaseRows, then true peak's own (checkMeterCall), and the hostRoundTrip that
// brings nothing back.
#include "engine_internal.hpp"

namespace cpqi {

namespace {

constexpr size_t kTabDoubles = 2 * (size_t)cpq::kMeterSectionDoubles + 32 + 16;

int resetMeters(cpq_engine* e)
{
    if (!e->meterTab) return CPQ_OK;
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipMemsetAsync(e->meterState, 0, sizeof(double) * 8 * (size_t)e->nCh, e->stream));
    for (auto& h : e->meterHist) CPQ_HIP(e, hipMemsetAsync(h, 0, sizeof(double) * 32 * (size_t)e->nCh, e->stream));
    CPQ_HIP(e, hipMemsetAsync(e->meterHold, 0, sizeof(double) * (size_t)e->desc.n_streams, e->stream));
    e->meterHistSel = 0;
    e->meterWrite = e->meterRead = e->meterIndex = e->meterDropped = 0;
    return CPQ_OK;
}

int designMeters(cpq_engine* e)
{
    std::vector<double> tab(kTabDoubles, 0.0);
    double pre[5], rlb[5];
    cpq::meterKWeighting(baseRate(e), pre, rlb);
    cpq::meterSectionTables(pre, tab.data());
    cpq::meterSectionTables(rlb, tab.data() + cpq::kMeterSectionDoubles);
    cpq::OsStage s0, s1;
    cpq::meterTpDesignStage(0, s0);
    cpq::meterTpDesignStage(1, s1);
    if (s0.convCount != 32 || s1.convCount != 16 || s0.convParity != 0 || s1.convParity != 0 || s0.centerDelayInput != 15 ||
        s1.centerDelayInput != 7 || s0.centerCoeff != 0.5 || s1.centerCoeff != 0.5)
        return fail(e, CPQ_ERR_UNSUPPORTED, "true-peak stage geometry not supported by the kernel");
    std::copy(s0.conv.begin(), s0.conv.end(), tab.begin() + 2 * cpq::kMeterSectionDoubles);
    std::copy(s1.conv.begin(), s1.conv.end(), tab.begin() + 2 * cpq::kMeterSectionDoubles + 32);
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    CPQ_HIP(e, hipMemcpy(e->meterTab, tab.data(), sizeof(double) * kTabDoubles, hipMemcpyHostToDevice));
    return CPQ_OK;
}

int checkRows(cpq_engine* e, const void* in, int n)
{
    CPQ_TRY(checkBaseRows(e, in, in, n, e && e->meterFlags, "metering is off (cpq_engine_set_metering)", true));
    return checkMeterCall(e, n);
}

}  // namespace

int refreshMeters(cpq_engine* e)
{
    if (!e->meterFlags) return CPQ_OK;
    CPQ_TRY(designMeters(e));
    CPQ_TRY(resetMeters(e));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

int checkMeterCall(cpq_engine* e, int nBase)
{
    if (!(e->meterFlags & CPQ_METER_TRUE_PEAK)) return CPQ_OK;
    const int cb = callbackLen(e);
    if (cb < 8) return fail(e, CPQ_ERR_UNSUPPORTED, "true-peak metering needs callbacks of at least 8 samples, not %d", cb);
    // with callbacks of varying length the reference's history shift reads stale memory: not reproduced
    if (nBase % cb != 0)
        return fail(e, CPQ_ERR_UNSUPPORTED, "true-peak metering needs whole callbacks: n_samples=%d is not a multiple of %d", nBase, cb);
    return CPQ_OK;
}

// after everything that writes the call's rows, on the engine's stream
int enqueueMeters(cpq_engine* e, const double* rows, int64_t stride, int n)
{
    const int cb = callbackLen(e), nCb = (n + cb - 1) / cb, S = e->desc.n_streams;
    if (nCb > e->meterCbCap) return fail(e, CPQ_ERR_INVALID_ARG, "%d callbacks in one call exceed the meters' %d", nCb, e->meterCbCap);
    ProfScope p(e, CPQ_K_METER);
    double* tab = e->meterTab;
    if (e->meterFlags & CPQ_METER_LOUDNESS)
        cpq::launch_meter_kweight(e->stream, rows, stride, n, cb, e->nCh, tab, e->meterState, e->meterChSum, e->meterChPeak, e->meterCbCap);
    if (e->meterFlags & CPQ_METER_TRUE_PEAK) {
        CPQ_HIP(e, hipMemsetAsync(e->meterTp, 0, sizeof(unsigned long long) * (size_t)S * e->meterCbCap, e->stream));
        cpq::launch_meter_true_peak(e->stream, rows, stride, n, cb, e->nCh, e->meterHist[e->meterHistSel], e->meterHist[e->meterHistSel ^ 1],
                                    tab + 2 * cpq::kMeterSectionDoubles, tab + 2 * cpq::kMeterSectionDoubles + 32, e->meterTp, e->meterCbCap);
        e->meterHistSel ^= 1;
    }
    // LockFreeRingBuffer::push: a record that finds 4096 stored is dropped; blockCounter++ runs either way
    const unsigned long long room = (unsigned long long)kMeterRing - (e->meterWrite - e->meterRead);
    const int nStore = (int)std::min<unsigned long long>(room, (unsigned long long)nCb);
    cpq::MeterFinishArgs a{};
    a.flags = e->meterFlags;
    a.n = n; a.cb = cb; a.nCb = nCb; a.nStore = nStore;
    a.cbCap = e->meterCbCap; a.ringSize = kMeterRing;
    a.write0 = e->meterWrite; a.index0 = e->meterIndex;
    a.chSum = e->meterChSum; a.chPeak = e->meterChPeak; a.tp = e->meterTp;
    a.hold = e->meterHold; a.ring = e->meterRing;
    cpq::launch_meter_finish(e->stream, a, S);
    e->meterWrite += (unsigned long long)nStore;
    e->meterIndex += (unsigned long long)nCb;
    e->meterDropped += (unsigned long long)(nCb - nStore);
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

}  // namespace cpqi

using namespace cpqi;

extern "C" {

int32_t cpq_engine_set_metering(cpq_engine* e, int32_t flags)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (flags & ~(CPQ_METER_LOUDNESS | CPQ_METER_TRUE_PEAK)) return fail(e, CPQ_ERR_INVALID_ARG, "metering flags %d", flags);
    if ((flags & CPQ_METER_TRUE_PEAK) && callbackLen(e) < 8)
        return fail(e, CPQ_ERR_UNSUPPORTED, "true-peak metering needs callbacks of at least 8 samples, not %d", callbackLen(e));
    if (flags == e->meterFlags) return CPQ_OK;
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    if (flags && !e->meterTab) {
        const size_t S = (size_t)e->desc.n_streams, nCh = (size_t)e->nCh;
        const int cbCap = (e->maxCall + e->B - 1) / e->B;          // callbacks of the longest call, at any factor
        CPQ_TRY(allocAll(e, { { e->meterTab, kTabDoubles }, { e->meterState, 8 * nCh }, { e->meterHist[0], 32 * nCh },
                              { e->meterHist[1], 32 * nCh }, { e->meterHold, S }, { e->meterChSum, nCh * cbCap },
                              { e->meterChPeak, nCh * cbCap }, { e->meterTp, S * cbCap }, { e->meterRing, S * kMeterRing } },
                         "meter buffers could not be allocated"));
        e->meterCbCap = cbCap;
    }
    e->meterFlags = flags;
    return refreshMeters(e);
}

int32_t cpq_meter_reset(cpq_engine* e)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!e->meterFlags) return fail(e, CPQ_ERR_NOT_READY, "metering is off (cpq_engine_set_metering)");
    CPQ_TRY(resetMeters(e));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

int32_t cpq_meter_process_device(cpq_engine* e, const double* dIn, int32_t nSamples)
{
    CPQ_TRY(checkRows(e, dIn, nSamples));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueMeters(e, dIn, nSamples, nSamples);
}

int32_t cpq_meter_process(cpq_engine* e, const double* in, int32_t nSamples)
{
    CPQ_TRY(checkRows(e, in, nSamples));
    return hostRoundTrip(e, in, (size_t)nSamples, nullptr, 0, true,
                         [&](const double* a, double*) { return enqueueMeters(e, a, nSamples, nSamples); });
}

int32_t cpq_meter_read_blocks(cpq_engine* e, cpq_meter_block* out, int32_t maxBlocks, int32_t* nBlocks, int64_t* nDropped)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!e->meterFlags) return fail(e, CPQ_ERR_NOT_READY, "metering is off (cpq_engine_set_metering)");
    if (maxBlocks < 0 || (maxBlocks > 0 && !out)) return fail(e, CPQ_ERR_INVALID_ARG, "bad record buffer");
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    const int cnt = (int)std::min<unsigned long long>(e->meterWrite - e->meterRead, (unsigned long long)maxBlocks);
    if (cnt > 0) {
        const int first = (int)(e->meterRead % kMeterRing), head = std::min(cnt, kMeterRing - first);
        const size_t rec = sizeof(cpq_meter_block);
        const cpq_meter_block* ring = e->meterRing;
        CPQ_HIP(e, hipMemcpy2D(out, (size_t)maxBlocks * rec, ring + first, (size_t)kMeterRing * rec, (size_t)head * rec,
                               (size_t)e->desc.n_streams, hipMemcpyDeviceToHost));
        if (cnt > head)
            CPQ_HIP(e, hipMemcpy2D(out + head, (size_t)maxBlocks * rec, ring, (size_t)kMeterRing * rec, (size_t)(cnt - head) * rec,
                                   (size_t)e->desc.n_streams, hipMemcpyDeviceToHost));
        e->meterRead += (unsigned long long)cnt;
    }
    if (nBlocks) *nBlocks = cnt;
    if (nDropped) *nDropped = (int64_t)e->meterDropped;
    e->meterDropped = 0;
    return CPQ_OK;
}

}  // extern "C"
