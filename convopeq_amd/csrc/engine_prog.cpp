// engine_prog.cpp -- cpq_loudness: gated programme loudness (EBU R 128) per stream, an object of its own beside cpq_engine.  The
// definition and the plan of a call are prog_plan.hpp's, the kernels prog_kernels.hip's: this file checks, allocates, launches and
// copies, and holds no arithmetic of its own.  The rules are the device object of cpq_src's, and what can be
// shared of keeping them is object_support.hpp's.  No device-side tables of the call: what the kernels index with arrives by value.  Zeroed at create: hop sums, partial hops and filter states
// are cleared synchronously before create returns.  One stream: everything is enqueued on the object's stream, and the position
// advances only after the launch was enqueued without an error.  With cpq_loudness_set_true_peak a call also enqueues k_prog_peak
// behind k_prog_hops (the position advances after both); cpq_loudness_apply_device touches no programme state.
#include "engine_internal.hpp"

#include "object_support.hpp"

using cpqi::failTo;

struct cpq_loudness {
    cpq_loudness_desc desc{};
    int H = 0, maxHops = 0;
    long long pos = 0;                              // samples every programme has taken
    std::string lastError;
    hipStream_t stream = nullptr;
    cpqi::DeviceBuffer<double> tab, state, part, hops;      // section tables; [2 S][8]; [2 S]; [S][maxHops]
    cpqi::DeviceBuffer<cpq::ProgRecord> rec;                // [S]
    cpqi::RowStage rows;                                    // [2 S][rows.cap]: the host rows of cpq_loudness_process
    cpqi::DeviceBuffer<double> pk;                          // [2 S][kPeakState]: true peak per programme, allocated by its switch
    bool peakOn = false;
    cpqi::DeviceBuffer<double> gains;                       // [S]: the gains of cpq_loudness_apply_device
};

namespace {

constexpr size_t kTabDoubles = 2 * (size_t)cpq::kMeterSectionDoubles;

// the refusals of a call, host rows or device rows alike, all before any state moves; c: the plan of the call
int checkCall(cpq_loudness* p, const double* rows, int64_t stride, int32_t n, cpq::ProgCall& c)
{
    if (!rows) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "null buffer");
    if (n < 1 || n > cpq::kProgMaxCall) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "n_samples=%d outside 1..%d", n, cpq::kProgMaxCall);
    if (stride < n) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "row stride %lld shorter than its row of %d", (long long)stride, n);
    if (reinterpret_cast<uintptr_t>(rows) & 15u) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "buffers must be 16-byte aligned");
    if (!cpq::progPlan(p->pos, n, p->H, p->maxHops, p->desc.n_streams, stride, c))
        return failTo(&p->lastError, CPQ_ERR_UNSUPPORTED, "%d samples after %lld pass the %d hops of max_seconds=%g", n, p->pos, p->maxHops, p->desc.max_seconds);
    return CPQ_OK;
}

int runDevice(cpq_loudness* p, const double* dRows, const cpq::ProgCall& c)
{
    cpq::launch_prog_hops(p->stream, dRows, c, p->tab, p->state, p->part, p->hops);
    CPQ_OBJ_HIP(&p->lastError, hipGetLastError());
    if (p->peakOn) {
        cpq::PeakCall k;
        k.n = c.n; k.mask = cpq::progPeakMask(p->desc.sample_rate); k.rows = 2 * c.streams; k.stride = c.stride;
        cpq::launch_prog_peak(p->stream, dRows, k, p->pk);
        CPQ_OBJ_HIP(&p->lastError, hipGetLastError());
    }
    p->pos += c.n;
    return CPQ_OK;
}

int clearState(cpq_loudness* p)
{
    CPQ_OBJ_HIP(&p->lastError, hipMemsetAsync(p->state, 0, p->state.count() * sizeof(double), p->stream));
    CPQ_OBJ_HIP(&p->lastError, hipMemsetAsync(p->part, 0, p->part.count() * sizeof(double), p->stream));
    CPQ_OBJ_HIP(&p->lastError, hipMemsetAsync(p->hops, 0, p->hops.count() * sizeof(double), p->stream));
    if (p->pk) CPQ_OBJ_HIP(&p->lastError, hipMemsetAsync(p->pk, 0, p->pk.count() * sizeof(double), p->stream));
    CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
    p->pos = 0;
    return CPQ_OK;
}

int createDevice(cpq_loudness* p)
{
    const size_t S = (size_t)p->desc.n_streams;
    CPQ_TRY(cpqi::allocAll(nullptr, { { p->tab, kTabDoubles }, { p->state, 16 * S, true }, { p->part, 2 * S, true },
                                      { p->hops, S * (size_t)p->maxHops, true }, { p->rec, S }, { p->gains, S } },
                           "hop sums of %d streams and %d hops could not be allocated", p->desc.n_streams, p->maxHops));
    std::vector<double> tab(kTabDoubles, 0.0);
    double pre[5], rlb[5];
    cpq::meterKWeighting(p->desc.sample_rate, pre, rlb);
    cpq::meterSectionTables(pre, tab.data());
    cpq::meterSectionTables(rlb, tab.data() + cpq::kMeterSectionDoubles);
    CPQ_OBJ_HIP(nullptr, hipMemcpy(p->tab, tab.data(), kTabDoubles * sizeof(double), hipMemcpyHostToDevice));
    CPQ_OBJ_HIP(nullptr, hipDeviceSynchronize());      // the clears have run before the first call, whatever its stream
    return CPQ_OK;
}

}  // namespace

extern "C" {

int32_t cpq_loudness_create(const cpq_loudness_desc* d, cpq_loudness** out)
{
    if (!d || !out) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (d->n_streams < 1 || d->n_streams > 32767) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "n_streams %d outside 1..32767", d->n_streams);
    if (d->flags) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "unknown flags");
    if (!(d->sample_rate > 0.0) || !std::isfinite(d->sample_rate)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "sample_rate must be finite and > 0");
    const long long maxHops = cpq::progMaxHops(d->max_seconds);
    if (!maxHops) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "max_seconds must be finite and > 0");
    const int H = cpq::progHop(d->sample_rate);
    if (!H) return failTo(nullptr, CPQ_ERR_UNSUPPORTED, "sample_rate %g is not a whole number of Hz in 8000..768000 that is divisible by 10", d->sample_rate);
    if (cpq::progShortCount(maxHops) > cpq::kProgSortMax)
        return failTo(nullptr, CPQ_ERR_UNSUPPORTED, "max_seconds=%g holds more than %d short-term blocks at the 1 s step", d->max_seconds, cpq::kProgSortMax);
    return cpqi::guardAlloc(nullptr, [&]() -> int {
        std::unique_ptr<cpq_loudness, void (*)(cpq_loudness*)> p(new cpq_loudness(), cpq_loudness_destroy);
        p->desc = *d;
        p->rows.rows = 2 * (size_t)d->n_streams;
        p->H = H;
        p->maxHops = (int)maxHops;
        CPQ_TRY(cpqi::checkCurrentDevice());
        CPQ_TRY(createDevice(p.get()));
        *out = p.release();
        return CPQ_OK;
    });
}

void cpq_loudness_destroy(cpq_loudness* p) { delete p; }

const char* cpq_loudness_last_error(const cpq_loudness* p) { return p ? p->lastError.c_str() : cpq_last_error(nullptr); }

int32_t cpq_loudness_reset(cpq_loudness* p)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    return clearState(p);
}

int32_t cpq_loudness_set_stream(cpq_loudness* p, void* stream)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    return cpqi::setStream(&p->lastError, p->stream, stream);
}

int32_t cpq_loudness_process_device(cpq_loudness* p, const double* d_rows, int64_t row_stride, int32_t n_samples)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    cpq::ProgCall c;
    CPQ_TRY(checkCall(p, d_rows, row_stride, n_samples, c));
    return runDevice(p, d_rows, c);
}

int32_t cpq_loudness_process(cpq_loudness* p, const double* rows, int64_t row_stride, int32_t n_samples)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    cpq::ProgCall c;
    CPQ_TRY(checkCall(p, rows, row_stride, n_samples, c));
    CPQ_TRY(p->rows.ensure(&p->lastError, p->stream, n_samples));
    c.stride = p->rows.cap;
    CPQ_TRY(p->rows.upload(&p->lastError, rows, row_stride, n_samples, hipMemcpyHostToDevice, p->stream));
    CPQ_TRY(runDevice(p, p->rows.buf, c));
    CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
    return CPQ_OK;
}

int32_t cpq_loudness_finish(cpq_loudness* p, cpq_loudness_result* out)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!out) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "null result");
    return cpqi::guardAlloc(&p->lastError, [&]() -> int {
        const int S = p->desc.n_streams;
        cpq::ProgFinish f;
        f.nHops = (int)(p->pos / p->H); f.H = p->H; f.maxHops = p->maxHops; f.zAbs = cpq::progAbsGate();
        std::vector<cpq::ProgRecord> rec((size_t)S);
        cpq::launch_prog_finish(p->stream, p->hops, f, S, p->rec);
        CPQ_OBJ_HIP(&p->lastError, hipGetLastError());
        CPQ_OBJ_HIP(&p->lastError, hipMemcpyAsync(rec.data(), p->rec, rec.size() * sizeof(cpq::ProgRecord), hipMemcpyDeviceToHost, p->stream));
        CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
        for (int s = 0; s < S; ++s) out[s] = cpq::progResult(rec[(size_t)s], f.nHops);
        return CPQ_OK;
    });
}

int32_t cpq_loudness_read_hops(cpq_loudness* p, int32_t stream, double* out, int64_t capacity, int64_t* n)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (stream < 0 || stream >= p->desc.n_streams) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "stream %d outside 0..%d", stream, p->desc.n_streams - 1);
    if (!n || capacity < 0 || (capacity > 0 && !out)) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "bad hop buffer");
    CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
    const int64_t have = p->pos / p->H, cnt = std::min(have, capacity);
    if (cnt > 0)
        CPQ_OBJ_HIP(&p->lastError, hipMemcpy(out, p->hops.get() + (size_t)stream * (size_t)p->maxHops, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost));
    *n = have;
    return CPQ_OK;
}

int32_t cpq_loudness_finish_host(const double* hops, int64_t n_hops, double sample_rate, cpq_loudness_result* out)
{
    if (!out || n_hops < 0 || (n_hops > 0 && !hops)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "null argument");
    cpq::ProgFinish f;
    f.H = cpq::progHop(sample_rate);
    if (!f.H) return failTo(nullptr, CPQ_ERR_UNSUPPORTED, "sample_rate %g is not a whole number of Hz in 8000..768000 that is divisible by 10", sample_rate);
    if (cpq::progShortCount(n_hops) > cpq::kProgSortMax) return failTo(nullptr, CPQ_ERR_UNSUPPORTED, "more than %d short-term blocks at the 1 s step", cpq::kProgSortMax);
    f.nHops = (int)n_hops; f.maxHops = (int)n_hops; f.zAbs = cpq::progAbsGate();
    return cpqi::guardAlloc(nullptr, [&] {
        *out = cpq::progResult(cpq::progFinishHost(hops, f), n_hops);
        return (int)CPQ_OK;
    });
}

int32_t cpq_loudness_gain(const cpq_loudness_result* r, double target_lufs, double* gain)
{
    if (!r || !gain || !std::isfinite(target_lufs)) return CPQ_ERR_INVALID_ARG;
    if (!std::isfinite(r->integrated)) return failTo(nullptr, CPQ_ERR_NOT_READY, "nothing passed the gates: no integrated loudness");
    *gain = std::pow(10.0, (target_lufs - r->integrated) / 20.0);
    return CPQ_OK;
}

int32_t cpq_loudness_set_true_peak(cpq_loudness* p, int32_t on)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (on != 0 && on != 1) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "on must be 0 or 1");
    if (p->pos) return failTo(&p->lastError, CPQ_ERR_NOT_READY, "true peak is switched at the start of a programme: %lld samples were taken; reset first", p->pos);
    CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
    if (!on) {
        p->peakOn = false;
        p->pk.reset();
        return CPQ_OK;
    }
    if (!p->pk) {
        const int rc = cpqi::allocAll(nullptr, { { p->pk, 2 * (size_t)p->desc.n_streams * cpq::kPeakState, true } }, "peak state");
        if (rc != CPQ_OK) return failTo(&p->lastError, rc, "the peak state of %d streams could not be allocated", p->desc.n_streams);
    } else {
        CPQ_OBJ_HIP(&p->lastError, hipMemset(p->pk, 0, p->pk.count() * sizeof(double)));
    }
    CPQ_OBJ_HIP(&p->lastError, hipDeviceSynchronize());        // cleared before the first call, whatever its stream
    p->peakOn = true;
    return CPQ_OK;
}

int32_t cpq_loudness_read_peaks(cpq_loudness* p, cpq_loudness_peaks* out)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!out) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "null result");
    if (!p->peakOn) return failTo(&p->lastError, CPQ_ERR_NOT_READY, "true peak is not switched on (cpq_loudness_set_true_peak)");
    return cpqi::guardAlloc(&p->lastError, [&]() -> int {
        const int S = p->desc.n_streams;
        std::vector<double> st(p->pk.count());
        CPQ_OBJ_HIP(&p->lastError, hipMemcpyAsync(st.data(), p->pk, st.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
        for (int s = 0; s < S; ++s)
            for (int ch = 0; ch < 2; ++ch) {
                const double* r = st.data() + (size_t)(2 * s + ch) * cpq::kPeakState;
                out[s].true_peak[ch] = r[cpq::kPeakTp];
                out[s].sample_peak[ch] = r[cpq::kPeakSp];
            }
        return CPQ_OK;
    });
}

int32_t cpq_loudness_peaks_host(const double* rows, int64_t row_stride, int32_t n_rows, int64_t n_samples, double sample_rate,
                                double* true_peak, double* sample_peak)
{
    if (!rows || !true_peak || !sample_peak) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "null argument");
    if (n_rows < 1 || n_samples < 0 || row_stride < n_samples) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "bad rows");
    if (!cpq::progHop(sample_rate)) return failTo(nullptr, CPQ_ERR_UNSUPPORTED, "sample_rate %g is not a whole number of Hz in 8000..768000 that is divisible by 10", sample_rate);
    const int mask = cpq::progPeakMask(sample_rate);
    for (int32_t r = 0; r < n_rows; ++r) {
        double st[cpq::kPeakState] = {};
        cpq::progPeakRowHost(rows + (size_t)r * (size_t)row_stride, n_samples, mask, st);
        true_peak[r] = st[cpq::kPeakTp];
        sample_peak[r] = st[cpq::kPeakSp];
    }
    return CPQ_OK;
}

int32_t cpq_loudness_gain_limited(const cpq_loudness_result* r, const cpq_loudness_peaks* pk, double target_lufs, double max_true_peak_dbtp,
                                  double* gain, int32_t* limited)
{
    if (!r || !pk || !gain || !limited || !std::isfinite(target_lufs) || !std::isfinite(max_true_peak_dbtp)) return CPQ_ERR_INVALID_ARG;
    double peak = 0.0;
    for (double v : { pk->true_peak[0], pk->true_peak[1], pk->sample_peak[0], pk->sample_peak[1] }) {
        if (!std::isfinite(v) || v < 0.0) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "a peak is not a finite linear value >= 0");
        peak = v > peak ? v : peak;
    }
    if (!std::isfinite(r->integrated)) return failTo(nullptr, CPQ_ERR_NOT_READY, "nothing passed the gates: no integrated loudness");
    bool lim = false;
    *gain = cpq::progGainLimited(r->integrated, peak, target_lufs, max_true_peak_dbtp, lim);
    *limited = lim ? 1 : 0;
    return CPQ_OK;
}

int32_t cpq_loudness_apply_device(cpq_loudness* p, const double* gains, const double* d_in, int64_t in_stride, double* d_out, int64_t out_stride,
                                  int32_t n_samples)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!gains) d_in = nullptr;         // null gains are a null buffer, the first refusal
    CPQ_TRY(cpqi::checkRowPair(&p->lastError, d_in, in_stride, d_out, out_stride, n_samples, cpq::kProgMaxCall, true));
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
    const int S = p->desc.n_streams;
    for (int s = 0; s < S; ++s)
        if (!std::isfinite(gains[s])) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "the gain of stream %d is not finite", s);
    if (cpq::progApplyOverlap(a / 8, in_stride, b / 8, out_stride, 2 * S, n_samples))
        return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, cpqi::kRowsOverlap);
    cpq::ApplyCall c;
    c.n = n_samples; c.rows = 2 * S; c.inStride = in_stride; c.outStride = out_stride;
    c.wide = in_stride % 2 == 0 && out_stride % 2 == 0;
    CPQ_OBJ_HIP(&p->lastError, hipMemcpyAsync(p->gains, gains, (size_t)S * sizeof(double), hipMemcpyHostToDevice, p->stream));
    cpq::launch_prog_apply(p->stream, d_in, c, p->gains, d_out);
    CPQ_OBJ_HIP(&p->lastError, hipGetLastError());
    return CPQ_OK;
}

}  // extern "C"
