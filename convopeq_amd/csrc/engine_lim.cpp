// engine_lim.cpp -- cpq_limiter: look-ahead true-peak limiter per stereo programme, an object of its own beside cpq_engine.  The
// definition and the plan of a call are lim_plan.hpp's.  The host object (CPQ_LIM_HOST) computes the rows with lim_host.hpp.  The
// device object (CPQ_LIM_DEVICE) launches lim_kernels.hip's k_lim_apply and k_lim_keep with the launch lim_plan.hpp states from the
// same plan: this file checks, allocates, launches and copies, and holds no arithmetic of its own.
//
// The device object keeps the rules of the device object of cpq_src, with object_support.hpp where they share.
// No device-side tables: what the kernels index with arrives by value (the gains are values, not indices).  Cleared at create: hist is zeroed and the gains are uploaded
// synchronously; reset and flush are host state only, since a history extent of 0 means that no history sample is read and the
// first call of a programme starts the telemetry over.  One stream: both launches of a call go to the object's stream, apply
// first, and the state advances only after both were enqueued without an error.
//
// k_lim_apply reads the rows of a tile's neighbours, so it cannot run in place.  A call in place first copies its rows to a buffer
// of the object (device to device, on the stream) and limits from there: the price of in place is that copy.
#include "engine_internal.hpp"

#include "lim_host.hpp"
#include "object_support.hpp"

using cpqi::failTo;

static_assert(sizeof(cpq_limiter_telemetry) == sizeof(cpq::LimPartial) && offsetof(cpq_limiter_telemetry, limited_samples) == offsetof(cpq::LimPartial, limited),
              "the telemetry is copied out as the kernels fold it");

struct cpq_limiter {
    int streams = 0, W = 0, mask = 0;
    double rate = 0.0, c = 1.0;
    cpq::LimHost h;                     // the device object uses its state and gains, not its rows
    std::string lastError;
    bool device = false;
    bool telValid = false;              // a call has run since create / reset
    hipStream_t stream = nullptr;
    cpqi::DeviceBuffer<double> hist, gains;             // [2 S][limHalo(W)], [S]
    cpqi::DeviceBuffer<cpq::LimPartial> tel, part;      // [S], [S][partCap]
    int partCap = 0;
    cpqi::RowStage rowsIn, rowsOut;                     // [2 S][cap]: host rows, and in rowsIn the copy of a call in place
    bool timed = false;
    cpqi::TimingEvents<2> ev;                           // the last member: destroyed before the buffers are freed
};

namespace {

// the refusals of a call, host rows or device rows alike, all before any state moves.  n: the samples a row takes and gives
int checkRows(cpq_limiter* p, const double* in, int64_t inStride, const double* out, int64_t outStride, int32_t n, bool deviceRows)
{
    CPQ_TRY(cpqi::checkRowPair(&p->lastError, in, inStride, out, outStride, n, cpq::kLimMaxCall, deviceRows));
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    if (((a | b) & 7u) || cpq::progApplyOverlap(a / 8, inStride, b / 8, outStride, 2 * p->streams, n))
        return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, cpqi::kRowsOverlap);
    return CPQ_OK;
}

int checkFlush(cpq_limiter* p, const double* out, int64_t outStride, bool deviceRows)
{
    if (!out) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "null buffer");
    if (outStride < cpq::limD(p->W)) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "row stride %lld below the %d samples of a flush", (long long)outStride, cpq::limD(p->W));
    if (deviceRows && (reinterpret_cast<uintptr_t>(out) & 15u)) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "buffers must be 16-byte aligned");
    return CPQ_OK;
}

// a stage to rows of at least n samples, an even count: the wide path of the kernels wants even strides
int growRows(cpq_limiter* p, cpqi::RowStage& rows, int n) { return rows.ensure(&p->lastError, p->stream, (n + 1) & ~1); }

// a checked call on device rows that do not overlap: enqueued on the object's stream, the state advanced once everything was
int runDevice(cpq_limiter* p, const double* dIn, int64_t inStride, double* dOut, int64_t outStride, int n, bool flush)
{
    const cpq::LimCall call = cpq::limPlan(p->W, p->h.s, n, flush);
    const int tiles = (call.nOut + cpq::kLimTile - 1) / cpq::kLimTile;
    if (tiles > p->partCap) {
        CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
        if (cpqi::grow(nullptr, p->part, p->partCap, tiles, (size_t)p->streams, "tile partials") != CPQ_OK)
            return failTo(&p->lastError, CPQ_ERR_OOM, "the partials of %d tiles could not be allocated", tiles);
    }
    const cpq::LimLaunch a = cpq::limLaunch(p->W, p->mask, p->c, call, p->streams, inStride, outStride, p->partCap);
    CPQ_OBJ_HIP(&p->lastError, hipEventRecord(p->ev[0], p->stream));
    cpq::launch_lim_apply(p->stream, p->hist, p->gains, dIn, dOut, p->part, a);
    cpq::launch_lim_keep(p->stream, p->hist, p->gains, dIn, p->part, p->tel, a);
    CPQ_OBJ_HIP(&p->lastError, hipGetLastError());
    CPQ_OBJ_HIP(&p->lastError, hipEventRecord(p->ev[1], p->stream));
    p->h.s = call.next;
    p->telValid = true;
    p->timed = true;
    return CPQ_OK;
}

// device rows, in place or apart: in place goes through the object's copy
int runDeviceRows(cpq_limiter* p, const double* dIn, int64_t inStride, double* dOut, int64_t outStride, int n)
{
    if (dIn != dOut) return runDevice(p, dIn, inStride, dOut, outStride, n, false);
    CPQ_TRY(growRows(p, p->rowsIn, n));
    CPQ_TRY(p->rowsIn.upload(&p->lastError, dIn, inStride, n, hipMemcpyDeviceToDevice, p->stream));
    return runDevice(p, p->rowsIn.buf, p->rowsIn.cap, dOut, outStride, n, false);
}

// host rows through the object's buffers; in: null at a flush
int runDeviceHostRows(cpq_limiter* p, const double* in, int64_t inStride, double* out, int64_t outStride, int n, bool flush)
{
    const int nOut = flush ? cpq::limD(p->W) : n;
    if (!flush) CPQ_TRY(growRows(p, p->rowsIn, n));
    CPQ_TRY(growRows(p, p->rowsOut, nOut));
    if (!flush) CPQ_TRY(p->rowsIn.upload(&p->lastError, in, inStride, n, hipMemcpyHostToDevice, p->stream));
    CPQ_TRY(runDevice(p, flush ? nullptr : p->rowsIn.buf.get(), p->rowsIn.cap, p->rowsOut.buf, p->rowsOut.cap, n, flush));
    CPQ_TRY(p->rowsOut.download(&p->lastError, out, outStride, nOut, hipMemcpyDeviceToHost, p->stream));
    CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
    return CPQ_OK;
}

// the host object's rows
int hostProcess(cpq_limiter* p, const double* in, int64_t inStride, int n, double* out, int64_t outStride, bool flush)
{
    return cpqi::guardAlloc(&p->lastError, [&] {
        p->h.process(in, inStride, n, out, outStride, flush);
        p->telValid = true;
        return (int)CPQ_OK;
    });
}

int createDevice(cpq_limiter* p)
{
    const size_t S = (size_t)p->streams;
    CPQ_TRY(cpqi::allocAll(nullptr, { { p->hist, 2 * S * (size_t)cpq::limHalo(p->W), true }, { p->gains, S }, { p->tel, S, true } },
                           "history of %d streams at a window of %d could not be allocated", p->streams, p->W));
    CPQ_TRY(p->ev.create(nullptr));
    CPQ_OBJ_HIP(nullptr, hipMemcpy(p->gains, p->h.gains.data(), S * sizeof(double), hipMemcpyHostToDevice));
    CPQ_OBJ_HIP(nullptr, hipDeviceSynchronize());       // the clears have run before the first call, whatever its stream
    return CPQ_OK;
}

}  // namespace

extern "C" {

int32_t cpq_limiter_default_window(double sample_rate)
{
    if (!(sample_rate > 0.0) || !std::isfinite(sample_rate)) return CPQ_ERR_INVALID_ARG;
    return cpq::limDefaultWindow(sample_rate);
}

int32_t cpq_limiter_create(int32_t n_streams, double sample_rate, double ceiling_dbtp, int32_t window_samples, uint32_t flags, cpq_limiter** out)
{
    if (!out) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (n_streams < 1 || n_streams > 32767) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "n_streams %d outside 1..32767", n_streams);
    if (flags & ~(uint32_t)(CPQ_LIM_HOST | CPQ_LIM_DEVICE)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "unknown flags");
    if ((flags & CPQ_LIM_HOST) && (flags & CPQ_LIM_DEVICE)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "CPQ_LIM_HOST and CPQ_LIM_DEVICE exclude each other");
    if (!(sample_rate > 0.0) || !std::isfinite(sample_rate)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "sample_rate must be finite and > 0");
    if (!(ceiling_dbtp >= -200.0) || !(ceiling_dbtp <= 200.0)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "ceiling_dbtp outside -200..200");
    if (window_samples != 0 && (window_samples < cpq::kLimMinWindow || window_samples > cpq::kLimMaxWindow))
        return failTo(nullptr, CPQ_ERR_INVALID_ARG, "window_samples %d is neither 0 nor in %d..%d", window_samples, cpq::kLimMinWindow, cpq::kLimMaxWindow);
    if (!cpq::progHop(sample_rate))
        return failTo(nullptr, CPQ_ERR_UNSUPPORTED, "sample_rate %g is not a whole number of Hz in 8000..768000 that is divisible by 10", sample_rate);
    if (!flags) return failTo(nullptr, CPQ_ERR_UNSUPPORTED, "say CPQ_LIM_HOST or CPQ_LIM_DEVICE");
    return cpqi::guardAlloc(nullptr, [&]() -> int {
        std::unique_ptr<cpq_limiter, void (*)(cpq_limiter*)> p(new cpq_limiter(), cpq_limiter_destroy);
        p->streams = n_streams;
        p->rate = sample_rate;
        p->W = window_samples ? window_samples : cpq::limDefaultWindow(sample_rate);
        p->mask = cpq::progPeakMask(sample_rate);
        p->c = std::pow(10.0, ceiling_dbtp / 20.0);
        p->device = (flags & CPQ_LIM_DEVICE) != 0;
        p->h.init(p->W, p->mask, p->c, n_streams);
        p->rowsIn.rows = p->rowsOut.rows = 2 * (size_t)n_streams;
        if (p->device) {
            p->h.hist = std::vector<double>();          // the history is on the device
            CPQ_TRY(cpqi::checkCurrentDevice());
            CPQ_TRY(createDevice(p.get()));
        }
        *out = p.release();
        return CPQ_OK;
    });
}

void cpq_limiter_destroy(cpq_limiter* p) { delete p; }

const char* cpq_limiter_last_error(const cpq_limiter* p) { return p ? p->lastError.c_str() : cpq_last_error(nullptr); }

int32_t cpq_limiter_set_stream(cpq_limiter* p, void* stream)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!p->device) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "cpq_limiter_set_stream on a host object");
    return cpqi::setStream(&p->lastError, p->stream, stream);
}

int32_t cpq_limiter_reset(cpq_limiter* p)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    p->h.reset();
    p->telValid = false;
    return CPQ_OK;
}

int32_t cpq_limiter_latency(const cpq_limiter* p) { return p ? cpq::limD(p->W) : CPQ_ERR_INVALID_ARG; }

int32_t cpq_limiter_window(const cpq_limiter* p) { return p ? p->W : CPQ_ERR_INVALID_ARG; }

int32_t cpq_limiter_set_gains(cpq_limiter* p, const double* gains)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!gains) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "null gains");
    for (int s = 0; s < p->streams; ++s)
        if (!std::isfinite(gains[s]) || gains[s] < 0.0) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "the gain of stream %d is not finite and >= 0", s);
    if (p->h.s.pos)
        return failTo(&p->lastError, CPQ_ERR_NOT_READY, "gains are set at the start of a programme: %lld samples were taken; flush or reset first", p->h.s.pos);
    if (p->device) {
        CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));    // the last programme's launches have read the gains they ran with
        CPQ_OBJ_HIP(&p->lastError, hipMemcpy(p->gains, gains, (size_t)p->streams * sizeof(double), hipMemcpyHostToDevice));
    }
    std::copy(gains, gains + p->streams, p->h.gains.begin());
    return CPQ_OK;
}

int32_t cpq_limiter_process_device(cpq_limiter* p, const double* d_in, int64_t in_stride, double* d_out, int64_t out_stride, int32_t n_samples)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!p->device) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "cpq_limiter_process_device on a host object");
    CPQ_TRY(checkRows(p, d_in, in_stride, d_out, out_stride, n_samples, true));
    return runDeviceRows(p, d_in, in_stride, d_out, out_stride, n_samples);
}

int32_t cpq_limiter_process(cpq_limiter* p, const double* in, int64_t in_stride, double* out, int64_t out_stride, int32_t n_samples)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(checkRows(p, in, in_stride, out, out_stride, n_samples, false));
    if (p->device) return runDeviceHostRows(p, in, in_stride, out, out_stride, n_samples, false);
    return hostProcess(p, in, in_stride, n_samples, out, out_stride, false);
}

int32_t cpq_limiter_flush_device(cpq_limiter* p, double* d_out, int64_t out_stride)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!p->device) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "cpq_limiter_flush_device on a host object");
    CPQ_TRY(checkFlush(p, d_out, out_stride, true));
    return runDevice(p, nullptr, 0, d_out, out_stride, 0, true);
}

int32_t cpq_limiter_flush(cpq_limiter* p, double* out, int64_t out_stride)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(checkFlush(p, out, out_stride, false));
    if (p->device) return runDeviceHostRows(p, nullptr, 0, out, out_stride, 0, true);
    return hostProcess(p, nullptr, 0, 0, out, out_stride, true);
}

int32_t cpq_limiter_read_telemetry(cpq_limiter* p, cpq_limiter_telemetry* out)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!out) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "null result");
    if (p->device) CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
    if (p->device && p->telValid) {
        CPQ_OBJ_HIP(&p->lastError, hipMemcpy(out, p->tel, (size_t)p->streams * sizeof(cpq::LimPartial), hipMemcpyDeviceToHost));
        return CPQ_OK;
    }
    for (int s = 0; s < p->streams; ++s) {
        out[s].min_gain = p->telValid ? p->h.tel[(size_t)s].minGain : 1.0;
        out[s].limited_samples = p->telValid ? p->h.tel[(size_t)s].limited : 0;
    }
    return CPQ_OK;
}

double cpq_limiter_last_kernel_ms(cpq_limiter* p)
{
    if (!p || !p->device || !p->timed) return -1.0;
    if (hipEventSynchronize(p->ev[1]) != hipSuccess) {
        (void)hipGetLastError();
        return -1.0;
    }
    return p->ev.elapsed(0, 1);
}

}  // extern "C"
