// engine_src.cpp -- cpq_src: streaming sample-rate conversion of audio, an object of its own beside cpq_engine.  The plan of a
// call (which outputs, where their taps lie in [ history | new samples ], what is kept) is src_plan.hpp's.  The host object
// (CPQ_SRC_HOST) computes the rows with src_host.hpp.  The device object (CPQ_SRC_DEVICE) launches resample_kernels.hip's
// k_src_resample and k_src_keep with the launch src_device_plan.hpp states from the same plan: this file allocates, launches and
// copies, and holds no arithmetic of its own.  Both objects share the state (cpq::SrcState), the checks of every call and the
// answers that are host arithmetic (out_count, max_out, latency, reset).
//
// The device object keeps three rules.  No device-side tables: what the kernels index with arrives by value.
// Zeroed at create: taps are uploaded once, synchronously, hist is cleared there; reset and flush are host state only, since a
// history extent of 0 means that no history sample is read.  One stream: both launches of a call go to the object's stream,
// resample first, and the state advances only after both were enqueued without an error.
#include "engine_internal.hpp"

#include "src_host.hpp"

struct cpq_src {
    cpq_src_desc desc{};
    cpq::SrcHost h;             // the device object uses its geometry and state, not its rows
    int maxOut = 0;
    std::string lastError;
    bool device = false;
    hipStream_t stream = nullptr;
    cpqi::DeviceBuffer<double> taps, hist;      // [L][T], [n_channels][srcHistoryBound]
    cpqi::DeviceBuffer<double> rowsIn, rowsOut; // [n_channels][max_in], [n_channels][maxOut]: the host rows of cpq_src_process
    hipEvent_t ev[2] = {};
    double lastKernelMs = -1.0;
    ~cpq_src()
    {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

int rfail(cpq_src* s, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (s) s->lastError = buf;
    else return cpqi::fail(nullptr, code, "%s", buf);       // before an object exists: cpq_last_error(NULL) has it
    return code;
}

#define CPQ_SRC_HIP(s, call)                                                                          \
    do {                                                                                              \
        hipError_t err__ = (call);                                                                    \
        if (err__ != hipSuccess) {                                                                    \
            (void)hipGetLastError();                                                                  \
            return rfail((s), CPQ_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(err__));      \
        }                                                                                             \
    } while (0)

// the refusals of a call, host rows or device rows alike, all before any state changes; n: the samples the call writes
int checkCall(cpq_src* s, const double* in, int64_t in_stride, int32_t n_in, double* out, int64_t out_stride, int32_t out_capacity, int32_t flush,
              int32_t* n_out, int& n)
{
    if (!n_out) return rfail(s, CPQ_ERR_INVALID_ARG, "null n_out");
    if (n_in < 0 || n_in > s->desc.max_in) return rfail(s, CPQ_ERR_INVALID_ARG, "%d samples outside 0..%d", n_in, s->desc.max_in);
    if (n_in > 0 && !in) return rfail(s, CPQ_ERR_INVALID_ARG, "null input");
    if (in_stride < n_in) return rfail(s, CPQ_ERR_INVALID_ARG, "input stride %lld shorter than its row of %d", (long long)in_stride, n_in);
    n = (int)s->h.outCount(n_in, flush != 0);
    if (out_capacity < n) return rfail(s, CPQ_ERR_INVALID_ARG, "out_capacity %d below the %d samples of this call", out_capacity, n);
    if (n > 0 && !out) return rfail(s, CPQ_ERR_INVALID_ARG, "null output");
    if (out_stride < n) return rfail(s, CPQ_ERR_INVALID_ARG, "output stride %lld shorter than its row of %d", (long long)out_stride, n);
    if (n_in > 0 && n > 0) {
        const int64_t ch = s->desc.n_channels - 1;
        const uintptr_t a0 = (uintptr_t)in, a1 = (uintptr_t)(in + ch * in_stride + n_in), b0 = (uintptr_t)out, b1 = (uintptr_t)(out + ch * out_stride + n);
        if (a0 < b1 && b0 < a1) return rfail(s, CPQ_ERR_INVALID_ARG, "in and out overlap");
    }
    return CPQ_OK;
}

// a checked call on device rows: enqueued on the object's stream, the state advanced once everything was
int runDevice(cpq_src* s, const double* dIn, int64_t inStride, int nIn, double* dOut, int64_t outStride, bool flush, int32_t* nOut)
{
    cpq::SrcHost& h = s->h;
    if (h.copy) {
        if (nIn > 0)
            CPQ_SRC_HIP(s, hipMemcpy2DAsync(dOut, (size_t)outStride * sizeof(double), dIn, (size_t)inStride * sizeof(double), (size_t)nIn * sizeof(double),
                                            (size_t)h.channels, hipMemcpyDeviceToDevice, s->stream));
        *nOut = nIn;
        return CPQ_OK;
    }
    const cpq::SrcCall call = cpq::srcPlan(h.g, h.s, nIn, flush, h.fresh());
    const cpq::SrcLaunch a = cpq::srcLaunch(h.g, call, h.s.hLen, nIn, h.channels, inStride, outStride);
    cpq::launch_src_resample(s->stream, s->taps, s->hist, dIn, dOut, a);
    cpq::launch_src_keep(s->stream, s->hist, dIn, a);
    CPQ_SRC_HIP(s, hipGetLastError());
    h.s = call.next;
    *nOut = a.nOut;
    return CPQ_OK;
}

// cpq_src_process of the device object: the rows through the object's own buffers
int runDeviceHostRows(cpq_src* s, const double* in, int64_t inStride, int nIn, double* out, int64_t outStride, int n, bool flush, int32_t* nOut)
{
    const size_t channels = (size_t)s->desc.n_channels, pitchIn = (size_t)s->desc.max_in * sizeof(double), pitchOut = (size_t)s->maxOut * sizeof(double);
    if (nIn > 0)
        CPQ_SRC_HIP(s, hipMemcpy2DAsync(s->rowsIn, pitchIn, in, (size_t)inStride * sizeof(double), (size_t)nIn * sizeof(double), channels,
                                        hipMemcpyHostToDevice, s->stream));
    CPQ_SRC_HIP(s, hipEventRecord(s->ev[0], s->stream));
    int32_t wrote = 0;
    CPQ_TRY(runDevice(s, s->rowsIn, s->desc.max_in, nIn, s->rowsOut, s->maxOut, flush, &wrote));
    CPQ_SRC_HIP(s, hipEventRecord(s->ev[1], s->stream));
    if (n > 0)
        CPQ_SRC_HIP(s, hipMemcpy2DAsync(out, (size_t)outStride * sizeof(double), s->rowsOut, pitchOut, (size_t)n * sizeof(double), channels,
                                        hipMemcpyDeviceToHost, s->stream));
    CPQ_SRC_HIP(s, hipStreamSynchronize(s->stream));
    float ms = 0.0f;
    CPQ_SRC_HIP(s, hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    s->lastKernelMs = ms;
    *nOut = wrote;
    return CPQ_OK;
}

int createDevice(cpq_src* s)
{
    const cpq::SrcHost& h = s->h;
    CPQ_TRY(cpqi::allocAll(nullptr, { { s->rowsIn, (size_t)h.channels * (size_t)s->desc.max_in }, { s->rowsOut, (size_t)h.channels * (size_t)s->maxOut } },
                           "row buffers for %d channels of %d samples could not be allocated", h.channels, s->desc.max_in));
    for (auto& e : s->ev) CPQ_SRC_HIP(nullptr, hipEventCreate(&e));
    if (h.copy) return CPQ_OK;
    CPQ_TRY(cpqi::allocAll(nullptr, { { s->taps, h.taps.size() }, { s->hist, (size_t)h.channels * (size_t)cpq::srcHistoryBound(h.g), true } },
                           "filter and history of %d channels could not be allocated", h.channels));
    CPQ_SRC_HIP(nullptr, hipMemcpy(s->taps, h.taps.data(), h.taps.size() * sizeof(double), hipMemcpyHostToDevice));
    CPQ_SRC_HIP(nullptr, hipDeviceSynchronize());       // the clear of hist has run before the first call, whatever its stream
    return CPQ_OK;
}

}  // namespace

extern "C" {

int32_t cpq_src_create(const cpq_src_desc* d, cpq_src** out)
{
    if (!d || !out) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (d->n_channels < 1 || d->n_channels > 65535) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "n_channels %d outside 1..65535", d->n_channels);
    if (d->max_in < 1) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "max_in must be >= 1");
    if (d->start_period < 0 || d->start_period > (INT64_C(1) << 50)) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "start_period outside 0..2^50");
    if (d->flags & ~(CPQ_SRC_HOST | CPQ_SRC_DEVICE)) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "unknown flags");
    if ((d->flags & CPQ_SRC_HOST) && (d->flags & CPQ_SRC_DEVICE)) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "CPQ_SRC_HOST and CPQ_SRC_DEVICE exclude each other");
    if (d->phase != CPQ_RESAMPLE_LINEAR_PHASE && d->phase != CPQ_RESAMPLE_MINIMUM_PHASE) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "unknown phase response");
    if (!(d->in_rate > 0.0) || !std::isfinite(d->in_rate) || !(d->out_rate > 0.0) || !std::isfinite(d->out_rate))
        return rfail(nullptr, CPQ_ERR_INVALID_ARG, "sample rates must be finite and > 0");
    if (d->phase == CPQ_RESAMPLE_MINIMUM_PHASE) return rfail(nullptr, CPQ_ERR_UNSUPPORTED, "the minimum-phase resampler is not built");
    if (!d->flags) return rfail(nullptr, CPQ_ERR_UNSUPPORTED, "say CPQ_SRC_HOST or CPQ_SRC_DEVICE");
    try {
        std::unique_ptr<cpq_src, void (*)(cpq_src*)> s(new cpq_src(), cpq_src_destroy);
        s->desc = *d;
        s->device = (d->flags & CPQ_SRC_DEVICE) != 0;
        cpq::SrcHost& h = s->h;
        h.channels = d->n_channels;
        h.copy = std::fabs(d->in_rate - d->out_rate) <= 1e-6;
        s->maxOut = d->max_in;
        if (!h.copy) {
            cpq::ResampleDesign design;
            const char* why = "";
            const int rc = cpq::resampleDesign(d->in_rate, d->out_rate, design, &why);
            if (rc != CPQ_OK) return rfail(nullptr, rc, "%s", why);
            h.g = cpq::SrcGeometry{ design.L, design.M, design.T };
            h.taps = std::move(design.taps);
            const int64_t maxOut = cpq::srcMaxOut(h.g, d->max_in);
            if (maxOut > (1 << 30) || (int64_t)d->max_in + cpq::srcHistoryBound(h.g) > (1 << 30))
                return rfail(nullptr, CPQ_ERR_UNSUPPORTED, "a call of %d samples would write more than 2^30", d->max_in);
            s->maxOut = (int)maxOut;
            h.startPeriod = d->start_period;
            if (!s->device) h.hist.assign((size_t)d->n_channels * (size_t)cpq::srcHistoryBound(h.g), 0.0);
        }
        h.reset();
        if (s->device) {
            CPQ_TRY(cpqi::checkCurrentDevice());
            CPQ_TRY(createDevice(s.get()));
        }
        *out = s.release();
        return CPQ_OK;
    } catch (const std::exception&) {
        return rfail(nullptr, CPQ_ERR_OOM, "host allocation failed");
    }
}

void cpq_src_destroy(cpq_src* s) { delete s; }

const char* cpq_src_last_error(const cpq_src* s) { return s ? s->lastError.c_str() : cpq_last_error(nullptr); }

int32_t cpq_src_reset(cpq_src* s)
{
    if (!s) return CPQ_ERR_INVALID_ARG;
    s->h.reset();
    return CPQ_OK;
}

int32_t cpq_src_latency(const cpq_src* s) { return s ? s->h.g.T / 2 : CPQ_ERR_INVALID_ARG; }

int32_t cpq_src_out_count(const cpq_src* s, int32_t n_in, int32_t flush)
{
    if (!s || n_in < 0 || n_in > s->desc.max_in) return CPQ_ERR_INVALID_ARG;
    return (int32_t)s->h.outCount(n_in, flush != 0);
}

int32_t cpq_src_max_out(const cpq_src* s) { return s ? s->maxOut : CPQ_ERR_INVALID_ARG; }

int32_t cpq_src_process(cpq_src* s, const double* in, int64_t in_stride, int32_t n_in, double* out, int64_t out_stride, int32_t out_capacity,
                        int32_t flush, int32_t* n_out)
{
    if (!s) return CPQ_ERR_INVALID_ARG;
    int n = 0;
    CPQ_TRY(checkCall(s, in, in_stride, n_in, out, out_stride, out_capacity, flush, n_out, n));
    if (s->device) return runDeviceHostRows(s, in, in_stride, n_in, out, out_stride, n, flush != 0, n_out);
    try {
        *n_out = s->h.process(in, (size_t)in_stride, n_in, out, (size_t)out_stride, flush != 0);
        return CPQ_OK;
    } catch (const std::exception&) {
        return rfail(s, CPQ_ERR_OOM, "host allocation failed");
    }
}

int32_t cpq_src_process_device(cpq_src* s, const double* d_in, int64_t in_stride, int32_t n_in, double* d_out, int64_t out_stride,
                               int32_t out_capacity, int32_t flush, int32_t* n_out)
{
    if (!s) return CPQ_ERR_INVALID_ARG;
    if (!s->device) return rfail(s, CPQ_ERR_INVALID_ARG, "cpq_src_process_device on a host object");
    int n = 0;
    CPQ_TRY(checkCall(s, d_in, in_stride, n_in, d_out, out_stride, out_capacity, flush, n_out, n));
    return runDevice(s, d_in, in_stride, n_in, d_out, out_stride, flush != 0, n_out);
}

int32_t cpq_src_set_stream(cpq_src* s, void* stream)
{
    if (!s) return CPQ_ERR_INVALID_ARG;
    if (!s->device) return rfail(s, CPQ_ERR_INVALID_ARG, "cpq_src_set_stream on a host object");
    CPQ_SRC_HIP(s, hipStreamSynchronize(s->stream));        // what was enqueued has run before a call on the new stream touches hist
    s->stream = (hipStream_t)stream;
    return CPQ_OK;
}

double cpq_src_last_kernel_ms(const cpq_src* s) { return s && s->device ? s->lastKernelMs : -1.0; }

}  // extern "C"
