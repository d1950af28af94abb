// engine_src.cpp -- cpq_src: streaming sample-rate conversion of audio, an object of its own beside cpq_engine.  The plan of a
// call (which outputs, where their taps lie in [ history | new samples ], what is kept) is src_plan.hpp's, the object that
// computes the rows src_host.hpp's; this file is the C ABI around them: the checks of cpq_src_create and of every call.  Only the
// host object (CPQ_SRC_HOST) is built: a request for a device object is refused, never served by the host in its place.
#include "engine_internal.hpp"

#include "src_host.hpp"

struct cpq_src {
    cpq_src_desc desc{};
    cpq::SrcHost h;
    int maxOut = 0;
    std::string lastError;
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

}  // namespace

extern "C" {

int32_t cpq_src_create(const cpq_src_desc* d, cpq_src** out)
{
    if (!d || !out) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (d->n_channels < 1 || d->n_channels > 65535) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "n_channels %d outside 1..65535", d->n_channels);
    if (d->max_in < 1) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "max_in must be >= 1");
    if (d->start_period < 0 || d->start_period > (INT64_C(1) << 50)) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "start_period outside 0..2^50");
    if (d->flags & ~CPQ_SRC_HOST) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "unknown flags");
    if (d->phase != CPQ_RESAMPLE_LINEAR_PHASE && d->phase != CPQ_RESAMPLE_MINIMUM_PHASE) return rfail(nullptr, CPQ_ERR_INVALID_ARG, "unknown phase response");
    if (!(d->in_rate > 0.0) || !std::isfinite(d->in_rate) || !(d->out_rate > 0.0) || !std::isfinite(d->out_rate))
        return rfail(nullptr, CPQ_ERR_INVALID_ARG, "sample rates must be finite and > 0");
    if (d->phase == CPQ_RESAMPLE_MINIMUM_PHASE) return rfail(nullptr, CPQ_ERR_UNSUPPORTED, "the minimum-phase resampler is not built");
    if (!(d->flags & CPQ_SRC_HOST)) return rfail(nullptr, CPQ_ERR_UNSUPPORTED, "the device object is not built: set CPQ_SRC_HOST");
    try {
        std::unique_ptr<cpq_src, void (*)(cpq_src*)> s(new cpq_src(), cpq_src_destroy);
        s->desc = *d;
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
            h.hist.assign((size_t)d->n_channels * (size_t)cpq::srcHistoryBound(h.g), 0.0);
        }
        h.reset();
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
    // every refusal before any state changes
    if (!s) return CPQ_ERR_INVALID_ARG;
    if (!n_out) return rfail(s, CPQ_ERR_INVALID_ARG, "null n_out");
    if (n_in < 0 || n_in > s->desc.max_in) return rfail(s, CPQ_ERR_INVALID_ARG, "%d samples outside 0..%d", n_in, s->desc.max_in);
    if (n_in > 0 && !in) return rfail(s, CPQ_ERR_INVALID_ARG, "null input");
    if (in_stride < n_in) return rfail(s, CPQ_ERR_INVALID_ARG, "input stride %lld shorter than its row of %d", (long long)in_stride, n_in);
    const int n = (int)s->h.outCount(n_in, flush != 0);
    if (out_capacity < n) return rfail(s, CPQ_ERR_INVALID_ARG, "out_capacity %d below the %d samples of this call", out_capacity, n);
    if (n > 0 && !out) return rfail(s, CPQ_ERR_INVALID_ARG, "null output");
    if (out_stride < n) return rfail(s, CPQ_ERR_INVALID_ARG, "output stride %lld shorter than its row of %d", (long long)out_stride, n);
    if (n_in > 0 && n > 0) {
        const int64_t ch = s->desc.n_channels - 1;
        const uintptr_t a0 = (uintptr_t)in, a1 = (uintptr_t)(in + ch * in_stride + n_in), b0 = (uintptr_t)out, b1 = (uintptr_t)(out + ch * out_stride + n);
        if (a0 < b1 && b0 < a1) return rfail(s, CPQ_ERR_INVALID_ARG, "in and out overlap");
    }
    try {
        *n_out = s->h.process(in, (size_t)in_stride, n_in, out, (size_t)out_stride, flush != 0);
        return CPQ_OK;
    } catch (const std::exception&) {
        return rfail(s, CPQ_ERR_OOM, "host allocation failed");
    }
}

}  // extern "C"
