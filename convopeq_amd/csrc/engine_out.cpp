// engine_out.cpp -- the output stage: the base-rate steps DSPCore::processOutputDouble runs on the chain's result when dither
// is off (DSPCoreDouble.cpp:577-744): the 3 Hz output UltraHighRateDCBlocker, the kOutputHeadroom multiply with the scrub, the
// SimplePeakLimiter and the hard clamp.  The kernels are in out_kernels.hip, the design in out_design.cpp; the host owns the
// tables and the carried states (two one-pole states per channel, one envelope per stream).  The whole-chain call runs the
// first two steps before the meters and the last two after them (engine_core.cpp, meteredChain).  cpq_out_process takes the
// refusals of checkBaseRows and the in-place hostRoundTrip, callbackLen and baseRate are the engine's (engine_internal.hpp).
#include "engine_internal.hpp"

namespace cpqi {

namespace {

constexpr int kPreFlags = CPQ_OUT_DC_BLOCK | CPQ_OUT_HEADROOM, kPostFlags = CPQ_OUT_LIMITER | CPQ_OUT_CLAMP;

int resetOutStage(cpq_engine* e)
{
    if (!e->outTab) return CPQ_OK;
    const std::vector<double> ones((size_t)e->desc.n_streams, 1.0);
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    CPQ_HIP(e, hipMemset(e->outDc, 0, sizeof(double) * 2 * (size_t)e->nCh));
    CPQ_HIP(e, hipMemcpy(e->outEnv, ones.data(), sizeof(double) * ones.size(), hipMemcpyHostToDevice));
    return CPQ_OK;
}

int checkRows(cpq_engine* e, const void* in, const void* out, int n)
{
    return checkBaseRows(e, in, out, n, e && e->outFlags, "the output stage is off (cpq_engine_set_output_stage)", true);
}

// both halves on rows of n samples; a half that is off copies nothing, so the first half that runs takes in -> out
int enqueueOutRows(cpq_engine* e, const double* in, double* out, int n)
{
    const double* src = in;
    if (e->outFlags & kPreFlags) {
        CPQ_TRY(enqueueOutPre(e, src, n, out, n, n));
        src = out;
    }
    if (e->outFlags & kPostFlags) CPQ_TRY(enqueueOutPost(e, src, n, out, n, n));
    return CPQ_OK;
}

}  // namespace

int refreshOutStage(cpq_engine* e)
{
    if (!e->outFlags) return CPQ_OK;
    double alpha[2], tab[2 * cpq::kOutSectionDoubles];
    cpq::outDesign(baseRate(e), alpha, &e->outRelease);
    cpq::outSectionTable(alpha[0], tab);
    cpq::outSectionTable(alpha[1], tab + cpq::kOutSectionDoubles);
    CPQ_TRY(resetOutStage(e));              // synchronises the stream: nothing in flight reads the tables
    CPQ_HIP(e, hipMemcpy(e->outTab, tab, sizeof(tab), hipMemcpyHostToDevice));
    return CPQ_OK;
}

int enqueueOutPre(cpq_engine* e, const double* in, int64_t inStride, double* out, int64_t outStride, int n, bool headroom)
{
    const int flags = e->outFlags & (headroom ? kPreFlags : CPQ_OUT_DC_BLOCK);
    if (!flags) return CPQ_OK;
    ProfScope p(e, CPQ_K_OUT);
    cpq::launch_out_pre(e->stream, in, inStride, out, outStride, n, callbackLen(e), e->nCh, (flags & CPQ_OUT_DC_BLOCK) != 0,
                        (flags & CPQ_OUT_HEADROOM) != 0, e->outTab, e->outDc);
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

int enqueueOutPost(cpq_engine* e, const double* in, int64_t inStride, double* out, int64_t outStride, int n)
{
    if (!(e->outFlags & kPostFlags)) return CPQ_OK;
    ProfScope p(e, CPQ_K_OUT);
    cpq::launch_out_post(e->stream, in, inStride, out, outStride, n, e->desc.n_streams, (e->outFlags & CPQ_OUT_LIMITER) != 0,
                         (e->outFlags & CPQ_OUT_CLAMP) != 0, e->outRelease, e->outEnv);
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

}  // namespace cpqi

using namespace cpqi;

extern "C" {

int32_t cpq_engine_set_output_stage(cpq_engine* e, int32_t flags)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (flags & ~CPQ_OUT_ALL) return fail(e, CPQ_ERR_INVALID_ARG, "output stage flags %d", flags);
    if (flags == e->outFlags) return CPQ_OK;
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    if (flags && !e->outTab)
        CPQ_TRY(allocAll(e, { { e->outTab, 2 * (size_t)cpq::kOutSectionDoubles }, { e->outDc, 2 * (size_t)e->nCh },
                              { e->outEnv, (size_t)e->desc.n_streams } }, "output stage buffers could not be allocated"));
    e->outFlags = flags;
    return refreshOutStage(e);
}

int32_t cpq_out_reset(cpq_engine* e)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!e->outFlags) return fail(e, CPQ_ERR_NOT_READY, "the output stage is off (cpq_engine_set_output_stage)");
    return resetOutStage(e);
}

int32_t cpq_out_process_device(cpq_engine* e, const double* dIn, double* dOut, int32_t nSamples)
{
    CPQ_TRY(checkRows(e, dIn, dOut, nSamples));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueOutRows(e, dIn, dOut, nSamples);
}

int32_t cpq_out_process(cpq_engine* e, const double* in, double* out, int32_t nSamples)
{
    CPQ_TRY(checkRows(e, in, out, nSamples));
    return hostRoundTrip(e, in, (size_t)nSamples, out, (size_t)nSamples, true,
                         [&](const double* a, double* b) { return enqueueOutRows(e, a, b, nSamples); });
}

int32_t cpq_out_read_envelope(cpq_engine* e, int32_t stream, double* envelope)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!e->outFlags) return fail(e, CPQ_ERR_NOT_READY, "the output stage is off (cpq_engine_set_output_stage)");
    if (!envelope || stream < 0 || stream >= e->desc.n_streams) return fail(e, CPQ_ERR_INVALID_ARG, "stream %d", stream);
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    CPQ_HIP(e, hipMemcpy(envelope, e->outEnv + stream, sizeof(double), hipMemcpyDeviceToHost));
    return CPQ_OK;
}

}  // extern "C"
