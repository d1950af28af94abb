// engine_dither.cpp -- the dither stage: processOutputDouble's ditherBitDepth > 0 branch (DSPCoreDouble.cpp:644-654) for the
// reference's three deterministic shapers, FixedNoiseShaper, Fixed15TapNoiseShaper and LatticeNoiseShaper.  The kernels are in
// dither_kernels.hip, the design and the seeds in dither_design.cpp; the host owns the coefficients and the per-channel state
// (error taps or lattice states, generator words).  Every stream is a DSPCore of its own, so every stream starts from the same
// two generator states (L, R).  The adaptive shaper's coefficients are the stream's: cpq_dither_set_adaptive_coeffs is
// applyMatchedCoefficients at the start of a callback (DSPCoreDouble.cpp:617-628).  In the whole-chain call the stage sits
// between the DC blocker and the meters (engine_core.cpp, meteredChain).  cpq_dither_process takes the refusals of
// checkBaseRows and the in-place hostRoundTrip; baseRate is the engine's (engine_internal.hpp).
#include "engine_internal.hpp"

namespace cpqi {

namespace {

int clearErrors(cpq_engine* e)
{
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    CPQ_HIP(e, hipMemset(e->ditherErr, 0, sizeof(double) * cpq::kDitherMaxOrder * (size_t)e->nCh));
    return CPQ_OK;
}

int seed(cpq_engine* e)
{
    std::vector<unsigned long long> words(4 * (size_t)e->nCh);
    for (int side = 0; side < 2; ++side) {
        unsigned long long s[4];
        cpq::ditherSeed(e->ditherShaper, baseRate(e), e->ditherBits, side, s);
        for (int k = 0; k < 4; ++k)
            for (int ch = side; ch < e->nCh; ch += 2) words[(size_t)k * e->nCh + ch] = s[k];
    }
    CPQ_HIP(e, hipMemcpy(e->ditherRng, words.data(), sizeof(unsigned long long) * words.size(), hipMemcpyHostToDevice));
    return CPQ_OK;
}

// streams [s0, s1) take the clamped set k[kLatticeOrder]; the whole table goes up
int loadAdaptive(cpq_engine* e, int s0, int s1, const double* k)
{
    for (int i = 0; i < cpq::kLatticeOrder; ++i)
        for (int ch = 2 * s0; ch < 2 * s1; ++ch) e->ditherCoefHost[(size_t)i * e->nCh + ch] = k[i];
    CPQ_HIP(e, hipMemcpy(e->ditherCoef, e->ditherCoefHost.data(), sizeof(double) * e->ditherCoefHost.size(), hipMemcpyHostToDevice));
    return CPQ_OK;
}

void design(cpq_engine* e)
{
    cpq::DitherParams& p = e->ditherParams;
    cpq::ditherDesign(baseRate(e), e->ditherShaper, e->ditherBits, p.c, &p.scale);     // arguments checked by cpq_engine_set_dither
    p.invScale = std::ldexp(1.0, e->ditherBits - 1);
    p.maxV = 1.0 - (1.0 / p.invScale);
}

int checkRows(cpq_engine* e, const void* in, const void* out, int n)
{
    return checkBaseRows(e, in, out, n, e && e->ditherShaper != CPQ_DITHER_OFF, "dither is off (cpq_engine_set_dither)", true);
}

}  // namespace

int refreshDither(cpq_engine* e)
{
    if (e->ditherShaper == CPQ_DITHER_OFF) return CPQ_OK;
    design(e);
    CPQ_TRY(clearErrors(e));                    // synchronises the stream
    return e->ditherShaper == CPQ_DITHER_FIXED15 ? seed(e) : CPQ_OK;
}

int enqueueDither(cpq_engine* e, const double* in, int64_t inStride, double* out, int64_t outStride, int n)
{
    if (e->ditherShaper == CPQ_DITHER_OFF) return CPQ_OK;
    cpq::DitherParams p = e->ditherParams;
    p.scrub = (e->outFlags & CPQ_OUT_HEADROOM) != 0;
    p.headroom = p.scrub ? cpq::kOutHeadroom : 1.0;
    ProfScope ps(e, CPQ_K_DITHER);
    if (!cpq::launch_dither(e->stream, in, inStride, out, outStride, n, e->nCh, cpq::ditherOrder(e->ditherShaper), p,
                            e->ditherShaper == CPQ_DITHER_ADAPTIVE9 ? e->ditherCoef.get() : nullptr, e->ditherErr, e->ditherRng))
        return fail(e, CPQ_ERR_UNSUPPORTED, "no dither kernel for shaper %d", e->ditherShaper);       // a missing kernel is an error
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

}  // namespace cpqi

using namespace cpqi;

extern "C" {

int32_t cpq_engine_set_dither(cpq_engine* e, int32_t shaper, int32_t bitDepth)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (shaper != CPQ_DITHER_OFF && !cpq::ditherOrder(shaper)) return fail(e, CPQ_ERR_INVALID_ARG, "unknown dither shaper %d", shaper);
    if (shaper != CPQ_DITHER_OFF && (bitDepth < 1 || bitDepth > 32)) return fail(e, CPQ_ERR_INVALID_ARG, "dither bit depth %d outside 1..32", bitDepth);
    if (shaper == CPQ_DITHER_OFF) bitDepth = 0;
    if (shaper == e->ditherShaper && bitDepth == e->ditherBits) return CPQ_OK;
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    if (shaper != CPQ_DITHER_OFF && !e->ditherErr) {
        CPQ_TRY(allocAll(e, { { e->ditherErr, cpq::kDitherMaxOrder * (size_t)e->nCh }, { e->ditherRng, 4 * (size_t)e->nCh },
                              { e->ditherCoef, cpq::kLatticeOrder * (size_t)e->nCh } },
                         "dither state buffers could not be allocated"));
        e->ditherCoefHost.assign(cpq::kLatticeOrder * (size_t)e->nCh, 0.0);
    }
    e->ditherShaper = shaper;
    e->ditherBits = bitDepth;
    if (shaper == CPQ_DITHER_OFF) return CPQ_OK;
    design(e);
    CPQ_TRY(clearErrors(e));
    if (shaper == CPQ_DITHER_ADAPTIVE9) CPQ_TRY(loadAdaptive(e, 0, e->desc.n_streams, e->ditherParams.c));     // the default set
    return seed(e);
}

int32_t cpq_dither_reset(cpq_engine* e)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (e->ditherShaper == CPQ_DITHER_OFF) return fail(e, CPQ_ERR_NOT_READY, "dither is off (cpq_engine_set_dither)");
    return clearErrors(e);
}

int32_t cpq_dither_set_adaptive_coeffs(cpq_engine* e, int32_t stream, const double* k, int32_t n)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (e->ditherShaper != CPQ_DITHER_ADAPTIVE9) return fail(e, CPQ_ERR_NOT_READY, "the adaptive shaper is not on (cpq_engine_set_dither)");
    int s0, s1;
    CPQ_TRY(streamRange(e, stream, s0, s1));
    if (n < 0 || n > cpq::kLatticeOrder) return fail(e, CPQ_ERR_INVALID_ARG, "%d coefficients outside 0..%d", n, cpq::kLatticeOrder);
    if (n > 0 && !k) return fail(e, CPQ_ERR_INVALID_ARG, "null coefficients");
    double c[cpq::kLatticeOrder];
    cpq::ditherClampAdaptive(k, n, c);
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    CPQ_TRY(loadAdaptive(e, s0, s1, c));
    // reset() of those streams: rows 0 .. kLatticeOrder - 1 of their channels
    CPQ_HIP(e, hipMemset2D(e->ditherErr.get() + 2 * s0, sizeof(double) * (size_t)e->nCh, 0, sizeof(double) * 2 * (size_t)(s1 - s0), cpq::kLatticeOrder));
    return CPQ_OK;
}

int32_t cpq_dither_get_adaptive_coeffs(const cpq_engine* e, int32_t stream, double k[9])
{
    if (!e || !k) return CPQ_ERR_INVALID_ARG;
    if (e->ditherShaper != CPQ_DITHER_ADAPTIVE9) return CPQ_ERR_NOT_READY;
    if (stream < 0 || stream >= e->desc.n_streams) return CPQ_ERR_INVALID_ARG;
    for (int i = 0; i < cpq::kLatticeOrder; ++i) k[i] = e->ditherCoefHost[(size_t)i * e->nCh + 2 * stream];
    return CPQ_OK;
}

int32_t cpq_dither_process_device(cpq_engine* e, const double* dIn, double* dOut, int32_t nSamples)
{
    CPQ_TRY(checkRows(e, dIn, dOut, nSamples));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueDither(e, dIn, nSamples, dOut, nSamples, nSamples);
}

int32_t cpq_dither_process(cpq_engine* e, const double* in, double* out, int32_t nSamples)
{
    CPQ_TRY(checkRows(e, in, out, nSamples));
    return hostRoundTrip(e, in, (size_t)nSamples, out, (size_t)nSamples, true,
                         [&](const double* a, double* b) { return enqueueDither(e, a, nSamples, b, nSamples, nSamples); });
}

}  // extern "C"
