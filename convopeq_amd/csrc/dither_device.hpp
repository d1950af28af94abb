// dither_device.hpp -- the device code the dither stage (dither_kernels.hip) and the quantizer (quant_kernels.hip) share: the
// shape of a wave's tile, its load, and FixedNoiseShaper / Fixed15TapNoiseShaper::processSample, one sample of one channel.  The
// generator draw and the lattice's processSample are lattice_device.hpp's.  Included inside a kernel file, after kernels.hpp;
// every function is inlined into the kernel that calls it.
#pragma once

#include "kernels.hpp"
#include "lattice_device.hpp"

namespace cpq {
namespace {

#ifndef CPQ_DITHER_CPL
#define CPQ_DITHER_CPL 1
#endif
constexpr int kDitherCpl = CPQ_DITHER_CPL;          // channels per lane (measured: RESULTS.md, "dither stage")
constexpr int kDitherRows = 64 * kDitherCpl;        // rows per wave
constexpr int kDitherStep = kDitherTile / kDitherCpl;   // samples per tile: rows x (step + 1) doubles stay below 64 KiB of LDS
constexpr int kDitherPitch = kDitherStep + 1;

// the wave's rows x len samples from t0 on, into the tile: lane = sample.  GAIN: row r times gain[(row0 + r) / 2], its stream's
template <bool GAIN = false>
__device__ __forceinline__ void dTileLoad(double* tile, const double* in, int64_t inStride, int row0, int rows, int t0, int len, int lane,
                                          const double* gain = nullptr)
{
    if (lane < len) {
#pragma unroll 8
        for (int r = 0; r < rows; ++r) {
            if constexpr (GAIN) tile[r * kDitherPitch + lane] = in[(row0 + r) * inStride + t0 + lane] * gain[(row0 + r) >> 1];
            else tile[r * kDitherPitch + lane] = in[(row0 + r) * inStride + t0 + lane];
        }
    }
}

// processSample: x in, yq out; e and s are the channel's state
template <int ORDER>
__device__ __forceinline__ double dSample(double x, double (&e)[ORDER], unsigned long long (&s)[4], const DitherParams& p)
{
    double fb;
    if constexpr (ORDER == 4) {
        fb = p.c[0] * e[0] + p.c[1] * e[1] + p.c[2] * e[2] + p.c[3] * e[3];
    } else {
        fb = 0.0;
#pragma unroll
        for (int k = 0; k < ORDER; ++k) fb += p.c[k] * e[k];
    }
    const double y = x - fb;
    double v = ORDER == 4 ? dFiniteOrZero(y) : y;
    if (v < -1.0) v = -1.0;
    else if (v > p.maxV) v = p.maxV;
    const double u1 = dUniform(s);
    const double u2 = dUniform(s);
    v += (u1 + u2 - 1.0) * p.scale;
    const double q = __builtin_rint(v * p.invScale);
    const double lim = 2.0 * p.scale;
    double yq, stored;
    if constexpr (ORDER == 4) {
        yq = dFiniteOrZero(q * p.scale);
        const double error = yq - y;
        stored = error < -lim ? -lim : (lim < error ? lim : error);         // std::clamp: a NaN stays
    } else {
        const double minQ = -p.invScale, maxQ = p.invScale - 1.0;
        yq = (q < minQ ? minQ : (maxQ < q ? maxQ : q)) * p.scale;           // std::clamp: a NaN stays
        const double error = yq - y;
        stored = error > -lim ? error : -lim;                               // max_sd: a NaN gives the second operand
        stored = stored < lim ? stored : lim;                               // min_sd
    }
    stored = dFiniteOrZero(stored);
#pragma unroll
    for (int k = ORDER - 1; k > 0; --k) e[k] = e[k - 1];
    e[0] = stored;
    return yq;
}

}  // namespace
}  // namespace cpq
