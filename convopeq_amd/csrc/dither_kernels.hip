// dither_kernels.hip -- the dither stage on gfx950: FixedNoiseShaper / Fixed15TapNoiseShaper::processStereoBlock of the reference
// (src/FixedNoiseShaper.h:162-184, 272-297; src/Fixed15TapNoiseShaper.h:204-230, 318-342) on rows [channel][sample].
//
// The quantiser sits inside the error feedback loop, so a channel is one sequential chain and no scan reproduces it: the only
// parallelism is across channels.  k_dither<ORDER> runs one wave per workgroup; a lane owns kDitherCpl consecutive channels (1: a
// channel; 2: a stream, L and R as two independent chains in one instruction stream) and keeps their error taps (a shift register,
// e[0] the newest) and the four 64-bit words of their xoshiro256++ generators in registers for the whole call.
//
// Rows are [channel][sample], so lanes walking their own rows would touch 64 cache lines per load.  A tile of kDitherTile samples
// x the wave's rows goes through LDS instead: the wave reads each row's stretch with lane = sample (one 512-byte line per
// instruction), writes tile[row][t] with a row pitch of kDitherTile + 1 doubles, each lane walks its own row in place, and the
// tile is stored the way it came.  Pitch 65 is odd: lane l reads the double at 65 l + t, its dword pair at banks 2 (65 l + t) mod
// 64, distinct for the 32 lanes an 8-byte LDS access serves together; the staging writes are consecutive doubles.  Loads and
// stores are single doubles, so a row on an odd double or with any stride is nothing special, and a tile is read whole before any
// of it is written, so in and out may be the same rows.
#include "kernels.hpp"

namespace cpq {
namespace {

#ifndef CPQ_DITHER_CPL
#define CPQ_DITHER_CPL 1
#endif
constexpr int kDitherCpl = CPQ_DITHER_CPL;          // channels per lane (measured: RESULTS.md, "dither stage")
constexpr int kDitherRows = 64 * kDitherCpl;        // rows per wave
constexpr int kDitherStep = kDitherTile / kDitherCpl;   // samples per tile: rows x (step + 1) doubles stay below 64 KiB of LDS
constexpr int kDitherPitch = kDitherStep + 1;

__device__ __forceinline__ unsigned long long dRotl(unsigned long long x, int k) { return (x << k) | (x >> (64 - k)); }

__device__ __forceinline__ double dUniform(unsigned long long (&s)[4])
{
    const unsigned long long result = dRotl(s[0] + s[3], 23) + s[0];
    const unsigned long long t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = dRotl(s[3], 45);
    return (double)(result >> 11) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ double dFiniteOrZero(double v) { return fabs(v) < __builtin_huge_val() ? v : 0.0; }

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

// grid: ceil(nCh / kDitherRows) workgroups of one wave.  err [kDitherMaxOrder][nCh], rng [4][nCh]
template <int ORDER>
__global__ void __launch_bounds__(64)
k_dither(const double* in, int64_t inStride, double* out, int64_t outStride, int n, int nCh, DitherParams p, double* __restrict__ err,
         unsigned long long* __restrict__ rng)
{
    __shared__ double tile[kDitherRows * kDitherPitch];
    const int lane = threadIdx.x;
    const int row0 = blockIdx.x * kDitherRows;
    const int rows = min(kDitherRows, nCh - row0);                  // >= 1
    double e[kDitherCpl][ORDER];
    unsigned long long s[kDitherCpl][4];
#pragma unroll
    for (int c = 0; c < kDitherCpl; ++c) {
        const int r = lane * kDitherCpl + c;
        const bool live = r < rows;
#pragma unroll
        for (int k = 0; k < ORDER; ++k) e[c][k] = live ? err[(size_t)k * nCh + row0 + r] : 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) s[c][k] = live ? rng[(size_t)k * nCh + row0 + r] : 1ull;
    }
    for (int t0 = 0; t0 < n; t0 += kDitherStep) {
        const int len = min(kDitherStep, n - t0);
        if (lane < len) {
#pragma unroll 8
            for (int r = 0; r < rows; ++r) tile[r * kDitherPitch + lane] = in[(row0 + r) * inStride + t0 + lane];
        }
        __syncthreads();
        double* mine = tile + lane * kDitherCpl * kDitherPitch;
        if (lane * kDitherCpl < rows) {
            int t = 0;
            for (; t + ORDER <= len; t += ORDER) {                  // whole groups: the shift register turns once, no moves survive
#pragma unroll
                for (int k = 0; k < ORDER; ++k) {
#pragma unroll
                    for (int c = 0; c < kDitherCpl; ++c) {
                        const double yq = dSample<ORDER>(mine[c * kDitherPitch + t + k] * p.headroom, e[c], s[c], p);
                        mine[c * kDitherPitch + t + k] = p.scrub ? (fabs(yq) < 1.0e300 ? yq : 0.0) : yq;
                    }
                }
            }
            for (; t < len; ++t) {
#pragma unroll
                for (int c = 0; c < kDitherCpl; ++c) {
                    const double yq = dSample<ORDER>(mine[c * kDitherPitch + t] * p.headroom, e[c], s[c], p);
                    mine[c * kDitherPitch + t] = p.scrub ? (fabs(yq) < 1.0e300 ? yq : 0.0) : yq;
                }
            }
        }
        __syncthreads();
        if (lane < len) {
#pragma unroll 8
            for (int r = 0; r < rows; ++r) out[(row0 + r) * outStride + t0 + lane] = tile[r * kDitherPitch + lane];
        }
        __syncthreads();                                            // the tile is free again
    }
#pragma unroll
    for (int c = 0; c < kDitherCpl; ++c) {
        const int r = lane * kDitherCpl + c;
        if (r < rows) {
#pragma unroll
            for (int k = 0; k < ORDER; ++k) err[(size_t)k * nCh + row0 + r] = e[c][k];
#pragma unroll
            for (int k = 0; k < 4; ++k) rng[(size_t)k * nCh + row0 + r] = s[c][k];
        }
    }
}

}  // namespace

bool launch_dither(hipStream_t stream, const double* in, int64_t inStride, double* out, int64_t outStride, int n, int nCh, int order,
                   const DitherParams& p, double* err, unsigned long long* rng)
{
    const dim3 grid((unsigned)((nCh + kDitherRows - 1) / kDitherRows)), block(64);
    if (order == 4) hipLaunchKernelGGL(k_dither<4>, grid, block, 0, stream, in, inStride, out, outStride, n, nCh, p, err, rng);
    else if (order == 16) hipLaunchKernelGGL(k_dither<16>, grid, block, 0, stream, in, inStride, out, outStride, n, nCh, p, err, rng);
    else return false;
    return true;
}

}  // namespace cpq
