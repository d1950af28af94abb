// dither_kernels.hip -- the dither stage on gfx950: FixedNoiseShaper / Fixed15TapNoiseShaper / LatticeNoiseShaper::processStereoBlock
// of the reference (src/FixedNoiseShaper.h:162-184, 272-297; src/Fixed15TapNoiseShaper.h:204-230, 318-342;
// src/LatticeNoiseShaper.h:73-111, 203-293) on rows [channel][sample].
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
//
// k_dither_lattice is the adaptive 9th-order shaper on the same tile: the stored error runs through nine lattice stages, each
// depending on the one before, and the coefficients belong to the stream, so a lane loads its channel's nine from coef [9][nCh]
// once and keeps them beside the nine states and the generator words (22 doubles a channel).  The feedback sum holds the file's
// only fused multiply-adds, the four computeFeedback writes as _mm256_fmadd_pd; the file is built with -ffp-contract=off, so
// nothing else fuses.  processStereoBlock's closing clampStateSIMD (+-1e12) cannot act on states advanceState already holds to
// +-2 and is not built.
#include "kernels.hpp"
#include "dither_device.hpp"

namespace cpq {
namespace {

// the tile of dither_device.hpp back to the rows it came from: lane = sample
__device__ __forceinline__ void dTileStore(const double* tile, double* out, int64_t outStride, int row0, int rows, int t0, int len, int lane)
{
    if (lane < len) {
#pragma unroll 8
        for (int r = 0; r < rows; ++r) out[(row0 + r) * outStride + t0 + lane] = tile[r * kDitherPitch + lane];
    }
}

__device__ __forceinline__ double dScrub(double yq, int scrub) { return scrub ? (fabs(yq) < 1.0e300 ? yq : 0.0) : yq; }

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
        dTileLoad(tile, in, inStride, row0, rows, t0, len, lane);
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
                        mine[c * kDitherPitch + t + k] = dScrub(yq, p.scrub);
                    }
                }
            }
            for (; t < len; ++t) {
#pragma unroll
                for (int c = 0; c < kDitherCpl; ++c) {
                    const double yq = dSample<ORDER>(mine[c * kDitherPitch + t] * p.headroom, e[c], s[c], p);
                    mine[c * kDitherPitch + t] = dScrub(yq, p.scrub);
                }
            }
        }
        __syncthreads();
        dTileStore(tile, out, outStride, row0, rows, t0, len, lane);
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

// grid and rows as k_dither.  coef [kLatticeOrder][nCh]; the states are err's rows 0 .. kLatticeOrder - 1
__global__ void __launch_bounds__(64)
k_dither_lattice(const double* in, int64_t inStride, double* out, int64_t outStride, int n, int nCh, DitherParams p,
                 const double* __restrict__ coef, double* __restrict__ err, unsigned long long* __restrict__ rng)
{
    __shared__ double tile[kDitherRows * kDitherPitch];
    const int lane = threadIdx.x;
    const int row0 = blockIdx.x * kDitherRows;
    const int rows = min(kDitherRows, nCh - row0);                  // >= 1
    double st[kDitherCpl][kLatticeOrder], c[kDitherCpl][kLatticeOrder];
    unsigned long long s[kDitherCpl][4];
#pragma unroll
    for (int ch = 0; ch < kDitherCpl; ++ch) {
        const int r = lane * kDitherCpl + ch;
        const bool live = r < rows;
#pragma unroll
        for (int k = 0; k < kLatticeOrder; ++k) {
            st[ch][k] = live ? err[(size_t)k * nCh + row0 + r] : 0.0;
            c[ch][k] = live ? coef[(size_t)k * nCh + row0 + r] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s[ch][k] = live ? rng[(size_t)k * nCh + row0 + r] : 1ull;
    }
    for (int t0 = 0; t0 < n; t0 += kDitherStep) {
        const int len = min(kDitherStep, n - t0);
        dTileLoad(tile, in, inStride, row0, rows, t0, len, lane);
        __syncthreads();
        double* mine = tile + lane * kDitherCpl * kDitherPitch;
        if (lane * kDitherCpl < rows) {
            for (int t = 0; t < len; ++t) {
#pragma unroll
                for (int ch = 0; ch < kDitherCpl; ++ch) {
                    const double yq = dLatticeSample(mine[ch * kDitherPitch + t] * p.headroom, st[ch], c[ch], s[ch], p);
                    mine[ch * kDitherPitch + t] = dScrub(yq, p.scrub);
                }
            }
        }
        __syncthreads();
        dTileStore(tile, out, outStride, row0, rows, t0, len, lane);
        __syncthreads();                                            // the tile is free again
    }
#pragma unroll
    for (int ch = 0; ch < kDitherCpl; ++ch) {
        const int r = lane * kDitherCpl + ch;
        if (r < rows) {
#pragma unroll
            for (int k = 0; k < kLatticeOrder; ++k) err[(size_t)k * nCh + row0 + r] = st[ch][k];
#pragma unroll
            for (int k = 0; k < 4; ++k) rng[(size_t)k * nCh + row0 + r] = s[ch][k];
        }
    }
}

}  // namespace

bool launch_dither(hipStream_t stream, const double* in, int64_t inStride, double* out, int64_t outStride, int n, int nCh, int order,
                   const DitherParams& p, const double* coef, double* err, unsigned long long* rng)
{
    const dim3 grid((unsigned)((nCh + kDitherRows - 1) / kDitherRows)), block(64);
    if (order == 4) hipLaunchKernelGGL(k_dither<4>, grid, block, 0, stream, in, inStride, out, outStride, n, nCh, p, err, rng);
    else if (order == 16) hipLaunchKernelGGL(k_dither<16>, grid, block, 0, stream, in, inStride, out, outStride, n, nCh, p, err, rng);
    else if (order == kLatticeOrder && coef)
        hipLaunchKernelGGL(k_dither_lattice, grid, block, 0, stream, in, inStride, out, outStride, n, nCh, p, coef, err, rng);
    else return false;
    return true;
}

}  // namespace cpq
