// resample_kernels.hip -- k_ir_resample: the polyphase sample-rate converter of cpq_ir_resample over a batch of rows (a row is
// one channel of one IR, rows of any lengths), one launch per source rate.
//
// Mapping: a workgroup takes a tile of consecutive outputs of one row, a lane one output j.  The outputs of a tile read one short
// stretch of the row (tile * M / L + T samples), which is staged in LDS, kResampleChunk taps at a time, with the zero extension
// written into the stage: the inner loop has no bounds check and no branch.  Consecutive lanes read LDS addresses that advance
// by M / L doubles on average: below 1 they repeat (a broadcast), at 2 : 1 every second bank pair is used (two-way, the price
// of ds_read_b64 on a stride of 16 bytes).  Each lane walks its own coefficient row, phase (j M) mod L, from global memory: a
// row is T contiguous doubles, so a lane uses every cache line it fetches sixteen times, and the rows of a tile (at most L of
// them) stay in L1 / L2.  The other mapping, a wave per phase with its coefficients in scalar registers, reads the row at a
// stride of M samples: its stage is 64 M + T doubles a wave, which no LDS holds at M = 1280.  DESIGN.md has the comparison.
//
// Arithmetic: acc = 0, then acc = fma(taps[p][k], x[n0 + T / 2 - k], acc) for k = 0 ... T - 1 in that order, n0 = floor(j M / L),
// x zero outside the row.  The order does not depend on the tile, the chunk or the batch, and it is the host path's order.
//
// k_src_resample, k_src_keep: the device object of cpq_src (engine_src.cpp), the same mapping over the channels of a stream, call
// by call.  Every index, offset, count and stride of theirs is src_device_plan.hpp's arithmetic on SrcLaunch, which arrives by
// value: there is no table in device memory.  They read taps, hist and the caller's in, and write out and hist.
#include "kernels.hpp"

namespace cpq {

namespace {

// the stretch of the row the chunk [kc, kc + kn) needs goes to stage[0 ... span + kn - 2]: stage[s] = x[lo + s],
// lo = nBase + T / 2 - (kc + kn - 1); the lane with n0 = nBase + d reads stage[d + kn - 1 - kk] for tap kc + kk
__global__ void __launch_bounds__(kResampleTileMax) k_ir_resample(const double* __restrict__ taps, int L, int M, int T,
                                                                  const double* __restrict__ x, double* __restrict__ y,
                                                                  const ResampleRow* __restrict__ rows,
                                                                  const ResampleTile* __restrict__ tiles, int span)
{
    extern __shared__ double stage[];
    const ResampleTile tile = tiles[blockIdx.x];
    const ResampleRow row = rows[tile.row];
    const int tid = (int)threadIdx.x, nThreads = (int)blockDim.x;
    const int j = tile.j0 + tid;
    const bool live = j < row.nOut;
    const long long at = (long long)(live ? j : row.nOut - 1) * M;     // idle lanes follow the row's last output: no address is new
    const long long nBase = ((long long)tile.j0 * M) / L;
    const int d = (int)(at / L - nBase);                                // 0 ... span - 1
    const double* __restrict__ h = taps + (size_t)(at % L) * (size_t)T;
    const double* __restrict__ xr = x + row.inOff;
    const int half = T / 2;

    double acc = 0.0;
    for (int kc = 0; kc < T; kc += kResampleChunk) {
        const int kn = min(kResampleChunk, T - kc);
        const long long lo = nBase + half - (kc + kn - 1);
        for (int s = tid; s < span + kn - 1; s += nThreads) {
            const long long idx = lo + s;
            stage[s] = (idx >= 0 && idx < row.n) ? xr[idx] : 0.0;
        }
        __syncthreads();
        const double* __restrict__ hk = h + kc;
        const double* xs = stage + d + kn - 1;
#pragma unroll 8
        for (int kk = 0; kk < kn; ++kk) acc = fma(hk[kk], xs[-kk], acc);
        __syncthreads();
    }
    if (live) y[row.outOff + j] = acc;
}

static_assert(kSrcTileMax == kResampleTileMax && kSrcChunk == kResampleChunk, "cpq_src launches with k_ir_resample's geometry");

// grid (tilesPerRow, channels), a.tile lanes: lane `tid` of tile blockIdx.x computes output srcLaneOutput of channel blockIdx.y
__global__ void __launch_bounds__(kSrcTileMax) k_src_resample(const double* __restrict__ taps, const double* __restrict__ hist,
                                                              const double* __restrict__ in, double* __restrict__ out, SrcLaunch a)
{
    extern __shared__ double stage[];
    const int tid = (int)threadIdx.x, nThreads = (int)blockDim.x;
    const int tileIndex = (int)blockIdx.x, ch = (int)blockIdx.y;
    const int o = tileIndex * a.tile + tid;
    const SrcOutput at = srcOutput(a, srcLaneOutput(a, tileIndex, tid));
    const int cBase = srcTileBase(a, tileIndex);
    const int d = at.c - cBase;                                         // 0 ... span - 1
    const int kEnd = srcTapEnd(a, at.c);
    const double* __restrict__ h = taps + (size_t)at.row * (size_t)a.T;

    double acc = 0.0;
    for (int kc = 0; kc < a.T; kc += kSrcChunk) {
        const int kn = srcChunkLen(a, kc);
        const int lo = srcStageLo(cBase, kc, kn);
        for (int s = tid; s < srcStageLen(a.span, kn); s += nThreads) stage[s] = srcVirt(a, hist, in, ch, lo + s);
        __syncthreads();
        const double* __restrict__ hk = h + kc;
        const double* xs = stage + srcStageAt(d, kn, 0);
        const int mine = min(kn, kEnd - kc);                            // below kn only where the row starts inside the filter
#pragma unroll 8
        for (int kk = 0; kk < mine; ++kk) acc = fma(hk[kk], xs[-kk], acc);
        __syncthreads();
    }
    if (o < a.nOut) out[(long long)ch * a.outStride + o] = acc;
}

// one workgroup of kSrcKeepBlock lanes per channel: ascending chunks, each loaded whole before it is stored
__global__ void __launch_bounds__(kSrcKeepBlock) k_src_keep(double* hist, const double* __restrict__ in, SrcLaunch a)
{
    const int tid = (int)threadIdx.x, ch = (int)blockIdx.x;
    for (int chunk = 0; chunk < srcKeepChunks(a); ++chunk) {
        const int i = chunk * kSrcKeepBlock + tid;
        const double v = i < a.keepLen ? srcVirt(a, hist, in, ch, a.keepShift + i) : 0.0;
        __syncthreads();
        if (i < a.keepLen) hist[(long long)ch * a.hBound + i] = v;
        __syncthreads();
    }
}

}  // namespace

int resampleTile(int L, int M) { return (long long)M <= 8LL * L ? kResampleTileMax : 64; }

int resampleSpan(int L, int M, int tile) { return (int)(((long long)(tile - 1) * M) / L) + 2; }

void launch_ir_resample(hipStream_t stream, const double* taps, int L, int M, int T, const double* x, double* y, const ResampleRow* rows,
                        const ResampleTile* tiles, int nTiles)
{
    if (nTiles <= 0) return;
    const int tile = resampleTile(L, M), span = resampleSpan(L, M, tile);
    const size_t lds = (size_t)(span + kResampleChunk - 1) * sizeof(double);
    hipLaunchKernelGGL(k_ir_resample, dim3((unsigned)nTiles), dim3((unsigned)tile), lds, stream, taps, L, M, T, x, y, rows, tiles, span);
}

void launch_src_resample(hipStream_t stream, const double* taps, const double* hist, const double* in, double* out, const SrcLaunch& a)
{
    if (a.tilesPerRow <= 0 || a.channels <= 0) return;
    hipLaunchKernelGGL(k_src_resample, dim3((unsigned)a.tilesPerRow, (unsigned)a.channels), dim3((unsigned)a.tile), (size_t)srcLdsBytes(a.span),
                       stream, taps, hist, in, out, a);
}

void launch_src_keep(hipStream_t stream, double* hist, const double* in, const SrcLaunch& a)
{
    if (!srcKeepMoves(a) || a.channels <= 0) return;
    hipLaunchKernelGGL(k_src_keep, dim3((unsigned)a.channels), dim3(kSrcKeepBlock), 0, stream, hist, in, a);
}

}  // namespace cpq
