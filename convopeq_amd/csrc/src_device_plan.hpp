// src_device_plan.hpp -- everything about a launch of the device object of cpq_src that is integer arithmetic, stated once for
// the kernels (resample_kernels.hip: k_src_resample, k_src_keep), for engine_src.cpp, which fills SrcLaunch from the plan of a
// call (src_plan.hpp), and for tests/sanitize/src_device_check.cpp, which restates the kernels as host loops over grid, lanes and
// chunks on exactly sized heap blocks.  No HIP include: what both sides call is CPQ_HD, __host__ __device__ under hipcc.
//
// The mapping is k_ir_resample's: a workgroup takes a tile of consecutive outputs of one channel, a lane one output, the stretch
// of the channel's virtual row [ history | new samples ] the tile reads is staged kSrcChunk taps at a time with the zero
// extension written into the stage.  The tile and span formulas are resampleTile's and resampleSpan's (kernels.hpp); the two
// kernels are unified later, not here.
//
// No number below comes from device memory.  SrcLaunch travels by value in the kernel arguments; the kernels read taps, hist
// and the caller's in, and write out and hist, nothing else.
#pragma once

#include "src_plan.hpp"

#if defined(__HIPCC__)
#define CPQ_HD __host__ __device__
#else
#define CPQ_HD
#endif

namespace cpq {

constexpr int kSrcTileMax = 256;        // outputs a workgroup takes while M <= 8 L; 64 beyond, so that the stage fits LDS
constexpr int kSrcChunk = 256;          // taps a workgroup stages the row for at a time
constexpr int kSrcKeepBlock = 256;      // lanes of k_src_keep: samples one ascending chunk of the move holds in registers
constexpr int kSrcLdsLimit = 64 * 1024;

struct SrcLaunch {
    int L = 1, M = 1, T = 0;
    int c0 = 0, phase = 0;              // centre (index into the virtual row) and coefficient row of the call's output 0
    int nOut = 0;                       // outputs per channel
    int hLen = 0, nVirt = 0;            // the virtual row: hist[0 ... hLen) then in[0 ... nVirt - hLen)
    int hBound = 0;                     // doubles between the channels of hist
    int tile = 0, span = 0;
    int tilesPerRow = 0, channels = 0;  // the grid: (tilesPerRow, channels)
    int keepShift = 0, keepLen = 0;     // keep step: hist[ch][i] = virt(keepShift + i) for i < keepLen
    long long inStride = 0, outStride = 0;
};

CPQ_HD inline int srcTile(int L, int M) { return (long long)M <= 8LL * L ? kSrcTileMax : 64; }
// input samples the centres of a tile's outputs spread over: d of srcOutput lies in 0 ... span - 1
CPQ_HD inline int srcSpan(int L, int M, int tile) { return (int)(((long long)(tile - 1) * M) / L) + 2; }
CPQ_HD inline int srcStageLen(int span, int kn) { return span + kn - 1; }
CPQ_HD inline long long srcLdsBytes(int span) { return (long long)srcStageLen(span, kSrcChunk) * 8; }

// output o of the call (o < 2^30): p = phase + o M, centre c0 + p / L, coefficient row p mod L
struct SrcOutput { int c, row; };
CPQ_HD inline SrcOutput srcOutput(const SrcLaunch& a, int o)
{
    const long long p = a.phase + (long long)o * a.M;
    return SrcOutput{ a.c0 + (int)(p / a.L), (int)(p % a.L) };
}
// the centre of the tile's first output: a lane's d is its centre minus this
CPQ_HD inline int srcTileBase(const SrcLaunch& a, int tileIndex) { return srcOutput(a, tileIndex * a.tile).c; }
// the output a lane computes: idle lanes of the last tile follow the row's last output, so that no lane forms an address that a
// live lane does not
CPQ_HD inline int srcLaneOutput(const SrcLaunch& a, int tileIndex, int lane)
{
    const int o = tileIndex * a.tile + lane;
    return o < a.nOut ? o : a.nOut - 1;
}
// taps of an output that lie at or above v = 0: k = 0 ... min(T, c + 1) - 1.  Below v = 0 is the time before the stream's start;
// src_plan.hpp passes those terms over, and so does the lane, by its trip count: they come last in the sum, and
// fma(h, 0.0, acc) turns an acc of -0.0 (a sum of denormals that underflowed) into +0.0 where h > 0.  The zeros above the row
// (a flush) come first, onto an acc of +0.0, which they leave as it is: they are computed from the stage's zero extension.
CPQ_HD inline int srcTapEnd(const SrcLaunch& a, int c) { return c + 1 < a.T ? (c + 1 > 0 ? c + 1 : 0) : a.T; }

// chunk [kc, kc + kn) of the taps: stage[s] = virt(srcStageLo + s) for s < srcStageLen(span, kn); the lane with centre
// cBase + d reads stage[d + kn - 1 - kk] for tap kc + kk
CPQ_HD inline int srcChunkLen(const SrcLaunch& a, int kc) { return a.T - kc < kSrcChunk ? a.T - kc : kSrcChunk; }
CPQ_HD inline int srcStageLo(int cBase, int kc, int kn) { return cBase - (kc + kn - 1); }
CPQ_HD inline int srcStageAt(int d, int kn, int kk) { return d + kn - 1 - kk; }

// the virtual row of channel ch at v: history, then the call's samples, zero on either side
CPQ_HD inline double srcVirt(const SrcLaunch& a, const double* hist, const double* in, int ch, int v)
{
    if (v < 0 || v >= a.nVirt) return 0.0;
    if (v < a.hLen) return hist[(long long)ch * a.hBound + v];
    return in[(long long)ch * a.inStride + (v - a.hLen)];
}

// The keep step moves virt[nVirt - hKeep ... nVirt) to hist[ch][0 ... hKeep).  A slot i is read from hist[keepShift + i] or from
// in, so the destination index never exceeds the source index: chunks of kSrcKeepBlock samples in ascending order, each loaded
// whole before it is stored, read no slot an earlier chunk has written.  Nothing moves at a flush (hKeep = 0) and in a call of
// no samples that keeps all it had.
CPQ_HD inline bool srcKeepMoves(const SrcLaunch& a) { return a.keepLen > 0 && (a.keepShift > 0 || a.nVirt > a.hLen); }
CPQ_HD inline int srcKeepChunks(const SrcLaunch& a) { return (a.keepLen + kSrcKeepBlock - 1) / kSrcKeepBlock; }

// the launch of a planned call: hLen is the history extent before it, strides in doubles
inline SrcLaunch srcLaunch(const SrcGeometry& g, const SrcCall& call, int hLen, int nIn, int nChannels, long long inStride,
                           long long outStride)
{
    SrcLaunch a;
    a.L = g.L; a.M = g.M; a.T = g.T;
    a.c0 = call.c0; a.phase = call.phase;
    a.nOut = (int)(call.j1 - call.j0);
    a.hLen = hLen; a.nVirt = hLen + nIn;
    a.hBound = srcHistoryBound(g);
    a.tile = srcTile(g.L, g.M);
    a.span = srcSpan(g.L, g.M, a.tile);
    a.tilesPerRow = (a.nOut + a.tile - 1) / a.tile;
    a.channels = nChannels;
    a.keepShift = a.nVirt - call.hKeep; a.keepLen = call.hKeep;
    a.inStride = inStride; a.outStride = outStride;
    return a;
}

}  // namespace cpq
