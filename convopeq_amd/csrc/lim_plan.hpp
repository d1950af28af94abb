// lim_plan.hpp -- the definition of cpq_limiter (look-ahead true-peak limiter per stereo programme) and every piece of integer
// arithmetic of its calls, stated once for the kernels (lim_kernels.hip: k_lim_apply, k_lim_keep), for engine_lim.cpp, which plans
// a call on the host and passes the plan by value, for lim_host.hpp, the host object, and for tests/sanitize/lim_plan_check.cpp,
// which restates both kernels as host loops over grid, lanes and LDS-sized heap blocks.  No HIP include: what both sides call is
// CPQ_HD.  The detector is prog_plan.hpp's Annex 2 interpolator (progPeakAt): its table and term order are used, not copied.
//
// Definition.  A stream is a stereo pair of rows.  Fixed at create: the rate (which decides the phases in use, progPeakMask), the
// ceiling c > 0 (linear) and the window W in 8 ... 1024.  M = W + 12, D = W + 11 (the latency).  g is the stream's pre-gain, set
// at the start of a programme.  x[ch][i], i >= 0, is everything received since create, reset or the last flush; it is 0.0 for
// i < 0 and, after a flush, from its end on.
//   pre-gain   u[ch][i] = scrub(x[ch][i] * g): one rounding, then progPeakScrub (not finite or |v| >= 1e300 reads as 0.0, so a
//              sample that is not finite comes out as 0.0 whatever g is, and every u is finite)
//   detector   p[i] = the largest of |u[0][i]|, |u[1][i]| and progPeakAt(&u[ch][i], phase) over both channels and the phases in use
//   required   r[i] = p[i] > c ? c / p[i] : 1.0;  r[i] = 1.0 for i < 0 (u is 0.0 there, so the rule gives it)
//   minimum    m[i] = min(r[i - M + 1 ... i]): exact in any order
//   envelope   a[i] = (m[i] + m[i - 1] + ... + m[i - W + 1]) / (double)W, summed in that order from 0.0: exactly 1.0 where
//              nothing limits
//   output     y[ch][i] = u[ch][i - D] * a[i]
// A call of n samples emits n outputs, the first D of a programme are zeros, a flush emits the last D.
//
// Why M and D.  The windows of m[i - j], j < W, all contain every k in [i - W - 11, i - W + 1].  u[i - D] enters the detector
// outputs k = i - D ... i - D + 11 = i - W - 11 ... i - W.  So a[i] is a mean of values none of which exceeds any r[k] the delayed
// sample enters.
//
// The bound on |y| (kLimBoundUlps).  Let t = 2^-53.  Every m[i - j] <= r[i - D] = rho, and a floating-point sum is monotone in
// its terms, so the W-term sum is at most W rho (1 + t)^(W - 1) and a <= rho (1 + t)^W.  rho <= (c / p)(1 + t) with
// p >= |u[i - D]| where p > c, and where p <= c, |u[i - D]| <= c already.  So |y| <= c (1 + t)^(W + 2) <= c + (W + 3) ulp(c) for
// every W <= 1024, since ulp(c) >= c t.  The true peak of y may pass c by more: a moves inside the interpolator's 12 taps.  That
// overshoot is measured, not derived.
//
// A call.  The outputs of a call read the virtual row [ history | new samples ] of u, history being the last limHalo(W) values of
// u, already scrubbed and scaled.  In the row's index v the call's output o is v = hLen + o; it reads u at v - limHalo(W) ... v.
// No index, count or offset comes from device memory: LimLaunch travels by value.  Only positions are 64-bit, and they stay on
// the host: the kernels work in the call's own indices, all below 2^31.
#pragma once

#include "prog_plan.hpp"

namespace cpq {

constexpr int kLimMinWindow = 8, kLimMaxWindow = 1024;
constexpr int kLimMaxCall = 1 << 30;                // samples of one call
constexpr int kLimThreads = 256;
constexpr int kLimTile = 1024;                      // outputs a workgroup takes
constexpr int kLimPairs = kLimTile / 2 / kLimThreads;       // pairs of adjacent outputs a lane holds
constexpr int kLimKeepBlock = 256;                  // lanes of k_lim_keep: samples one ascending chunk of the move holds in registers
constexpr int kLimLdsLimit = 64 * 1024;
static_assert(kLimPairs >= 1 && kLimPairs * 2 * kLimThreads == kLimTile, "a lane holds whole pairs");

CPQ_HD inline int limM(int W) { return W + kPeakTaps; }
CPQ_HD inline int limD(int W) { return W + kPeakHist; }
// r values in front of an output's own that its envelope reads, and u values in front of an output's own that those read
CPQ_HD inline int limReach(int W) { return limM(W) + W - 2; }
CPQ_HD inline int limHalo(int W) { return limReach(W) + kPeakHist; }
CPQ_HD inline int limBoundUlps(int W) { return W + 3; }
// the stage of a tile: slot s of a channel is u at v = lo + s, lo = hLen + tile0 - limHalo(W); r[q] is computed from slots
// q ... q + 11 and belongs to output o = q - limReach(W) of the tile; the delayed sample of output o is slot o + W + 10
CPQ_HD inline int limStageLen(int W, int tile) { return tile + limHalo(W); }
CPQ_HD inline int limStagePitch(int W, int tile) { return (limStageLen(W, tile) + 1) & ~1; }
CPQ_HD inline int limRCount(int W, int tile) { return tile + limReach(W); }
CPQ_HD inline int limDelaySlot(int W, int o) { return o + limHalo(W) - limD(W); }
CPQ_HD inline long long limLdsBytes(int W) { return 2LL * limStagePitch(W, kLimTile) * 8; }
static_assert(2LL * ((kLimTile + 2 * kLimMaxWindow + 21 + 1) & ~1) * 8 + 256 <= kLimLdsLimit, "the stage of the largest window fits LDS");

inline int limDefaultWindow(double rate)
{
    const double w = std::floor(0.0015 * rate + 0.5);
    return w < kLimMinWindow ? kLimMinWindow : w > kLimMaxWindow ? kLimMaxWindow : (int)w;
}

// ---------------------------------------------------------------------------------------------------------- the arithmetic
CPQ_HD inline double limPre(double x, double g) { return progPeakScrub(x * g); }
// w0, w1: the current sample of either channel, w[-1 ... -11] the samples before it
CPQ_HD inline double limRequired(const double* w0, const double* w1, int mask, double c)
{
    const double a0 = std::fabs(w0[0]), a1 = std::fabs(w1[0]);
    double p = a1 > a0 ? a1 : a0;
#pragma GCC unroll 4
    for (int ph = 0; ph < 4; ++ph) {
        if (!((mask >> ph) & 1)) continue;
        const double y0 = progPeakAt(w0, ph), y1 = progPeakAt(w1, ph);
        p = y0 > p ? y0 : p;
        p = y1 > p ? y1 : p;
    }
    return p > c ? c / p : 1.0;
}
// m: the newest of the W minima
CPQ_HD inline double limEnvelope(const double* m, int W)
{
    double s = 0.0;
    for (int j = 0; j < W; ++j) s = s + m[-j];
    return s / (double)W;
}
// the envelopes of two adjacent outputs, m the newest minimum of the first: m[-j] of the second is m[1 - j] of the first, so one
// read serves both sums, and either sum takes its terms in limEnvelope's order
CPQ_HD inline void limEnvelopePair(const double* m, int W, double& a0, double& a1)
{
    double s0 = 0.0, s1 = 0.0, prev = m[1];
    for (int j = 0; j < W; ++j) {
        const double cur = m[-j];
        s1 = s1 + prev;
        s0 = s0 + cur;
        prev = cur;
    }
    a0 = s0 / (double)W;
    a1 = s1 / (double)W;
}

// what a tile hands to k_lim_keep, and what a stream's telemetry holds: the smallest a and the outputs with a < 1.0
struct LimPartial { double minGain; long long limited; };
CPQ_HD inline void limFold(LimPartial& t, double minGain, long long limited)
{
    t.minGain = minGain < t.minGain ? minGain : t.minGain;
    t.limited = t.limited + limited;
}

// ------------------------------------------------------------------------------------------------------------------ a call
struct LimState {
    long long pos = 0;      // samples the programme has received
    int hLen = 0;           // history extent: min(pos, limHalo(W))
};
struct LimCall {
    long long i0 = 0, i1 = 0;       // outputs of the programme the call emits
    long long base = 0;             // the programme's sample at v = 0 of the virtual row
    int nIn = 0, nOut = 0;
    int hLen = 0;                   // history extent before the call
    int hKeep = 0;                  // history extent after it: the last hKeep values of the virtual row
    bool first = false;             // the programme's first call: the telemetry starts over
    LimState next;
};
// n: the samples of the call (1 ... kLimMaxCall); a flush takes none and emits the last D outputs
inline LimCall limPlan(int W, const LimState& s, int n, bool flush)
{
    LimCall c;
    c.nIn = flush ? 0 : n;
    c.nOut = flush ? limD(W) : n;
    c.i0 = s.pos; c.i1 = s.pos + c.nOut;
    c.hLen = s.hLen;
    c.base = s.pos - s.hLen;
    c.first = s.pos == 0;
    const long long have = (long long)s.hLen + c.nIn;
    c.hKeep = flush ? 0 : (int)(have < limHalo(W) ? have : limHalo(W));
    c.next.pos = flush ? 0 : s.pos + n;
    c.next.hLen = c.hKeep;
    return c;
}

struct LimLaunch {
    int W = 0, mask = 0;
    double c = 1.0;
    int nOut = 0;                       // outputs per row
    int hLen = 0, nVirt = 0;            // the virtual row: hist[0 ... hLen) then the pre-gained in[0 ... nVirt - hLen)
    int hBound = 0;                     // doubles between the rows of hist
    int tilesPerRow = 0, streams = 0;   // the grid: (tilesPerRow, streams)
    int partStride = 0;                 // partials between the streams of part
    int keepShift = 0, keepLen = 0;     // keep step: hist[row][i] = virt(keepShift + i) for i < keepLen
    int first = 0;                      // the telemetry starts over with this call
    int wide = 0;                       // both strides even and both buffers 16-byte aligned: rows move two samples at a time
    long long inStride = 0, outStride = 0;
};
inline LimLaunch limLaunch(int W, int mask, double c, const LimCall& call, int streams, long long inStride, long long outStride, int partStride)
{
    LimLaunch a;
    a.W = W; a.mask = mask; a.c = c;
    a.nOut = call.nOut;
    a.hLen = call.hLen; a.nVirt = call.hLen + call.nIn;
    a.hBound = limHalo(W);
    a.tilesPerRow = (call.nOut + kLimTile - 1) / kLimTile;
    a.streams = streams;
    a.partStride = partStride;
    a.keepShift = a.nVirt - call.hKeep; a.keepLen = call.hKeep;
    a.first = call.first ? 1 : 0;
    a.wide = inStride % 2 == 0 && outStride % 2 == 0;
    a.inStride = inStride; a.outStride = outStride;
    return a;
}
CPQ_HD inline int limStageLo(const LimLaunch& a, int tileIndex) { return a.hLen + tileIndex * kLimTile - limHalo(a.W); }

// the virtual row of `row` (2 stream + channel) at v: history, then the call's samples with pre-gain and scrub, 0.0 on either side
CPQ_HD inline double limVirt(const LimLaunch& a, const double* hist, const double* in, double g, int row, int v)
{
    if (v < 0 || v >= a.nVirt) return 0.0;
    if (v < a.hLen) return hist[(long long)row * a.hBound + v];
    return limPre(in[(long long)row * a.inStride + (v - a.hLen)], g);
}
// Staging by pairs: pair j of a tile covers the call's samples e = limPairFirst + 2 j and e + 1 (e even, so the pair is one
// 16-byte access of a wide row), which are slots e - (lo - hLen) and the next.  Whole inside [0, nIn): one access; else each
// slot that lies in the stage goes through limVirt.
CPQ_HD inline int limPairFirst(int lo, int hLen) { const int e = lo - hLen; return e & ~1; }
CPQ_HD inline int limPairCount(int W) { return limStageLen(W, kLimTile) / 2 + 1; }

// The keep step moves virt[nVirt - hKeep ... nVirt) to hist[row][0 ... hKeep).  A slot i is read from hist[keepShift + i] or from
// in, so the destination index never exceeds the source index: ascending chunks of kLimKeepBlock samples, each loaded whole before
// it is stored, read no slot an earlier chunk has written.  Nothing moves at a flush (hKeep = 0).
CPQ_HD inline bool limKeepMoves(const LimLaunch& a) { return a.keepLen > 0 && (a.keepShift > 0 || a.nVirt > a.hLen); }
CPQ_HD inline int limKeepChunks(const LimLaunch& a) { return limKeepMoves(a) ? (a.keepLen + kLimKeepBlock - 1) / kLimKeepBlock : 0; }

}  // namespace cpq
