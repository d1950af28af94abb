// prog_plan.hpp -- the definition of cpq_loudness (gated programme loudness, EBU R 128) and every piece of integer arithmetic of
// its calls, stated once for the kernels (prog_kernels.hip: k_prog_hops, k_prog_finish), for engine_prog.cpp, which plans a call
// on the host and passes the plan by value, and for tests/sanitize/prog_plan_check.cpp, which restates both kernels as host loops
// over grid, waves and lanes on exactly sized heap blocks.  No HIP include: what both sides call is CPQ_HD.  The true peak per
// programme, the gain under a ceiling and its application (k_prog_peak, k_prog_apply; tests/sanitize/prog_peak_check.cpp) are
// defined at the end of the file.
//
// Definition.  A stream is a stereo pair of rows.  Every sample is scrubbed as the meters scrub it (not finite or |v| >= 1e300
// reads as 0) and K-weighted with cpq_meter_kweighting(rate): two Direct-Form-I biquads per channel, state carried over calls.
//   hop          H = rate / 10 samples (rate a whole number of Hz in 8000 ... 768000, divisible by 10).  Hop h of a stream is
//                E[h] = sum yL^2 + sum yR^2 over samples h H ... (h + 1) H - 1, counted from create / reset: the grid is the
//                stream's, not a call's.  Only complete hops count (n_hops = samples / H).
//   blocks       momentary  b >= 3:  z = (E[b-3] + E[b-2] + E[b-1] + E[b]) / (4 H), added left to right
//                short-term b >= 29: the same over 30 hops and 30 H
//   loudness     L(z) = -0.691 + 10 log10(z)
//   gates        are decided on mean squares, which is the same decision without a logarithm in it:
//                L > -70 is z > zAbs = 10^((-70 + 0.691) / 10);  L > L(m) - 10 is z > 0.1 m;  L > L(m) - 20 is z > 0.01 m
//   integrated   (BS.1770-4) m1 = mean of the momentary z > zAbs; relative_gate = L(m1) - 10; integrated = L(mean of the momentary
//                z > zAbs and z > 0.1 m1)
//   range        (EBU Tech 3342) the short-term blocks b = 29, 39, ... (a 1 s step); mS = mean of those with z > zAbs; kept: z > zAbs
//                and z > 0.01 mS; sorted ascending, n of them: LRA = L(z[i95]) - L(z[i10]) with i_p = round(p (n - 1)), the rounding
//                half up and in integers: i95 = (95 (n - 1) + 50) / 100, i10 = (10 (n - 1) + 50) / 100
//   maxima       the largest momentary and the largest short-term loudness over all hops
//   empty        an empty set gives -HUGE_VAL for its loudness and 0 for the range; the counts of every stage are in the result
// Means are lane sums (lane t of kProgFinishLanes takes every kProgFinishLanes-th block, in ascending order) reduced by the tree
// of progTreeStep: a fixed order.  The kernel delivers mean squares and counts (ProgRecord); the logarithms are taken on the
// host by progResult, so that a loudness is reproducible to the bit from its mean square with the host's log10.
//
// A call.  No index, count or offset comes from device memory: ProgCall and ProgFinish travel by value.  k_prog_hops reads the
// caller's rows, the section tables, the filter state and the per-channel partial hop sums, and writes the last two and hops.
#pragma once

#include "convopeq_mi355x.h"

#include <cmath>
#include <cstdint>

#if !defined(CPQ_HD)
#if defined(__HIPCC__)
#define CPQ_HD __host__ __device__
#else
#define CPQ_HD
#endif
#endif

namespace cpq {

constexpr int kProgChunk = 8;                       // samples a lane of the K-weighting scan holds (kMeterChunk: the same tables)
constexpr int kProgLanes = 256;                     // lanes of one channel: four waves
constexpr int kProgSpan = kProgLanes * kProgChunk;  // samples of a channel a workgroup K-weights at a time
constexpr int kProgThreads = 2 * kProgLanes;        // a workgroup is a stream: waves 0-3 its left row, waves 4-7 its right row
constexpr int kProgMinHop = 800;                    // rate >= 8000
constexpr int kProgSegs = 4;                        // hops a span overlaps at most: one per wave of a channel
static_assert((kProgSpan - 2) / kProgMinHop + 2 <= kProgSegs, "a span's hops are dealt one to a wave");
constexpr int kProgBufDoubles = kProgSpan + kProgSpan / 8 + 8;     // a span in LDS, padded one double in eight
constexpr int kProgFinishLanes = 256;
constexpr int kProgSortMax = 8192;                  // short-term blocks at the 1 s step the bitonic sort holds
constexpr int kProgMaxCall = 1 << 30;               // samples of one call

CPQ_HD inline int progPad(int i) { return i + (i >> 3); }

// whole Hz in 8000 ... 768000, divisible by 10: the hop, else 0
inline int progHop(double rate)
{
    if (!(rate >= 8000.0) || !(rate <= 768000.0) || rate != std::floor(rate)) return 0;
    const int r = (int)rate;
    return r % 10 == 0 ? r / 10 : 0;
}
// hops of max_seconds (0: not a valid length)
inline long long progMaxHops(double maxSeconds)
{
    if (!(maxSeconds > 0.0) || !(maxSeconds <= 1.0e7)) return 0;
    return (long long)std::ceil(maxSeconds * 10.0);
}
// short-term blocks at the 1 s step among nHops hops: b = 29, 39, ... < nHops
CPQ_HD inline int progShortCount(long long nHops) { return nHops >= 30 ? (int)((nHops - 30) / 10) + 1 : 0; }

// ---------------------------------------------------------------------------------------------------------------- a call
struct ProgCall {
    int n = 0;              // samples per row
    int H = 0;
    int fill0 = 0;          // samples of hop h0 that earlier calls summed (the partial hop carried in)
    int h0 = 0, h1 = 0;     // first and last hop the call touches
    int fillOut = 0;        // samples of the partial hop carried out (0: the call ends on the grid)
    int maxHops = 0;        // doubles between the streams of hops
    int streams = 0;        // the grid
    long long stride = 0;   // doubles between rows
};

// pos: samples the stream took before the call.  false: the call would pass maxHops (pos + n > maxHops H); nothing is planned
inline bool progPlan(long long pos, int n, int H, int maxHops, int streams, long long stride, ProgCall& c)
{
    if (n < 1 || pos + n > (long long)maxHops * H) return false;
    c.n = n; c.H = H;
    c.fill0 = (int)(pos % H);
    c.h0 = (int)(pos / H);
    c.h1 = (int)((pos + n - 1) / H);
    c.fillOut = (int)((pos + n) % H);
    c.maxHops = maxHops; c.streams = streams; c.stride = stride;
    return true;
}
CPQ_HD inline int progSpans(const ProgCall& c) { return (c.n + kProgSpan - 1) / kProgSpan; }
CPQ_HD inline int progSpanLen(const ProgCall& c, int s0) { return c.n - s0 < kProgSpan ? c.n - s0 : kProgSpan; }
// the hop that holds sample i of the call, and where hop k begins in the call's samples (negative: before the call)
CPQ_HD inline int progHopAt(const ProgCall& c, int i) { return c.h0 + (int)(((long long)i + c.fill0) / c.H); }
CPQ_HD inline int progHopBegin(const ProgCall& c, int k) { return (int)((long long)(k - c.h0) * c.H - c.fill0); }
// hop k inside the span [s0, s0 + len): its samples [a, b) of the call, whether it began before the span, whether it ends in it
struct ProgSeg { int a, b; bool carried, complete; };
CPQ_HD inline ProgSeg progSeg(const ProgCall& c, int k, int s0, int len)
{
    const int g = progHopBegin(c, k), e = s0 + len;
    const long long end = (long long)g + c.H;
    return ProgSeg{ g > s0 ? g : s0, end < e ? (int)end : e, g < s0, end <= e };
}

// ------------------------------------------------------------------------------------------------------------ the finish
struct ProgFinish {
    int nHops = 0, H = 0, maxHops = 0;
    double zAbs = 0.0;
};
inline double progAbsGate() { return std::pow(10.0, (-70.0 + 0.691) / 10.0); }

// what k_prog_finish writes per stream: mean squares and counts; progResult takes the logarithms
struct ProgRecord {
    double zInt, zGate, zMomMax, zShortMax, zLo, zHi;   // means past both gates / past the absolute gate, maxima, LRA's two picks
    int nAbs, nRel, nShortAbs, nShortKept;
};

CPQ_HD inline double progBlock(const double* E, int b, int w, int H)
{
    double s = E[b - w + 1];
    for (int i = b - w + 2; i <= b; ++i) s = s + E[i];
    return s / (double)(w * H);
}

struct ProgAcc { double sum; int cnt; double mx; };
// lane's share of the blocks b = first + step j, j = lane, lane + kProgFinishLanes, ... while b < nHops: sum and count of the
// z > lo and z > lo2, the largest z of all
CPQ_HD inline ProgAcc progLaneGate(const double* E, const ProgFinish& f, int w, int first, int step, int lane, double lo, double lo2)
{
    ProgAcc a{ 0.0, 0, 0.0 };
    for (long long b = first + (long long)step * lane; b < f.nHops; b += (long long)step * kProgFinishLanes) {
        const double z = progBlock(E, (int)b, w, f.H);
        if (z > lo && z > lo2) { a.sum = a.sum + z; a.cnt = a.cnt + 1; }
        a.mx = z > a.mx ? z : a.mx;
    }
    return a;
}
// one step of the tree over kProgFinishLanes slots: slot i takes slot i + stride, for i < stride, stride = 128, 64, ... 1
CPQ_HD inline void progTreeStep(double* sum, int* cnt, double* mx, int i, int stride)
{
    sum[i] = sum[i] + sum[i + stride];
    cnt[i] = cnt[i] + cnt[i + stride];
    mx[i] = mx[i + stride] > mx[i] ? mx[i + stride] : mx[i];
}
CPQ_HD inline double progMean(const ProgAcc& a) { return a.cnt ? a.sum / (double)a.cnt : 0.0; }
// candidate j of the range: z of block 29 + 10 j where it is kept, else HUGE_VAL (which sorts behind every kept value)
CPQ_HD inline double progShortKept(const double* E, const ProgFinish& f, int j, double meanShort)
{
    const double z = progBlock(E, 29 + 10 * j, 30, f.H);
    return z > f.zAbs && z > 0.01 * meanShort ? z : HUGE_VAL;
}
CPQ_HD inline int progSortSize(int nCand) { int p = 2; while (p < nCand) p <<= 1; return p; }
// bitonic network, ascending: in pass (k, j) slot i and its partner l = i ^ j (handled by the lower of the two) swap when out of order
CPQ_HD inline void progSortStep(double* v, int i, int j, int k)
{
    const int l = i ^ j;
    if (l > i) {
        const double a = v[i], b = v[l];
        if (((i & k) == 0) ? a > b : a < b) { v[i] = b; v[l] = a; }
    }
}
CPQ_HD inline int progPick95(int n) { return (95 * (n - 1) + 50) / 100; }
CPQ_HD inline int progPick10(int n) { return (10 * (n - 1) + 50) / 100; }

inline double progLoudness(double z) { return -0.691 + 10.0 * std::log10(z); }

inline cpq_loudness_result progResult(const ProgRecord& r, long long nHops)
{
    cpq_loudness_result o{};
    o.n_hops = nHops;
    o.n_blocks = nHops >= 4 ? (int32_t)(nHops - 3) : 0;
    o.n_abs = r.nAbs; o.n_rel = r.nRel; o.n_short_kept = r.nShortKept;
    o.integrated = r.nRel ? progLoudness(r.zInt) : -HUGE_VAL;
    o.relative_gate = r.nAbs ? progLoudness(r.zGate) - 10.0 : -HUGE_VAL;
    o.momentary_max = o.n_blocks ? progLoudness(r.zMomMax) : -HUGE_VAL;
    o.short_term_max = nHops >= 30 ? progLoudness(r.zShortMax) : -HUGE_VAL;
    o.range = r.nShortKept ? progLoudness(r.zHi) - progLoudness(r.zLo) : 0.0;
    return o;
}

// k_prog_finish on the host: the same lanes, tree and network, one after the other.  E: a stream's nHops hop sums
inline ProgRecord progFinishHost(const double* E, const ProgFinish& f)
{
    double sum[kProgFinishLanes], mx[kProgFinishLanes];
    int cnt[kProgFinishLanes];
    auto reduce = [&](int w, int first, int step, double lo, double lo2) {
        for (int t = 0; t < kProgFinishLanes; ++t) {
            const ProgAcc a = progLaneGate(E, f, w, first, step, t, lo, lo2);
            sum[t] = a.sum; cnt[t] = a.cnt; mx[t] = a.mx;
        }
        for (int s = kProgFinishLanes / 2; s >= 1; s >>= 1)
            for (int i = 0; i < s; ++i) progTreeStep(sum, cnt, mx, i, s);
        return ProgAcc{ sum[0], cnt[0], mx[0] };
    };
    ProgRecord r{};
    const ProgAcc abs = reduce(4, 3, 1, f.zAbs, -HUGE_VAL);
    const ProgAcc rel = reduce(4, 3, 1, f.zAbs, 0.1 * progMean(abs));
    const ProgAcc sMax = reduce(30, 29, 1, HUGE_VAL, HUGE_VAL);
    const ProgAcc sAbs = reduce(30, 29, 10, f.zAbs, -HUGE_VAL);
    r.zGate = progMean(abs); r.nAbs = abs.cnt; r.zMomMax = abs.mx;
    r.zInt = progMean(rel); r.nRel = rel.cnt;
    r.zShortMax = sMax.mx; r.nShortAbs = sAbs.cnt;
    const int nCand = progShortCount(f.nHops), P = progSortSize(nCand);
    double* v = new double[(size_t)P];
    int kept = 0;
    for (int j = 0; j < P; ++j) {
        v[j] = j < nCand ? progShortKept(E, f, j, progMean(sAbs)) : HUGE_VAL;
        kept += j < nCand && v[j] < HUGE_VAL;
    }
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1)
            for (int i = 0; i < P; ++i) progSortStep(v, i, j, k);
    r.nShortKept = kept;
    r.zLo = kept ? v[progPick10(kept)] : 0.0;
    r.zHi = kept ? v[progPick95(kept)] : 0.0;
    delete[] v;
    return r;
}

// ------------------------------------------------------------------------------------------------- true peak per programme
// ITU-R BS.1770-4 Annex 2: the 48-tap, 4-phase interpolator, every coefficient an integer over 8192 (exact in binary).  Phases 2
// and 3 are phases 1 and 0 reversed.  Per channel, for sample i of the programme (counted from create / reset) and phase p:
//     y = c[p][0] x[i];  y = y + c[p][k] x[i - k]  for k = 1 ... 11 in that order, the multiply and the add rounding separately
// with x scrubbed as above and x[j] = 0 for j < 0.  true_peak = max |y| over i and the phases in use, sample_peak = max |x|: both
// linear.  A maximum does not depend on order, so the result is defined to the bit.  Phases by rate: all four below 88200 Hz;
// 0 and 2 (the same low-pass at offsets 0 and 1 / 2) from 88200 Hz to below 176400 Hz; none from 176400 Hz, where true_peak is
// sample_peak.  State per channel (kPeakState doubles): the last 11 scrubbed samples, oldest first, then the two maxima.
constexpr int kPeakTaps = 12;
constexpr int kPeakHist = kPeakTaps - 1;
constexpr int kPeakThreads = 512;                   // a workgroup is a row
constexpr int kPeakPer = 8;                         // outputs a lane holds
constexpr int kPeakTile = kPeakThreads * kPeakPer;  // samples of a row staged in LDS at a time, behind a halo of kPeakHist
constexpr int kPeakWindow = kPeakPer + kPeakHist;   // inputs of a lane's outputs
constexpr int kPeakState = 16;                      // doubles per row: [0, 11) history, [11] true peak, [12] sample peak
constexpr int kPeakTp = kPeakHist, kPeakSp = kPeakHist + 1;
CPQ_HD inline int progPeakPad(int j) { return j + (j >> 3); }       // a lane's window begins 9 doubles behind its neighbour's
constexpr int kPeakBufDoubles = kPeakHist + kPeakTile + (kPeakHist + kPeakTile - 1) / 8;

CPQ_HD inline double progPeakCoef(int p, int k)
{
    constexpr double c[2][kPeakTaps] = {
        { 14.0 / 8192.0, 90.0 / 8192.0, -161.0 / 8192.0, 272.0 / 8192.0, -487.0 / 8192.0, 1125.0 / 8192.0,
          7964.0 / 8192.0, -838.0 / 8192.0, 390.0 / 8192.0, -218.0 / 8192.0, 122.0 / 8192.0, -68.0 / 8192.0 },
        { -239.0 / 8192.0, 240.0 / 8192.0, -424.0 / 8192.0, 730.0 / 8192.0, -1364.0 / 8192.0, 3810.0 / 8192.0,
          6388.0 / 8192.0, -1641.0 / 8192.0, 832.0 / 8192.0, -477.0 / 8192.0, 271.0 / 8192.0, -155.0 / 8192.0 } };
    return p < 2 ? c[p][k] : c[3 - p][kPeakTaps - 1 - k];
}
// bit p: phase p is in use
inline int progPeakMask(double rate) { return rate < 88200.0 ? 0xF : rate < 176400.0 ? 0x5 : 0; }
CPQ_HD inline double progPeakScrub(double v) { return std::fabs(v) < 1.0e300 ? v : 0.0; }
// |y| of phase p at the sample whose scrubbed value is w[0], w[-1 ... -11] the samples before it
CPQ_HD inline double progPeakAt(const double* w, int p)
{
    double y = progPeakCoef(p, 0) * w[0];
#pragma GCC unroll 12
    for (int k = 1; k < kPeakTaps; ++k) y = y + progPeakCoef(p, k) * w[-k];
    return std::fabs(y);
}

struct PeakCall {
    int n = 0;              // samples per row
    int mask = 0;           // phases in use
    int rows = 0;           // the grid
    long long stride = 0;   // doubles between rows
};
CPQ_HD inline int progPeakTileLen(const PeakCall& c, int s0) { return c.n - s0 < kPeakTile ? c.n - s0 : kPeakTile; }
// a lane's share of a tile: w[m] = the tile's buffer at 8 lane + m (the halo in front: output o reads w[o ... o + 11]); the first
// `valid` of its outputs are samples of the call.  tp and sp: the lane's maxima, carried over tiles
CPQ_HD inline void progPeakLane(const double w[kPeakWindow], int valid, int mask, double& tp, double& sp)
{
#pragma GCC unroll 8
    for (int o = 0; o < kPeakPer; ++o)
        if (o < valid) { const double a = std::fabs(w[kPeakHist + o]); sp = a > sp ? a : sp; }
#pragma GCC unroll 4
    for (int p = 0; p < 4; ++p) {
        if (!((mask >> p) & 1)) continue;
#pragma GCC unroll 8
        for (int o = 0; o < kPeakPer; ++o) {
            const double a = progPeakAt(w + kPeakHist + o, p);
            if (o < valid) tp = a > tp ? a : tp;
        }
    }
}
// one row of one call in a sequential pass: st is the row's kPeakState doubles
inline void progPeakRowHost(const double* x, long long n, int mask, double* st)
{
    double w[kPeakTaps];                            // w[11] the current sample, w[0 ... 10] the history
    for (int j = 0; j < kPeakHist; ++j) w[j] = st[j];
    double tp = 0.0, sp = 0.0;
    for (long long i = 0; i < n; ++i) {
        w[kPeakHist] = progPeakScrub(x[i]);
        const double a = std::fabs(w[kPeakHist]);
        sp = a > sp ? a : sp;
        for (int p = 0; p < 4; ++p)
            if ((mask >> p) & 1) { const double y = progPeakAt(w + kPeakHist, p); tp = y > tp ? y : tp; }
        for (int j = 0; j < kPeakHist; ++j) w[j] = w[j + 1];
    }
    if (!mask) tp = sp;
    for (int j = 0; j < kPeakHist; ++j) st[j] = w[j];
    st[kPeakTp] = tp > st[kPeakTp] ? tp : st[kPeakTp];
    st[kPeakSp] = sp > st[kPeakSp] ? sp : st[kPeakSp];
}

// gain under a ceiling: the loudness gain of cpq_loudness_gain, or what brings the largest of the four peaks to maxDbtp, whichever
// is smaller; peak == 0 sets no limit
inline double progGainLimited(double integrated, double peak, double targetLufs, double maxDbtp, bool& limited)
{
    const double gLoud = std::pow(10.0, (targetLufs - integrated) / 20.0);
    limited = false;
    if (!(peak > 0.0)) return gLoud;
    const double gPeak = std::pow(10.0, maxDbtp / 20.0) / peak;
    limited = gPeak < gLoud;
    return limited ? gPeak : gLoud;
}

// ------------------------------------------------------------------------------------------------------- applying a gain
struct ApplyCall {
    int n = 0;              // samples per row
    int rows = 0;
    int wide = 0;           // both strides even (and both buffers 16-byte aligned): rows are moved two samples at a time
    long long inStride = 0, outStride = 0;
};
constexpr int kApplyThreads = 256;
constexpr int kApplyMaxBlocks = 1024;               // per row: the lanes stride over what is left
// rows [rows][n] at stride s from a and from b (addresses in doubles): they overlap in part unless they are the same rows
inline bool progApplyOverlap(unsigned long long a, long long sa, unsigned long long b, long long sb, int rows, int n)
{
    if (a == b && sa == sb) return false;
    const unsigned long long ea = a + (unsigned long long)(rows - 1) * (unsigned long long)sa + (unsigned long long)n;
    const unsigned long long eb = b + (unsigned long long)(rows - 1) * (unsigned long long)sb + (unsigned long long)n;
    return a < eb && b < ea;
}
CPQ_HD inline int progApplyBlocks(const ApplyCall& c)
{
    const int units = c.wide ? (c.n + 1) / 2 : c.n, b = (units + kApplyThreads - 1) / kApplyThreads;
    return b < kApplyMaxBlocks ? b : kApplyMaxBlocks;
}

}  // namespace cpq
