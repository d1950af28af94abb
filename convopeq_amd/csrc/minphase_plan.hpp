// minphase_plan.hpp -- the plan of one cpq_ir_minimum_phase_batch call: pure functions, no HIP (compiled alone into
// tests/sanitize/minphase_plan_check.cpp).  engine_minphase.cpp allocates, uploads, launches and downloads from what is here;
// minphase_kernels.hip holds the kernels the launch list names.
//
// A row is one channel of one IR, n samples, transformed at N = nextPow2(4 n) complex points (the reference's
// juce::nextPowerOfTwo(numSamples * 4), ResampleAndFallback.cpp:341; above 8388608 the reference skips the conversion).
//   N <= kMinphaseLds   one workgroup keeps the row in LDS through the whole sequence (k_minphase_small)
//   above               N = N1 * N2, N1 = 2^floor(log2 N / 2) <= N2 <= kMinphaseLds: every transform is a pass over the columns
//                       (N1 points at stride N2, a tile of adjacent columns per workgroup) and a pass over the rows (N2 contiguous
//                       points); a forward transform leaves X[k1 + N1 k2] at [k1][k2] and the inverse reads that layout, so there
//                       is no transpose, and the row pass of a forward transform and of the inverse behind it are one kernel
// Rows of one N form a group; a group runs in chunks whose device scratch stays under the call's cap.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cmath>
#include <vector>

namespace cpq {

constexpr int kMinphaseLdsLog2 = 12;
constexpr int kMinphaseLds = 1 << kMinphaseLdsLog2;                 // N_LDS: complex points a workgroup holds (64 KB)
constexpr long long kMinphaseMaxFft = 8388608;                      // MAX_MINPHASE_FFT_SIZE
constexpr int kMinphaseRootLog2 = 12;                               // the stage twiddles: one table of the 4096th roots
constexpr int kMinphaseColElems = 8192;                             // complex points of a column tile (128 KB of LDS with the pad)
constexpr int kMinphaseColTileMax = 8;                              // adjacent columns of 16 bytes: one 128-byte line
constexpr long long kMinphaseDefaultWorkspace = 2LL << 30;          // workspace_bytes == 0
constexpr int kMinphaseMaxChunkRows = 65536;                        // rows * N1 workgroups stay far below 2^31
constexpr int kMinphaseThreads = 256;

// kernels and what they do to a row (minphase_kernels.hip)
enum MinphaseKernel { kMinphaseKSmall = 0, kMinphaseKCols = 1, kMinphaseKRows = 2 };
enum MinphaseColsOp {
    kColsFwdPad = 0,        // real row, zero-padded -> forward -> twiddle -> scratch
    kColsFwdComplex = 1,    // scratch -> forward -> twiddle -> scratch                        (cpq_diag_cfft)
    kColsInvFoldFwd = 2,    // scratch -> inverse / N -> cepstral fold -> forward -> twiddle -> scratch
    kColsInvExtract = 3,    // scratch -> inverse / N -> real part of the first n, flushed and checked -> output row
    kColsInvComplex = 4     // scratch -> inverse / N -> scratch                               (cpq_diag_cfft)
};
enum MinphaseRowsOp {
    kRowsFwd = 0,           // forward, natural order out                                       (cpq_diag_cfft)
    kRowsInv = 1,           // inverse -> conjugate twiddle                                      (cpq_diag_cfft)
    kRowsLog = 2,           // forward -> ln max(|X|, 1e-300) -> inverse -> conjugate twiddle
    kRowsExp = 3            // forward -> clamp +-50, exp(re) (cos im, sin im), checked -> inverse -> conjugate twiddle
};

struct MinphaseRowRef { int ir, ch, n; };
struct MinphaseGroup {
    int log2n = 0, log2n1 = 0, log2n2 = 0;      // N = 2^log2n = N1 * N2; N1 = 1 on the small path
    std::vector<MinphaseRowRef> rows;
};
struct MinphaseChunk { size_t first, count; long long samples; };     // rows [first, first + count) of a group; samples: sum of n
struct MinphaseLaunch { int kernel, op; long long grid; int block; size_t lds; };

inline int minphaseLog2(long long v) { int lg = 0; while ((1LL << lg) < v) ++lg; return lg; }

// log2 of the FFT size of an n-sample row; -1: the reference skips it
inline int minphaseFftLog2(long long n)
{
    if (n <= 0 || n * 4 > kMinphaseMaxFft) return -1;
    return minphaseLog2(n * 4);
}

inline void minphaseFactor(int log2n, int& log2n1, int& log2n2)
{
    if (log2n <= kMinphaseLdsLog2) { log2n1 = 0; log2n2 = log2n; return; }
    log2n1 = log2n / 2;
    log2n2 = log2n - log2n1;
}

inline int minphaseColTile(int log2n1)
{
    const int fit = kMinphaseColElems >> log2n1;
    return fit < kMinphaseColTileMax ? fit : kMinphaseColTileMax;
}

// device bytes of one row: the samples in and out, the complex scratch above the LDS bound, its table entry and flag word
inline long long minphaseRowBytes(int n, int log2n)
{
    const long long scratch = log2n > kMinphaseLdsLog2 ? 16LL << log2n : 0;
    return 16LL * n + scratch + 32;
}

// bytes a row moves through HBM, for the bench: n in, n out, and five read + write passes over the scratch (the first reads
// the samples, the last writes them)
inline long long minphaseRowTraffic(int n, int log2n)
{
    if (log2n <= kMinphaseLdsLog2) return 16LL * n;
    return 16LL * n + 8 * (16LL << log2n);
}

// groups in order of first appearance; status[i] = false where IR i is too long (decided here, on the host)
inline std::vector<MinphaseGroup> minphaseGroups(const int* channels, const int* samples, int count, std::vector<char>& tooLong)
{
    std::vector<MinphaseGroup> groups;
    tooLong.assign((size_t)(count > 0 ? count : 0), 0);
    for (int i = 0; i < count; ++i) {
        const int lg = minphaseFftLog2(samples[i]);
        if (lg < 0) { tooLong[(size_t)i] = 1; continue; }
        size_t g = 0;
        while (g < groups.size() && groups[g].log2n != lg) ++g;
        if (g == groups.size()) {
            groups.emplace_back();
            groups[g].log2n = lg;
            minphaseFactor(lg, groups[g].log2n1, groups[g].log2n2);
        }
        for (int ch = 0; ch < channels[i]; ++ch) groups[g].rows.push_back(MinphaseRowRef{ i, ch, samples[i] });
    }
    return groups;
}

// the largest need of one row of the group
inline long long minphaseRowNeed(const MinphaseGroup& g)
{
    long long need = 0;
    for (const MinphaseRowRef& r : g.rows) {
        const long long b = minphaseRowBytes(r.n, g.log2n);
        if (b > need) need = b;
    }
    return need;
}

// consecutive rows while their bytes stay within cap; false: cap is below one row's need (chunks is left empty)
inline bool minphaseChunks(const MinphaseGroup& g, long long cap, std::vector<MinphaseChunk>& chunks)
{
    chunks.clear();
    if (cap < minphaseRowNeed(g)) return false;
    size_t first = 0;
    long long bytes = 0, samples = 0;
    for (size_t r = 0; r < g.rows.size(); ++r) {
        const long long b = minphaseRowBytes(g.rows[r].n, g.log2n);
        if (r > first && (bytes + b > cap || r - first >= (size_t)kMinphaseMaxChunkRows)) {
            chunks.push_back(MinphaseChunk{ first, r - first, samples });
            first = r;
            bytes = samples = 0;
        }
        bytes += b;
        samples += g.rows[r].n;
    }
    if (first < g.rows.size()) chunks.push_back(MinphaseChunk{ first, g.rows.size() - first, samples });
    return true;
}

inline size_t minphaseColsLds(int log2n1)
{
    return (size_t)minphaseColTile(log2n1) * (((size_t)1 << log2n1) + 1) * 16;
}

// the launches of a chunk of `rows` rows, in order
inline std::vector<MinphaseLaunch> minphaseLaunches(const MinphaseGroup& g, long long rows)
{
    std::vector<MinphaseLaunch> l;
    if (g.log2n1 == 0) {
        l.push_back(MinphaseLaunch{ kMinphaseKSmall, 0, rows, kMinphaseThreads, (size_t)16 << g.log2n });
        return l;
    }
    const long long colGrid = rows * ((1LL << g.log2n2) / minphaseColTile(g.log2n1)), rowGrid = rows << g.log2n1;
    const size_t colLds = minphaseColsLds(g.log2n1), rowLds = (size_t)16 << g.log2n2;
    l.push_back(MinphaseLaunch{ kMinphaseKCols, kColsFwdPad, colGrid, kMinphaseThreads, colLds });
    l.push_back(MinphaseLaunch{ kMinphaseKRows, kRowsLog, rowGrid, kMinphaseThreads, rowLds });
    l.push_back(MinphaseLaunch{ kMinphaseKCols, kColsInvFoldFwd, colGrid, kMinphaseThreads, colLds });
    l.push_back(MinphaseLaunch{ kMinphaseKRows, kRowsExp, rowGrid, kMinphaseThreads, rowLds });
    l.push_back(MinphaseLaunch{ kMinphaseKCols, kColsInvExtract, colGrid, kMinphaseThreads, colLds });
    return l;
}

// exp(-2 pi i num / den), den a power of two: cos and sin of the angle reduced exactly to [0, pi / 4]
inline void minphaseRoot(long long num, long long den, double& re, double& im)
{
    num &= den - 1;
    if (den < 4) { re = num ? -1.0 : 1.0; im = 0.0; return; }
    const long long quarter = den / 4, quad = num / quarter;
    long long rem = num % quarter;
    double c = 1.0, s = 0.0;
    if (rem != 0) {
        const bool mirror = 2 * rem > quarter;
        if (mirror) rem = quarter - rem;
        if (2 * rem == quarter) c = s = std::sqrt(0.5);
        else {
            const double theta = 1.57079632679489661923 * ((double)rem / (double)quarter);
            c = std::cos(theta);
            s = std::sin(theta);
        }
        if (mirror) { const double t = c; c = s; s = t; }
    }
    switch (quad) {
    case 0: re = c; im = -s; break;
    case 1: re = -s; im = -c; break;
    case 2: re = -c; im = s; break;
    default: re = s; im = c; break;
    }
    re += 0.0;      // no negative zeros in the tables
    im += 0.0;
}

// the stage twiddles: [2^kMinphaseRootLog2][2], w^j for every j
inline std::vector<double> minphaseStageRoots()
{
    const long long T = 1LL << kMinphaseRootLog2;
    std::vector<double> t((size_t)T * 2);
    for (long long j = 0; j < T; ++j) minphaseRoot(j, T, t[(size_t)j * 2], t[(size_t)j * 2 + 1]);
    return t;
}

// the N-th roots in two levels, w_N^m = hi[m >> 12] * lo[m & 4095]: lo[b] = w_N^b, hi[a] = w_N^(4096 a); [..][2]
inline void minphaseSplitRoots(int log2n, std::vector<double>& hi, std::vector<double>& lo)
{
    const long long N = 1LL << log2n, nLo = N < 4096 ? N : 4096, nHi = N > 4096 ? N / 4096 : 1;
    lo.resize((size_t)nLo * 2);
    hi.resize((size_t)nHi * 2);
    for (long long b = 0; b < nLo; ++b) minphaseRoot(b, N, lo[(size_t)b * 2], lo[(size_t)b * 2 + 1]);
    for (long long a = 0; a < nHi; ++a) minphaseRoot(a * 4096, N, hi[(size_t)a * 2], hi[(size_t)a * 2 + 1]);
}

}  // namespace cpq
