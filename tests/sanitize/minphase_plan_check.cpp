// Stand-alone check of minphase_plan.hpp and of the split cpq_ir_prepare steps of ir_ingest.cpp under AddressSanitizer and UBSan.
//   g++ -O1 -g -std=c++20 -fsanitize=address,undefined -Iconvopeq_amd/csrc -Iinclude tests/sanitize/minphase_plan_check.cpp
//       convopeq_amd/csrc/ir_ingest.cpp -o minphase_plan_check
// The plan: every n in 1 ... 4100 and every power-of-two edge up to 2097152 -- N against the reference's nextPowerOfTwo(4 n), the
// factorisation, the launch list, the chunking under a cap.  The steps: cpq_ir_prepare against the three steps called by hand.
#include "ir_ingest.hpp"
#include "minphase_plan.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int g_failed = 0;

void check(bool ok, const char* what, double a = 0.0, double b = 0.0)
{
    if (ok) return;
    ++g_failed;
    std::printf("FAILED %s (%g, %g)\n", what, a, b);
}

// juce::nextPowerOfTwo
long long nextPowerOfTwo(long long n)
{
    --n;
    n |= n >> 1; n |= n >> 2; n |= n >> 4; n |= n >> 8; n |= n >> 16; n |= n >> 32;
    return n + 1;
}

void checkLength(int n)
{
    const int lg = cpq::minphaseFftLog2(n);
    if ((long long)n * 4 > cpq::kMinphaseMaxFft) { check(lg < 0, "too long is refused", n); return; }
    check(lg >= 2 && (1LL << lg) == nextPowerOfTwo((long long)n * 4), "N is the reference's", n, lg);
    int lg1 = -1, lg2 = -1;
    cpq::minphaseFactor(lg, lg1, lg2);
    check(lg1 >= 0 && lg2 >= 1 && lg1 + lg2 == lg, "N1 N2 == N", lg1, lg2);
    check(lg1 <= cpq::kMinphaseLdsLog2 && lg2 <= cpq::kMinphaseLdsLog2, "factors within N_LDS", lg1, lg2);
    check((lg <= cpq::kMinphaseLdsLog2) == (lg1 == 0), "the small path up to N_LDS", lg, lg1);
    if (lg1 > 0) {
        const int C = cpq::minphaseColTile(lg1);
        check(C >= 1 && (C & (C - 1)) == 0 && ((1 << lg2) % C) == 0, "column tile divides N2", C, lg2);
        check(cpq::minphaseColsLds(lg1) <= 160 * 1024 && ((size_t)16 << lg2) <= 160 * 1024, "LDS", (double)cpq::minphaseColsLds(lg1));
        check(lg1 <= lg2 && lg2 - lg1 <= 1, "balanced factors", lg1, lg2);
    }
    check(cpq::minphaseRowBytes(n, lg) >= 16LL * n + (lg1 > 0 ? 16LL << lg : 0), "row bytes hold the buffers", n);

    cpq::MinphaseGroup g;
    g.log2n = lg;
    g.log2n1 = lg1;
    g.log2n2 = lg2;
    const std::vector<cpq::MinphaseLaunch> l = cpq::minphaseLaunches(g, 3);
    check(l.size() == (lg1 > 0 ? 5u : 1u), "launch count", (double)l.size());
    for (const cpq::MinphaseLaunch& k : l) {
        check(k.grid >= 3 && k.grid < (1LL << 31) && k.block == cpq::kMinphaseThreads && k.lds <= 160 * 1024, "launch shape", (double)k.grid);
        if (k.kernel == cpq::kMinphaseKCols) check(k.grid == 3LL * ((1 << lg2) / cpq::minphaseColTile(lg1)), "column grid", (double)k.grid);
        if (k.kernel == cpq::kMinphaseKRows) check(k.grid == 3LL << lg1, "row grid", (double)k.grid);
        if (k.kernel == cpq::kMinphaseKSmall) check(k.grid == 3 && k.lds == ((size_t)16 << lg), "small grid", (double)k.grid);
    }
}

// a batch of mixed lengths: groups hold every row once; chunks cover a group's rows once, in order, under the cap
void checkBatch(const std::vector<int>& channels, const std::vector<int>& samples, long long cap)
{
    std::vector<char> tooLong;
    const auto groups = cpq::minphaseGroups(channels.data(), samples.data(), (int)samples.size(), tooLong);
    std::vector<int> seen(samples.size(), 0);
    for (const auto& g : groups) {
        for (size_t a = 0; a < groups.size(); ++a)
            if (&groups[a] != &g) check(groups[a].log2n != g.log2n, "one group per N");
        int lastIr = -1, lastCh = -1;
        for (const auto& r : g.rows) {
            check(r.ir >= 0 && r.ir < (int)samples.size() && r.n == samples[(size_t)r.ir] && cpq::minphaseFftLog2(r.n) == g.log2n, "row in its group");
            check(r.ir > lastIr || (r.ir == lastIr && r.ch == lastCh + 1), "rows in order");
            lastIr = r.ir;
            lastCh = r.ch;
            ++seen[(size_t)r.ir];
        }
        std::vector<cpq::MinphaseChunk> chunks;
        const bool ok = cpq::minphaseChunks(g, cap, chunks);
        const long long need = cpq::minphaseRowNeed(g);
        check(ok == (cap >= need), "a cap below one row is refused", (double)cap, (double)need);
        if (!ok) { check(chunks.empty(), "no chunks of a refused group"); continue; }
        size_t next = 0;
        for (const auto& c : chunks) {
            check(c.first == next && c.count >= 1 && c.count <= (size_t)cpq::kMinphaseMaxChunkRows, "chunks are consecutive");
            long long bytes = 0, total = 0;
            for (size_t r = c.first; r < c.first + c.count && r < g.rows.size(); ++r) {
                bytes += cpq::minphaseRowBytes(g.rows[r].n, g.log2n);
                total += g.rows[r].n;
            }
            check(bytes <= cap, "chunk under the cap", (double)bytes, (double)cap);
            check(total == c.samples, "chunk sample count", (double)total, (double)c.samples);
            next = c.first + c.count;
        }
        check(next == g.rows.size(), "chunks cover the group", (double)next, (double)g.rows.size());
        std::vector<cpq::MinphaseChunk> none;
        check(!cpq::minphaseChunks(g, need - 1, none) && none.empty(), "one byte short");
        check(cpq::minphaseChunks(g, need, none) && !none.empty(), "exactly one row's need");
    }
    for (size_t i = 0; i < samples.size(); ++i) {
        const bool refused = (long long)samples[i] * 4 > cpq::kMinphaseMaxFft;
        check((tooLong[i] != 0) == refused && seen[i] == (refused ? 0 : channels[i]), "every row once", (double)i, seen[i]);
    }
}

double noise(unsigned& s)
{
    s = s * 1664525u + 1013904223u;
    return (double)(int)(s >> 8) / 8388608.0 - 1.0;
}

bool sameBits(const void* a, const void* b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }

// cpq_ir_prepare against its three steps called by hand, the middle one given cpq_ir_convert_to_minimum_phase's result
void checkSteps(int channels, int n, int phase, bool withCurrent, double decay)
{
    unsigned seed = 99u + (unsigned)n;
    std::vector<double> x((size_t)channels * (size_t)n), cur(64);
    for (size_t i = 0; i < x.size(); ++i) x[i] = noise(seed) * std::exp(-decay * (double)(i % (size_t)n));
    for (auto& v : cur) v = 0.01 * noise(seed);
    cpq_ir_buffer in{ channels, n, 48000.0, x.data() }, current{ 1, 64, 48000.0, cur.data() };
    const cpq_ir_buffer* curPtr = withCurrent ? &current : nullptr;
    cpq_ir_prepared whole, steps;
    const int rcWhole = cpq_ir_prepare(&in, 48000.0, 0.01f, phase, curPtr, 0.5, &whole);
    int rcSteps = cpq::irPrepareTrim(&in, 48000.0, 0.01f, phase, curPtr, &steps);
    if (rcSteps == CPQ_OK) {
        if (phase == CPQ_PHASE_MINIMUM) {
            cpq_ir_buffer mp;
            if (cpq_ir_convert_to_minimum_phase(&steps.ir, &mp) == CPQ_OK) {
                check(cpq::irPrepareAccept(&mp, &steps.ir), "a converted IR validates");
                cpq_ir_buffer_free(&mp);
            }
        }
        rcSteps = cpq::irPrepareFinish(curPtr, 0.5, &steps);
    }
    check(rcWhole == rcSteps, "step status", rcWhole, rcSteps);
    if (rcWhole == CPQ_OK && rcSteps == CPQ_OK) {
        check(whole.ir.n_channels == steps.ir.n_channels && whole.ir.n_samples == steps.ir.n_samples && whole.ir.n_samples == 479, "shape");
        check(sameBits(whole.ir.data, steps.ir.data, sizeof(double) * (size_t)whole.ir.n_channels * (size_t)whole.ir.n_samples), "IR bits");
        check(sameBits(&whole.scale, &steps.scale, sizeof(whole.scale)) && whole.ir_peak_latency == steps.ir_peak_latency, "scale and latency");
    }
    cpq_ir_prepared_free(&whole);
    cpq_ir_prepared_free(&steps);
}

}  // namespace

int main()
{
    for (int n = 1; n <= 4100; ++n) checkLength(n);
    for (int lg = 0; lg <= 21; ++lg)
        for (int d = -1; d <= 1; ++d)
            if ((1 << lg) + d >= 1) checkLength((1 << lg) + d);
    checkLength(2097153);
    check(cpq::minphaseFftLog2(0) < 0 && cpq::minphaseFftLog2(-5) < 0 && cpq::minphaseFftLog2(2097152) == 23, "edges");
    check(cpq::minphaseFftLog2(1) == 2 && cpq::minphaseFftLog2(1024) == 12 && cpq::minphaseFftLog2(1025) == 13, "small edges");

    // mono and stereo IRs across small, boundary and four-step sizes, one too long; generous, tight and too small caps
    const std::vector<int> channels{ 2, 1, 2, 1, 2, 1, 2, 3, 1 }, samples{ 700, 1024, 1025, 3, 700, 2097153, 16385, 1000, 4097 };
    for (long long cap : { 1LL << 40, 2LL << 30, 16LL * 16385 + (16LL << 17) + 33, 16LL << 17, 70000LL, 100LL, 0LL }) checkBatch(channels, samples, cap);
    checkBatch({}, {}, 1 << 20);
    std::vector<int> many(3000, 1), lens(3000, 1024);       // rows beyond one chunk of 2048 bytes-per-row budget
    checkBatch(many, lens, 10 * cpq::minphaseRowBytes(1024, 12) + 5);

    // twiddles: unit modulus, symmetry, the two levels against the direct root
    const std::vector<double> roots = cpq::minphaseStageRoots();
    check(roots.size() == 8192 && roots[0] == 1.0 && roots[1] == 0.0 && roots[2 * 1024] == 0.0 && roots[2 * 1024 + 1] == -1.0, "stage roots");
    for (int j = 1; j < 2048; ++j) {
        check(roots[2 * (size_t)j] == -roots[2 * (size_t)(j + 2048)] && roots[2 * (size_t)j + 1] == -roots[2 * (size_t)(j + 2048) + 1], "half turn", j);
        check(roots[2 * (size_t)j] == roots[2 * (size_t)(4096 - j)] && roots[2 * (size_t)j + 1] == -roots[2 * (size_t)(4096 - j) + 1], "conjugate", j);
        check(std::fabs(std::hypot(roots[2 * (size_t)j], roots[2 * (size_t)j + 1]) - 1.0) <= 3.4e-16, "unit modulus", j);
    }
    for (int lg : { 2, 3, 12, 13, 18, 23 }) {
        std::vector<double> hi, lo;
        cpq::minphaseSplitRoots(lg, hi, lo);
        const long long N = 1LL << lg;
        check((long long)lo.size() == 2 * (N < 4096 ? N : 4096) && (long long)hi.size() == 2 * (N > 4096 ? N / 4096 : 1), "table sizes", lg);
        for (long long m = 0; m < N; m += (N > 4096 ? N / 997 : 1)) {
            double re, im;
            cpq::minphaseRoot(m, N, re, im);
            const double *a = &hi[2 * (size_t)(m >> 12)], *b = &lo[2 * (size_t)(m & 4095)];
            check(std::fabs(a[0] * b[0] - a[1] * b[1] - re) <= 5.0e-16 && std::fabs(a[0] * b[1] + a[1] * b[0] - im) <= 5.0e-16, "two-level root", lg, (double)m);
        }
    }

    // the steps of cpq_ir_prepare
    checkSteps(1, 300, CPQ_PHASE_AS_IS, false, 0.01);
    checkSteps(2, 700, CPQ_PHASE_AS_IS, true, 0.02);
    checkSteps(2, 480, CPQ_PHASE_MINIMUM, true, 0.02);
    checkSteps(1, 1000, CPQ_PHASE_MINIMUM, false, 0.005);
    checkSteps(1, 200, CPQ_PHASE_MIXED, false, 0.01);
    cpq_ir_prepared p;
    double one = 1.0;
    cpq_ir_buffer bad{ 0, 1, 48000.0, &one };
    check(cpq::irPrepareTrim(&bad, 48000.0, 1.0f, CPQ_PHASE_AS_IS, nullptr, &p) == CPQ_ERR_INVALID_ARG && !p.ir.data, "no channels");
    check(cpq::irPrepareTrim(nullptr, 48000.0, 1.0f, CPQ_PHASE_AS_IS, nullptr, &p) == CPQ_ERR_INVALID_ARG && !p.ir.data, "null IR");
    check(std::strlen(cpq::irPrepareWhy(CPQ_ERR_UNSUPPORTED)) > 0, "a reason");

    std::printf("lengths 1 ... 4100 and the power-of-two edges to 2097152, 9 batches, 6 table sizes, 5 prepare runs\n");
    std::printf("%d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
