// src_plan_check.cpp -- csrc/src_plan.hpp and csrc/src_host.hpp (the plan of a cpq_src call and the object) with resample_design.cpp as a program
// of its own, for the address and undefined-behaviour sanitizers.  Built and run by tests/test_stream_resample_cpu.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "src_host.hpp"

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++g_failed;                                   \
            std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

using namespace cpq;

// floor(j M / L), (j M) mod L and ceil(x L / M) in 128-bit integers: what the rebased forms must equal
static int64_t floorInWide(int64_t j, int L, int M) { return (int64_t)(((__int128)j * M) / L); }
static int phaseWide(int64_t j, int L, int M) { return (int)(((__int128)j * M) % L); }
static int64_t firstOutWide(int64_t x, int L, int M) { return (int64_t)(((__int128)x * L + M - 1) / M); }

static void rebasing()
{
    std::mt19937_64 rng(1);
    const int pairs[][2] = { { 160, 147 }, { 147, 160 }, { 2, 1 }, { 1, 2 }, { 1, 96 }, { 12, 1 }, { 1280, 1279 }, { 1279, 1280 }, { 1, 1 } };
    for (auto& p : pairs) {
        const int L = p[0], M = p[1];
        for (int t = 0; t < 2000; ++t) {
            const int64_t j = (int64_t)(rng() >> (12 + rng() % 40));             // up to 2^52: j M / L stays a position
            CHECK(srcFloorIn(j, L, M) == floorInWide(j, L, M), "L %d M %d j %" PRId64, L, M, j);
            CHECK(srcPhase(j, L, M) == phaseWide(j, L, M), "L %d M %d j %" PRId64, L, M, j);
            const int64_t x = (int64_t)(rng() >> (14 + rng() % 40));             // x L stays an input position's image
            const int64_t jf = srcFirstOutAt(x, L, M);
            CHECK(jf == firstOutWide(x, L, M), "L %d M %d x %" PRId64, L, M, x);
            CHECK(srcFloorIn(jf, L, M) >= x && (jf == 0 || srcFloorIn(jf - 1, L, M) < x), "L %d M %d x %" PRId64, L, M, x);
        }
        // j = q L + r: floor(j M / L) = q M + floor(r M / L)
        for (int r = 0; r < L; ++r) {
            const int64_t q = (INT64_C(1) << 41) + r;
            CHECK(srcFloorIn(q * L + r, L, M) == q * M + ((int64_t)r * M) / L, "L %d M %d r %d", L, M, r);
        }
    }
}

// consecutive calls tile the outputs; no output reads before the kept history; the history bound
static void sweep(int L, int M, int T, int64_t startPeriod, uint64_t seed, int calls, int maxIn)
{
    const SrcGeometry g{ L, M, T };
    SrcState s = srcInitial(g, startPeriod);
    const SrcState fresh = s;
    std::mt19937_64 rng(seed);
    int64_t emitted = s.jNext, total = 0;
    for (int i = 0; i < calls; ++i) {
        const int nIn = (int)(rng() % (uint64_t)(maxIn + 1));
        const bool flush = i == calls - 1 || rng() % 16 == 0;
        const SrcCall c = srcPlan(g, s, nIn, flush, fresh);
        const int64_t nRecvAfter = s.nRecv + nIn;
        total += nIn;
        CHECK(c.j0 == emitted, "gap or overlap: j0 %" PRId64 " after %" PRId64, c.j0, emitted);
        CHECK(c.j1 >= c.j0 && c.j1 - c.j0 <= srcMaxOut(g, maxIn), "count %" PRId64, c.j1 - c.j0);
        CHECK(c.base == s.nRecv - s.hLen && c.nVirt == s.hLen + nIn, "base");
        const int64_t firstIn = c.j1 > c.j0 ? srcFirstRead(g, s, c.j0) : nRecvAfter;      // first input index any output of the call reads
        CHECK(firstIn >= c.base, "L %d M %d: output %" PRId64 " reads %" PRId64 " before the history at %" PRId64, L, M, c.j0, firstIn, c.base);
        // what lies below v = 0 is before the stream's start only
        if (c.j1 > c.j0 && c.c0 - T + 1 < 0) CHECK(c.base == s.start, "output %" PRId64 " reads below the history of a running stream", c.j0);
        CHECK(c.hKeep >= 0 && c.hKeep <= srcHistoryBound(g) && c.hKeep <= c.nVirt, "history %d of bound %d", c.hKeep, srcHistoryBound(g));
        const int64_t nRecv = s.nRecv + nIn;
        for (int64_t j : { c.j0, c.j1 - 1 }) {
            if (c.j1 == c.j0) break;
            const int64_t newest = srcFloorIn(j, L, M) + T / 2;
            CHECK(flush || newest < nRecv, "output %" PRId64 " ahead of its input", j);
            CHECK(c.c0 + (int)((c.phase + (j - c.j0) * M) / L) == (int)(newest - c.base), "centre of %" PRId64, j);
        }
        if (!flush) CHECK(srcFloorIn(c.j1, L, M) + T / 2 >= nRecv, "output %" PRId64 " was due", c.j1);
        else CHECK(c.j1 - fresh.jNext == firstOutWide(total, L, M), "flush total %" PRId64 " of %" PRId64 " samples", c.j1 - fresh.jNext, total);
        emitted = flush ? fresh.jNext : c.j1;
        if (flush) total = 0;
        s = c.next;
        if (flush) CHECK(std::memcmp(&s, &fresh, sizeof(s)) == 0, "a flush leaves the object as new");
    }
}

// the host object against resampleRowHost over the concatenated input, bit for bit, for a seeded split
static void hostObject(double inRate, double outRate, int n, int64_t startPeriod, uint64_t seed)
{
    ResampleDesign d;
    const char* why = "";
    CHECK(resampleDesign(inRate, outRate, d, &why) == CPQ_OK, "%s", why);
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> u(-0.5, 0.5);
    const int channels = 2, maxIn = 700;
    std::vector<double> x((size_t)channels * n);
    for (double& v : x) v = u(rng);
    const int nOut = (int)resampleOutLen(n, d.L, d.M);
    std::vector<double> want((size_t)channels * nOut), got((size_t)channels * nOut);
    for (int ch = 0; ch < channels; ++ch) resampleRowHost(d, x.data() + (size_t)ch * n, n, want.data() + (size_t)ch * nOut, 0, nOut);

    SrcHost h;
    h.g = SrcGeometry{ d.L, d.M, d.T };
    h.taps = d.taps;
    h.channels = channels;
    h.startPeriod = startPeriod;
    h.hist.assign((size_t)channels * srcHistoryBound(h.g), 0.0);
    h.reset();
    std::vector<double> in((size_t)channels * maxIn);
    int at = 0, written = 0;
    while (true) {
        const int nIn = (int)std::min<uint64_t>(rng() % (maxIn + 1), (uint64_t)(n - at));
        const bool flush = at + nIn == n;
        for (int ch = 0; ch < channels; ++ch) std::copy_n(x.data() + (size_t)ch * n + at, nIn, in.data() + (size_t)ch * maxIn);
        const int64_t count = h.outCount(nIn, flush);
        // exactly as large as the call needs: a write beyond it is the sanitizer's to catch
        std::vector<double> exact((size_t)channels * (size_t)std::max<int64_t>(count, 1));
        const int m = h.process(nIn ? in.data() : nullptr, maxIn, nIn, exact.data(), (size_t)std::max<int64_t>(count, 1), flush);
        CHECK(m == count, "out_count %" PRId64 ", wrote %d", count, m);
        CHECK(written + m <= nOut, "more outputs than the one-shot row");
        if (written + m > nOut) return;
        for (int ch = 0; ch < channels; ++ch) std::copy_n(exact.data() + (size_t)ch * std::max<int64_t>(count, 1), m, got.data() + (size_t)ch * nOut + written);
        written += m;
        at += nIn;
        if (flush) break;
    }
    CHECK(written == nOut, "%d of %d outputs", written, nOut);
    CHECK(std::memcmp(got.data(), want.data(), got.size() * sizeof(double)) == 0, "%g -> %g, start period %" PRId64 ": bits differ", inRate, outRate, startPeriod);
}

int main()
{
    rebasing();
    std::mt19937_64 rng(7);
    for (int t = 0; t < 300; ++t) {
        const int L = 1 + (int)(rng() % 1280), M = 1 + (int)(rng() % 1280);
        const int T = 2 * (int)std::ceil(300.0 * std::max(1.0, (double)M / L));
        const int64_t period = t % 3 == 0 ? 0 : (int64_t)(rng() >> (14 + rng() % 40)) / L;      // up to 2^50 / L periods: positions beyond 2^40
        sweep(L, M, T, period, rng(), 60, t % 2 ? 1 + (int)(rng() % 50) : 1 + (int)(rng() % (3 * T)));
    }
    sweep(160, 147, 600, (INT64_C(1) << 50) / 160, 11, 400, 4096);
    sweep(1, 96, 57600, (INT64_C(1) << 50), 12, 200, 3000);
    hostObject(44100, 48000, 1237, 0, 21);
    hostObject(44100, 48000, 1237, (INT64_C(1) << 40) / 160, 21);
    hostObject(96000, 44100, 3000, 5, 22);
    hostObject(8000, 96000, 700, (INT64_C(1) << 44), 23);
    hostObject(768000, 8000, 2500, 3, 24);
    std::printf("\n%d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
