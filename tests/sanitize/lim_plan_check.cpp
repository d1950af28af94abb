// lim_plan_check.cpp -- csrc/lim_plan.hpp as a program of its own, for the address and undefined-behaviour sanitizers.  k_lim_apply
// and k_lim_keep (csrc/lim_kernels.hip) restated as host loops over grid, lanes, rounds and steps that call the header's functions,
// on heap blocks of exactly the sizes the device object allocates or the caller passes: hist [2 S][limHalo], in [2 S][inStride],
// out [2 S][outStride], part [S][tiles], and per workgroup an LDS block of limLdsBytes(W).  An index outside them is a sanitizer
// report; every staged index is also checked against the block by hand.  What lies between two barriers of the kernel runs lane
// after lane here, with the loads of a phase done before its stores, as the barriers order them.  Every call is compared with
// cpq::LimHost fed the same samples, bit for bit: the rows, the telemetry, and hist over hKeep after the keep step.  Built and run by
// tests/test_lim_plan_cpu.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "lim_host.hpp"
#include "lim_plan.hpp"

static int g_failed = 0;
static long long g_calls = 0, g_outputs = 0;
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

static bool sameBits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// the device object without a device: what engine_lim.cpp keeps (state, hist, gains, tel) and what its two launches do
struct Model {
    int W = 0, mask = 0, streams = 0;
    double c = 1.0;
    std::unique_ptr<double[]> hist, gains;      // [2 S][limHalo(W)] zeroed at create; [S]
    std::unique_ptr<LimPartial[]> tel;
    LimState s;

    Model(int window, int phaseMask, double ceiling, int nStreams) : W(window), mask(phaseMask), streams(nStreams), c(ceiling)
    {
        hist.reset(new double[2 * (size_t)streams * (size_t)limHalo(W)]());
        gains.reset(new double[(size_t)streams]);
        tel.reset(new LimPartial[(size_t)streams]());
    }

    // k_lim_apply over the grid (tilesPerRow, streams)
    void apply(const LimLaunch& a, const double* in, double* out, LimPartial* part) const
    {
        CHECK(limLdsBytes(W) + 64 <= kLimLdsLimit, "LDS %lld bytes", limLdsBytes(W));
        const int pitch = limStagePitch(W, kLimTile), len = limStageLen(W, kLimTile), nR = limRCount(W, kLimTile), M = limM(W);
        for (int st = 0; st < a.streams; ++st)
            for (int tileIndex = 0; tileIndex < a.tilesPerRow; ++tileIndex) {
                std::unique_ptr<double[]> lds(new double[(size_t)limLdsBytes(W) / 8]);
                double* A = lds.get();
                double* B = lds.get() + pitch;
                std::vector<char> written(2 * (size_t)pitch, 0);
                const double g = gains[(size_t)st];
                const int lo = limStageLo(a, tileIndex);
                const int eLo = lo - a.hLen, e0 = limPairFirst(lo, a.hLen), nIn = a.nVirt - a.hLen;
                CHECK((e0 & 1) == 0 && eLo - e0 >= 0 && eLo - e0 <= 1, "pair origin %d of %d", e0, eLo);
                for (int tid = 0; tid < kLimThreads; ++tid)
                    for (int j = tid; j < limPairCount(W); j += kLimThreads) {
                        const int e = e0 + 2 * j, sl = e - eLo;
                        const bool whole = a.wide && e >= 0 && e + 1 < nIn && sl >= 0 && sl + 1 < len;
                        for (int ch = 0; ch < 2; ++ch) {
                            double* S = ch ? B : A;
                            const long long rowAt = (long long)(2 * st + ch) * a.inStride;
                            if (whole) {
                                CHECK((rowAt + e) % 2 == 0, "a wide access at an odd double: row %d e %d", 2 * st + ch, e);
                                S[sl] = limPre(in[rowAt + e], g);
                                S[sl + 1] = limPre(in[rowAt + e + 1], g);
                                CHECK(sameBits(S[sl], limVirt(a, hist.get(), in, g, 2 * st + ch, lo + sl)) &&
                                      sameBits(S[sl + 1], limVirt(a, hist.get(), in, g, 2 * st + ch, lo + sl + 1)), "the wide path is not the accessor");
                                written[(size_t)(ch * pitch + sl)]++; written[(size_t)(ch * pitch + sl + 1)]++;
                            } else {
                                for (int k = 0; k < 2; ++k)
                                    if (sl + k >= 0 && sl + k < len) {
                                        S[sl + k] = limVirt(a, hist.get(), in, g, 2 * st + ch, lo + sl + k);
                                        written[(size_t)(ch * pitch + sl + k)]++;
                                    }
                            }
                        }
                    }
                for (int ch = 0; ch < 2; ++ch)
                    for (int k = 0; k < len; ++k) CHECK(written[(size_t)(ch * pitch + k)] == 1, "slot %d of channel %d staged %d times", k, ch, written[(size_t)(ch * pitch + k)]);
                // the delayed samples
                std::vector<double> d0(2 * (size_t)kLimPairs * kLimThreads), d1(d0.size());
                for (int tid = 0; tid < kLimThreads; ++tid)
                    for (int k = 0; k < kLimPairs; ++k) {
                        const int sl = limDelaySlot(W, 2 * (tid + k * kLimThreads));
                        CHECK(sl >= 0 && sl + 1 < len, "delay slot %d outside the stage of %d", sl, len);
                        const size_t at = 2 * ((size_t)k * kLimThreads + (size_t)tid);
                        d0[at] = A[sl]; d0[at + 1] = A[sl + 1];
                        d1[at] = B[sl]; d1[at + 1] = B[sl + 1];
                    }
                // r over B, in rounds: the loads of a round before its stores
                for (int q0 = 0; q0 < nR; q0 += kLimThreads) {
                    double rq[kLimThreads];
                    for (int tid = 0; tid < kLimThreads; ++tid) {
                        const int q = q0 + tid, qq = q < nR ? q : nR - 1;
                        CHECK(qq >= 0 && qq + kPeakHist < len, "window %d..%d outside the stage of %d", qq, qq + kPeakHist, len);
                        rq[tid] = limRequired(A + qq + kPeakHist, B + qq + kPeakHist, a.mask, a.c);
                    }
                    for (int tid = 0; tid < kLimThreads; ++tid)
                        if (q0 + tid < nR) B[q0 + tid] = rq[tid];
                }
                // the sliding minimum: the steps swing between the stages
                double* X = B;
                double* Y = A;
                CHECK(nR <= pitch, "r of %d in a stage of %d", nR, pitch);
                int have = 1, steps = 0;
                while (have < M) {
                    const int step = 2 * have <= M ? have : M - have;
                    CHECK(step >= 1 && step <= have, "step %d on windows of %d", step, have);
                    for (int tid = 0; tid < kLimThreads; ++tid)
                        for (int q = tid; q < nR; q += kLimThreads) {
                            const double x0 = X[q], x1 = X[q >= step ? q - step : q];
                            Y[q] = x1 < x0 ? x1 : x0;
                        }
                    std::swap(X, Y);
                    have += step;
                    ++steps;
                }
                CHECK(have == M && steps <= 12, "windows of %d after %d steps", have, steps);
                LimPartial p{ 1.0, 0 };
                const int tile0 = tileIndex * kLimTile;
                for (int tid = 0; tid < kLimThreads; ++tid)
                    for (int k = 0; k < kLimPairs; ++k) {
                        const int ot = 2 * (tid + k * kLimThreads), o = tile0 + ot, at0 = ot + limReach(W);
                        CHECK(at0 - (W - 1) >= M - 1 && at0 + 1 < nR, "minima %d..%d outside %d..%d", at0 - (W - 1), at0 + 1, M - 1, nR - 1);
                        double e[2];
                        limEnvelopePair(X + at0, W, e[0], e[1]);
                        const size_t at = 2 * ((size_t)k * kLimThreads + (size_t)tid);
                        for (int k2 = 0; k2 < 2; ++k2)
                            if (o + k2 < a.nOut) {
                                limFold(p, e[k2], e[k2] < 1.0 ? 1 : 0);
                                if (a.wide && k2 == 0 && o + 1 < a.nOut)
                                    CHECK(((long long)(2 * st) * a.outStride + o) % 2 == 0 && a.outStride % 2 == 0, "a wide store at an odd double");
                                out[(long long)(2 * st) * a.outStride + o + k2] = d0[at + (size_t)k2] * e[k2];
                                out[(long long)(2 * st + 1) * a.outStride + o + k2] = d1[at + (size_t)k2] * e[k2];
                            }
                    }
                part[(long long)st * a.partStride + tileIndex] = p;
            }
    }

    // k_lim_keep: one workgroup per stream
    void keep(const LimLaunch& a, const double* in, const LimPartial* part)
    {
        for (int st = 0; st < a.streams; ++st) {
            const double g = gains[(size_t)st];
            for (int chunk = 0; chunk < limKeepChunks(a); ++chunk) {
                double v[2][kLimKeepBlock];
                for (int tid = 0; tid < kLimKeepBlock; ++tid) {
                    const int i = chunk * kLimKeepBlock + tid;
                    for (int ch = 0; ch < 2; ++ch) v[ch][tid] = i < a.keepLen ? limVirt(a, hist.get(), in, g, 2 * st + ch, a.keepShift + i) : 0.0;
                }
                for (int tid = 0; tid < kLimKeepBlock; ++tid) {
                    const int i = chunk * kLimKeepBlock + tid;
                    if (i < a.keepLen)
                        for (int ch = 0; ch < 2; ++ch) hist[(size_t)(2 * st + ch) * (size_t)a.hBound + (size_t)i] = v[ch][tid];
                }
            }
            LimPartial lane[kLimKeepBlock];
            for (int tid = 0; tid < kLimKeepBlock; ++tid) {
                lane[tid] = LimPartial{ 1.0, 0 };
                for (int t = tid; t < a.tilesPerRow; t += kLimKeepBlock) {
                    const LimPartial q = part[(long long)st * a.partStride + t];
                    limFold(lane[tid], q.minGain, q.limited);
                }
            }
            for (int sStep = kLimKeepBlock / 2; sStep >= 1; sStep >>= 1)
                for (int tid = 0; tid < sStep; ++tid) limFold(lane[tid], lane[tid + sStep].minGain, lane[tid + sStep].limited);
            LimPartial t = a.first ? LimPartial{ 1.0, 0 } : tel[(size_t)st];
            limFold(t, lane[0].minGain, lane[0].limited);
            tel[(size_t)st] = t;
        }
    }
};

enum Values { kNoise, kDenormal, kZero, kHot };

// a model and the host object, fed the same calls
struct Pair {
    Model m;
    LimHost h;
    std::mt19937_64 rng;
    Values values = kNoise;
    const char* name;
    int partCap = 0;                            // as engine_lim.cpp keeps it: the largest tile count seen
    std::unique_ptr<LimPartial[]> part;         // [S][partCap]

    Pair(int W, int mask, double c, int streams, uint64_t seed, const char* nm) : m(W, mask, c, streams), rng(seed), name(nm)
    {
        h.init(W, mask, c, streams);
        for (int s = 0; s < streams; ++s) m.gains[(size_t)s] = h.gains[(size_t)s] = 0.5 + 0.37 * s;
    }
    double sample(int i)
    {
        const double v = (double)(int64_t)(rng() % 20001) / 10000.0 - 1.0;
        switch (values) {
        case kZero: return 0.0;
        case kDenormal: return v * 4.0e-323;
        case kHot: return 3.0 * v;
        default: break;
        }
        const uint64_t k = rng() % 97;
        if (k == 0) return v * 6.0;                                 // a peak above any ceiling used here
        if (k == 1) return i % 2 ? HUGE_VAL : std::nan("");         // scrubbed
        return v * 0.4;
    }
    void reset()
    {
        m.s = LimState{};
        h.reset();
    }
    // n samples (or a flush) with padStride spare doubles in every row
    void call(int n, bool flush, int pad)
    {
        const int W = m.W, rows = 2 * m.streams;
        const LimCall c = limPlan(W, m.s, n, flush);
        CHECK(c.hLen <= limHalo(W) && c.hKeep <= limHalo(W) && c.base >= 0 && c.base + c.hLen == c.i0 && c.i1 - c.i0 == c.nOut,
              "plan: hLen %d hKeep %d base %lld", c.hLen, c.hKeep, c.base);
        const long long inStride = c.nIn + pad, outStride = c.nOut + pad;
        const int tiles = (c.nOut + kLimTile - 1) / kLimTile;
        if (tiles > partCap) {
            partCap = tiles;
            part.reset(new LimPartial[(size_t)m.streams * (size_t)partCap]);
        }
        const LimLaunch a = limLaunch(W, m.mask, m.c, c, m.streams, inStride, outStride, partCap);
        CHECK(a.tilesPerRow == tiles && a.partStride >= a.tilesPerRow, "%d tiles at a stride of %d", a.tilesPerRow, a.partStride);
        std::unique_ptr<double[]> in(new double[(size_t)rows * (size_t)inStride + 1]), out(new double[(size_t)rows * (size_t)outStride]),
            ref(new double[(size_t)rows * (size_t)outStride]);
        for (int r = 0; r < rows; ++r)
            for (long long i = 0; i < inStride; ++i) in[(size_t)(r * inStride + i)] = i < c.nIn ? sample((int)i) : std::nan("");
        for (size_t i = 0; i < (size_t)rows * (size_t)outStride; ++i) out[i] = ref[i] = -7.0;
        m.apply(a, flush ? nullptr : in.get(), out.get(), part.get());
        m.keep(a, flush ? nullptr : in.get(), part.get());
        m.s = c.next;
        h.process(flush ? nullptr : in.get(), inStride, n, ref.get(), outStride, flush);
        ++g_calls;
        g_outputs += (long long)rows * c.nOut;
        int bad = 0;
        for (size_t i = 0; i < (size_t)rows * (size_t)outStride; ++i) bad += !sameBits(out[i], ref[i]);
        CHECK(bad == 0, "%s W %d: %d doubles differ from the host object (n %d flush %d pad %d hLen %d)", name, W, bad, n, (int)flush, pad, c.hLen);
        for (int r = 0; r < rows; ++r)
            for (long long i = c.nOut; i < outStride; ++i) CHECK(out[(size_t)(r * outStride + i)] == -7.0, "row %d written past its %d outputs", r, c.nOut);
        CHECK(m.s.pos == h.s.pos && m.s.hLen == h.s.hLen, "state %lld/%d against %lld/%d", m.s.pos, m.s.hLen, h.s.pos, h.s.hLen);
        for (int s = 0; s < m.streams; ++s)
            CHECK(sameBits(m.tel[(size_t)s].minGain, h.tel[(size_t)s].minGain) && m.tel[(size_t)s].limited == h.tel[(size_t)s].limited,
                  "%s W %d: telemetry of stream %d: %g/%lld against %g/%lld", name, W, s, m.tel[(size_t)s].minGain, m.tel[(size_t)s].limited,
                  h.tel[(size_t)s].minGain, h.tel[(size_t)s].limited);
        int hbad = 0;
        for (int r = 0; r < rows; ++r)
            for (int i = 0; i < c.hKeep; ++i) hbad += !sameBits(m.hist[(size_t)r * (size_t)limHalo(W) + (size_t)i], h.hist[(size_t)r * (size_t)limHalo(W) + (size_t)i]);
        CHECK(hbad == 0, "%s W %d: %d history doubles differ after the keep step", name, W, hbad);
    }
};

// the calls of tests/test_gpu_limiter_windows.py's sweep: the history grows to one short of the halo in one call, reaches it with
// the next sample and then moves by the call's length
static void sweep(int W)
{
    Pair p(W, 0xF, std::pow(10.0, -1.0 / 20.0), 2, 300 + (uint64_t)W, "sweep");
    const int lens[] = { 5, limHalo(W) - 6, 1, kLimTile + 1, 2, 2 * kLimTile + 3 };
    const int pad = W % 2 ? 3 : 4;              // all lengths but one are odd: 3 is the 16-byte path, 4 the scalar one
    for (int n : lens) p.call(n, false, pad);
    p.call(0, true, pad);
}

// more than kLimKeepBlock tiles: a second trip of the fold, and partials whose stride is wider than the call's tile count
static void fold()
{
    Pair p(8, 0xF, std::pow(10.0, -1.0 / 20.0), 2, 400, "fold");
    const int lens[] = { 3, kLimKeepBlock * kLimTile, (kLimKeepBlock + 1) * kLimTile + 1, 1500 };
    for (int n : lens) p.call(n, false, 2);
    CHECK(p.partCap == kLimKeepBlock + 2, "partials for %d tiles", p.partCap);
    p.call(0, true, 3);
}

static void window(int W, int mask, double c, const char* name)
{
    const int D = limD(W);
    {   // the lengths a tile and the latency make special, then a flush and a second programme
        Pair p(W, mask, c, 2, 100 + (uint64_t)W, name);
        const int lens[] = { 1, 7, D, D + 1, kLimTile - 1, kLimTile, kLimTile + 1, 2 * kLimTile + 5, 2, 1 };
        int k = 0;
        for (int n : lens) p.call(n, false, k++ % 3);
        p.call(0, true, 1);
        p.call(kLimTile + 3, false, 0);
        p.call(0, true, 0);
        p.call(0, true, 2);                     // a flush of nothing: D zeros
    }
    {   // random lengths, resets, the value classes
        Pair p(W, mask, c, 3, 200 + (uint64_t)W, name);
        for (int i = 0; i < (W > 512 ? 8 : 24); ++i) {
            p.values = i % 7 == 5 ? kDenormal : i % 7 == 6 ? kZero : i % 5 == 3 ? kHot : kNoise;
            p.call(1 + (int)(p.rng() % (uint64_t)(i % 4 == 0 ? 2 * kLimTile : 2 * D)), false, (int)(p.rng() % 4));
            if (i == 13) p.reset();
            if (i == 17) p.call(0, true, 1);
        }
        p.call(0, true, 3);
    }
}

int main()
{
    CHECK(limDefaultWindow(48000.0) == 72 && limDefaultWindow(44100.0) == 66 && limDefaultWindow(1000.0) == 8 && limDefaultWindow(768000.0) == 1024, "default windows");
    CHECK(limHalo(1024) == 2069 && limReach(8) == 26 && limD(72) == 83 && limM(72) == 84, "derived constants");
    CHECK(limLdsBytes(kLimMaxWindow) + 64 <= kLimLdsLimit, "LDS at the largest window: %lld", limLdsBytes(kLimMaxWindow));
    window(8, 0xF, 0.5, "four phases");
    window(72, 0xF, std::pow(10.0, -1.0 / 20.0), "four phases");
    window(72, 0x5, 1.0, "two phases");
    window(9, 0x0, 0.75, "no phase");
    window(1024, 0xF, std::pow(10.0, -1.0 / 20.0), "four phases");
    window(1023, 0x5, 0.5, "two phases");
    // M = 2^k - 1, 2^k, 2^k + 1; nR % 256 = 254, 0, 2; halo = 255, 257, ... 1025; D = 1023, 1024, 1025
    for (int W : { 19, 20, 21, 117, 118, 122, 123, 124, 245, 246, 501, 502, 1013, 1014 }) sweep(W);
    fold();
    std::printf("%lld calls, %lld outputs\n", g_calls, g_outputs);
    std::printf("\n%d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
