// src_device_check.cpp -- csrc/src_device_plan.hpp as a program of its own, for the address and undefined-behaviour sanitizers.
// k_src_resample and k_src_keep (csrc/resample_kernels.hip) restated as host loops over grid, lanes and chunks that call the
// header's functions, on heap blocks of exactly the sizes the device object allocates or the caller passes: hist
// [channels][hBound], in [channels][n_in], out [channels][n_out], stage [srcStageLen].  An index outside them is a sanitizer
// report.  Every call is compared with cpq::SrcHost fed the same samples, bit for bit: the rows, and hist over hKeep after the
// keep step.  Built and run by tests/test_src_device_plan_cpu.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "src_device_plan.hpp"
#include "src_host.hpp"

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

// the device object without a device: what engine_src.cpp keeps (state, hist) and what its two launches do
struct Model {
    SrcGeometry g;
    int channels = 0;
    int64_t startPeriod = 0;
    const double* taps = nullptr;
    std::unique_ptr<double[]> hist;         // [channels][srcHistoryBound], zeroed at create, never again
    SrcState s;

    SrcState fresh() const { return srcInitial(g, startPeriod); }

    // k_src_resample over the grid (tilesPerRow, channels); the lanes of a workgroup between two barriers run one after another
    void resample(const SrcLaunch& a, const double* in, double* out) const
    {
        CHECK(srcLdsBytes(a.span) < kSrcLdsLimit, "LDS %lld bytes", srcLdsBytes(a.span));
        std::vector<double> acc((size_t)a.tile);
        for (int ch = 0; ch < a.channels; ++ch)
            for (int tileIndex = 0; tileIndex < a.tilesPerRow; ++tileIndex) {
                const int cBase = srcTileBase(a, tileIndex);
                std::fill(acc.begin(), acc.end(), 0.0);
                for (int kc = 0; kc < a.T; kc += kSrcChunk) {
                    const int kn = srcChunkLen(a, kc), lo = srcStageLo(cBase, kc, kn), len = srcStageLen(a.span, kn);
                    std::unique_ptr<double[]> stage(new double[(size_t)len]);
                    for (int tid = 0; tid < a.tile; ++tid)
                        for (int sIdx = tid; sIdx < len; sIdx += a.tile) stage[(size_t)sIdx] = srcVirt(a, hist.get(), in, ch, lo + sIdx);
                    for (int tid = 0; tid < a.tile; ++tid) {
                        const SrcOutput at = srcOutput(a, srcLaneOutput(a, tileIndex, tid));
                        const int d = at.c - cBase;
                        CHECK(d >= 0 && d < a.span, "d %d outside 0..%d (L %d M %d tile %d lane %d)", d, a.span - 1, a.L, a.M, tileIndex, tid);
                        CHECK(at.row >= 0 && at.row < a.L, "row %d", at.row);
                        const double* hk = taps + (size_t)at.row * (size_t)a.T + kc;
                        const int mine = std::min(kn, srcTapEnd(a, at.c) - kc);
                        for (int kk = 0; kk < mine; ++kk) acc[(size_t)tid] = std::fma(hk[kk], stage[(size_t)srcStageAt(d, kn, kk)], acc[(size_t)tid]);
                    }
                }
                for (int tid = 0; tid < a.tile; ++tid) {
                    const int o = tileIndex * a.tile + tid;
                    if (o < a.nOut) out[(long long)ch * a.outStride + o] = acc[(size_t)tid];
                }
            }
    }

    // k_src_keep: one workgroup per channel, ascending chunks, each loaded whole before it is stored
    void keep(const SrcLaunch& a, const double* in)
    {
        if (!srcKeepMoves(a)) return;
        std::vector<char> written((size_t)a.hBound);
        for (int ch = 0; ch < a.channels; ++ch) {
            std::fill(written.begin(), written.end(), 0);
            double reg[kSrcKeepBlock];
            for (int chunk = 0; chunk < srcKeepChunks(a); ++chunk) {
                for (int tid = 0; tid < kSrcKeepBlock; ++tid) {
                    const int i = chunk * kSrcKeepBlock + tid, v = a.keepShift + i;
                    if (i < a.keepLen && v >= 0 && v < a.hLen) CHECK(!written[(size_t)v], "keep reads slot %d after it was overwritten", v);
                    reg[tid] = i < a.keepLen ? srcVirt(a, hist.get(), in, ch, v) : 0.0;
                }
                for (int tid = 0; tid < kSrcKeepBlock; ++tid) {
                    const int i = chunk * kSrcKeepBlock + tid;
                    if (i < a.keepLen) {
                        hist[(size_t)ch * (size_t)a.hBound + (size_t)i] = reg[tid];
                        written[(size_t)i] = 1;
                    }
                }
            }
        }
    }
};

enum Values { kNoise, kDenormal, kZero };

struct Pair {
    SrcHost ref;
    Model dev;
    std::mt19937_64 rng;
    Values values = kNoise;
    const char* name = "";

    Pair(const ResampleDesign& d, int channels, int64_t startPeriod, uint64_t seed, const char* what) : rng(seed), name(what)
    {
        ref.g = SrcGeometry{ d.L, d.M, d.T };
        ref.taps = d.taps;
        ref.channels = channels;
        ref.startPeriod = startPeriod;
        ref.hist.assign((size_t)channels * (size_t)srcHistoryBound(ref.g), 0.0);
        ref.reset();
        dev.g = ref.g;
        dev.channels = channels;
        dev.startPeriod = startPeriod;
        dev.taps = d.taps.data();
        dev.hist.reset(new double[(size_t)channels * (size_t)srcHistoryBound(ref.g)]());
        dev.s = dev.fresh();
    }

    double sample()
    {
        if (values == kZero) return 0.0;
        if (values == kDenormal) {          // the smallest denormals, either sign: products and sums that underflow to +-0
            const double v = (double)(1 + rng() % 3) * 4.9406564584124654e-324;
            return rng() % 2 ? v : -v;
        }
        return std::uniform_real_distribution<double>(-0.5, 0.5)(rng);
    }

    // smallest call length that gives at least `want` outputs now (up-sampling ratios emit in steps of L), or -1 above maxIn
    int lengthFor(int64_t want, int maxIn) const
    {
        for (int n = 0; n <= maxIn; ++n)
            if (ref.outCount(n, false) >= want) return n;
        return -1;
    }

    void reset()
    {
        ref.reset();
        dev.s = dev.fresh();                // host state only: hist keeps what it held
    }

    int64_t call(int nIn, bool flush)
    {
        const int channels = ref.channels;
        const int64_t count = ref.outCount(nIn, flush);
        std::unique_ptr<double[]> in(nIn ? new double[(size_t)channels * (size_t)nIn] : nullptr);
        for (size_t i = 0; i < (size_t)channels * (size_t)nIn; ++i) in[i] = sample();
        const size_t nOutAll = (size_t)channels * (size_t)count;
        std::unique_ptr<double[]> want(count ? new double[nOutAll] : nullptr), got(count ? new double[nOutAll] : nullptr);

        const SrcCall plan = srcPlan(dev.g, dev.s, nIn, flush, dev.fresh());
        const SrcLaunch a = srcLaunch(dev.g, plan, dev.s.hLen, nIn, channels, nIn, count);
        CHECK(a.nOut == count, "%s: launch of %d outputs, out_count %" PRId64, name, a.nOut, count);
        CHECK(a.tile == (a.M <= 8LL * a.L ? 256 : 64) && a.tilesPerRow == (a.nOut + a.tile - 1) / a.tile, "%s: grid", name);
        CHECK(a.keepLen <= a.hBound && a.keepShift >= 0 && a.keepShift + a.keepLen == a.nVirt, "%s: keep step", name);
        if (a.tilesPerRow > 0) dev.resample(a, in.get(), got.get());
        dev.keep(a, in.get());
        dev.s = plan.next;

        const int m = ref.process(in.get(), (size_t)nIn, nIn, want.get(), (size_t)count, flush);
        CHECK(m == count, "%s: host wrote %d of %" PRId64, name, m, count);
        CHECK(count == 0 || std::memcmp(got.get(), want.get(), nOutAll * sizeof(double)) == 0, "%s: rows differ in a call of %d samples, %" PRId64 " outputs",
              name, nIn, count);
        CHECK(dev.s.start == ref.s.start && dev.s.nRecv == ref.s.nRecv && dev.s.jNext == ref.s.jNext && dev.s.hLen == ref.s.hLen, "%s: state", name);
        const size_t hs = (size_t)srcHistoryBound(ref.g);
        for (int ch = 0; ch < channels; ++ch)
            CHECK(plan.hKeep == 0 || std::memcmp(dev.hist.get() + ch * hs, ref.hist.data() + ch * hs, (size_t)plan.hKeep * sizeof(double)) == 0,
                  "%s: hist of channel %d differs over %d samples after a call of %d", name, ch, plan.hKeep, nIn);
        ++g_calls;
        g_outputs += count * channels;
        return count;
    }
};

static ResampleDesign design(double inRate, double outRate)
{
    ResampleDesign d;
    const char* why = "";
    CHECK(resampleDesign(inRate, outRate, d, &why) == CPQ_OK, "%g -> %g: %s", inRate, outRate, why);
    return d;
}

static void ratio(double inRate, double outRate, int expectL, int expectM, int expectTile)
{
    char name[64];
    std::snprintf(name, sizeof(name), "%g -> %g", inRate, outRate);
    const ResampleDesign d = design(inRate, outRate);
    const int T = d.T, tile = srcTile(d.L, d.M);
    CHECK(d.L == expectL && d.M == expectM && tile == expectTile, "%s: L %d M %d tile %d", name, d.L, d.M, tile);
    CHECK(srcLdsBytes(srcSpan(d.L, d.M, tile)) < kSrcLdsLimit, "%s: LDS", name);
    // a call of max_in samples holds 2 tile + 1 outputs and the whole filter
    const int maxIn = std::max(T, (int)(((long long)(2 * tile + 2) * d.M) / d.L) + 2);

    {   // the call lengths of the edges, one stream: short calls while nothing is due yet, then whole tiles, then max_in, then the flush
        Pair p(d, 2, 0, 31, name);
        for (int n : { 0, 1, T / 2 - 1, T / 2, T / 2 + 1, T }) p.call(std::min(n, maxIn), false);
        for (int want : { tile - 1, tile, tile + 1, 2 * tile + 1 }) {
            const int n = p.lengthFor(want, maxIn);
            CHECK(n >= 0, "%s: no call of up to %d samples gives %d outputs", name, maxIn, want);
            if (n < 0) continue;
            const int64_t count = p.call(n, false);
            CHECK(count >= want && count < want + d.L, "%s: %" PRId64 " outputs for %d", name, count, want);
        }
        p.call(maxIn, false);
        p.call(0, false);
        p.call(1, true);
        // after the flush: as new, hist still holding the old stream
        p.call(T / 2 + 3, false);
        p.call(0, true);
    }
    {   // a stream that ends inside its first tile, and one flushed before anything was due
        Pair p(d, 1, 0, 32, name);
        p.call(1, true);
        p.call(std::min(T / 2 - 1, maxIn), true);
        p.call(0, true);
    }
    const int most = T > 4000 ? T / 4 : std::min(maxIn, 3 * T / 2);
    for (int64_t period : { INT64_C(0), INT64_C(3), INT64_C(1) << 40 }) {    // seeded random splits, flushes in mid-stream, reset
        Pair p(d, 2, period, 33 + (uint64_t)period % 7, name);
        for (int i = 0; i < (T > 4000 ? 6 : 24); ++i) {
            const int n = (int)(p.rng() % (uint64_t)(most + 1));
            p.call(i % 5 == 4 ? n % 3 : n, p.rng() % 6 == 0);
            if (i == 13) p.reset();
        }
        p.call(5, true);
    }
    if (T < 4000) {     // values: sums that underflow at the start of a stream, where the row begins inside the filter; zeros
        Pair p(d, 2, 0, 40, name);
        p.values = kDenormal;
        p.call(T / 2 + 40, false);
        p.call(T, true);
        p.values = kZero;
        p.call(T, true);
    }
}

int main()
{
    ratio(44100, 48000, 160, 147, 256);
    ratio(48000, 44100, 147, 160, 256);
    ratio(48000, 96000, 2, 1, 256);
    ratio(96000, 48000, 1, 2, 256);
    ratio(96000, 8000, 1, 12, 64);
    ratio(8000, 96000, 12, 1, 256);
    ratio(768000, 8000, 1, 96, 64);
    std::printf("%lld calls, %lld outputs\n", g_calls, g_outputs);
    std::printf("\n%d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
