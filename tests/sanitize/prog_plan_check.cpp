// prog_plan_check.cpp -- csrc/prog_plan.hpp as a program of its own under ASan and UBSan: the plan of a call, and both kernels of
// prog_kernels.hip restated as host loops over grid, waves and lanes that call the header's functions, on heap blocks of exactly
// the sizes engine_prog.cpp allocates.  The K-weighting itself is a sequential biquad pair here (the scan's arithmetic is the
// GPU tests' matter): what is checked is every index the kernels form, the dealing of hops to waves, the carries across spans and
// calls, and the finish against the numpy model's recorded values (argv[1]: tests/golden/prog_finish_cases.txt, hop sums of real
// audio, means within the cost of another order of addition; argv[2]: tests/golden/prog_finish_edge_cases.txt, planted hop sums --
// blocks on a gate and beside it, padding between kept values -- whose sums are exact in any order: every value to the bit).
#include "prog_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

using namespace cpq;

static int failed = 0, checks = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        ++checks;                                                                 \
        if (!(cond)) { ++failed; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

struct Biquad2 {
    double x1 = 0, x2 = 0, y1 = 0, y2 = 0;
    double run(double v)
    {
        const double y = 0.9 * v - 0.3 * x1 + 0.1 * x2 + 1.2 * y1 - 0.4 * y2;     // any stable filter: the check is about indices
        x2 = x1; x1 = v; y2 = y1; y1 = y;
        return y;
    }
};

struct Device {
    int S, H, maxHops;
    long long pos = 0;
    std::unique_ptr<double[]> state, part, hops;            // [2 S][8], [2 S], [S][maxHops]: exactly as allocated
    std::vector<Biquad2> filt;
    Device(int s, int h, int m) : S(s), H(h), maxHops(m), state(new double[16 * s]()), part(new double[2 * s]()),
                                  hops(new double[(size_t)s * m]()), filt(2 * s) {}
};

// k_prog_hops for one workgroup (stream s): the same barriers' phases one after the other
static void hopsKernel(Device& d, const ProgCall& c, const double* in, int s)
{
    std::unique_ptr<double[]> bufs[2] = { std::unique_ptr<double[]>(new double[kProgBufDoubles]), std::unique_ptr<double[]>(new double[kProgBufDoubles]) };
    double seg[2][kProgSegs] = {}, pend[2][2] = {};
    for (int chn = 0; chn < 2; ++chn) pend[1][chn] = d.part[2 * s + chn];
    int par = 0;
    for (int s0 = 0; s0 < c.n; s0 += kProgSpan, par ^= 1) {
        const int len = progSpanLen(c, s0);
        CHECK(len >= 1 && len <= kProgSpan, "span length %d", len);
        for (int chn = 0; chn < 2; ++chn) {
            const double* x = in + (long long)(2 * s + chn) * c.stride;
            double* buf = bufs[chn].get();
            for (int t = 0; t < kProgLanes; ++t)
                for (int i = t; i < kProgSpan; i += kProgLanes) buf[progPad(i)] = i < len ? x[s0 + i] : 0.0;
            for (int i = 0; i < len; ++i) buf[progPad(i)] = d.filt[2 * s + chn].run(buf[progPad(i)]);
        }
        const int k0 = progHopAt(c, s0), k1 = progHopAt(c, s0 + len - 1);
        CHECK(k1 - k0 < kProgSegs && k0 >= c.h0 && k1 <= c.h1, "hops %d..%d of a span", k0, k1);
        for (int chn = 0; chn < 2; ++chn)
            for (int wave = 0; wave < 4; ++wave) {
                if (k0 + wave > k1) continue;
                const ProgSeg g = progSeg(c, k0 + wave, s0, len);
                CHECK(g.a >= s0 && g.b <= s0 + len && g.a < g.b, "segment [%d, %d) of span %d", g.a, g.b, s0);
                double lane[64];
                for (int l = 0; l < 64; ++l) {
                    double sum = 0.0;
                    for (int i = g.a + l; i < g.b; i += 64) { const double y = bufs[chn][progPad(i - s0)]; sum = sum + y * y; }
                    lane[l] = sum;
                }
                for (int dd = 32; dd >= 1; dd >>= 1) {
                    double nx[64];
                    for (int l = 0; l < 64; ++l) nx[l] = lane[l] + lane[l ^ dd];
                    std::memcpy(lane, nx, sizeof(lane));
                }
                seg[chn][wave] = lane[0];
            }
        for (int tid = 0; tid <= k1 - k0; ++tid) {
            const ProgSeg g = progSeg(c, k0 + tid, s0, len);
            CHECK(!g.carried || tid == 0, "only a span's first hop began before it");
            CHECK(g.complete || tid == k1 - k0, "only a span's last hop goes on");
            double l = seg[0][tid], r = seg[1][tid];
            if (g.carried) { l = pend[par ^ 1][0] + l; r = pend[par ^ 1][1] + r; }
            if (g.complete) {
                CHECK(k0 + tid < d.maxHops, "hop %d of %d", k0 + tid, d.maxHops);
                d.hops[(size_t)s * d.maxHops + k0 + tid] = l + r;
            } else { pend[par][0] = l; pend[par][1] = r; }
        }
    }
    for (int chn = 0; chn < 2; ++chn)
        if (c.fillOut) d.part[2 * s + chn] = pend[par ^ 1][chn];
}

static bool process(Device& d, const std::vector<double>& rows, long long stride, long long off, int n)
{
    ProgCall c;
    if (!progPlan(d.pos, n, d.H, d.maxHops, d.S, stride, c)) return false;
    CHECK(c.h0 == d.pos / d.H && c.h1 == (d.pos + n - 1) / d.H && c.fill0 == d.pos % d.H && c.fillOut == (d.pos + n) % d.H, "plan at %lld + %d", d.pos, n);
    CHECK(progHopBegin(c, c.h0) == -c.fill0 && progHopAt(c, 0) == c.h0 && progHopAt(c, n - 1) == c.h1, "hop grid at %lld + %d", d.pos, n);
    // the call's rows on a block of exactly the size the caller owns
    std::unique_ptr<double[]> in(new double[(size_t)(2 * d.S - 1) * stride + n]);
    for (int r = 0; r < 2 * d.S; ++r) std::copy_n(rows.data() + (size_t)r * (rows.size() / (2 * d.S)) + off, n, in.get() + (size_t)r * stride);
    for (int s = 0; s < d.S; ++s) hopsKernel(d, c, in.get(), s);
    d.pos += n;
    return true;
}

// the same programme in one sequential pass
static std::vector<double> direct(const std::vector<double>& rows, int S, int H, long long n)
{
    const long long nH = n / H;
    std::vector<double> E((size_t)S * nH, 0.0);
    for (int s = 0; s < S; ++s)
        for (int chn = 1; chn >= 0; --chn) {
            Biquad2 f;
            const double* x = rows.data() + (size_t)(2 * s + chn) * n;
            std::vector<double> sum((size_t)nH, 0.0);
            for (long long i = 0; i < n; ++i) { const double y = f.run(x[i]); if (i / H < nH) sum[(size_t)(i / H)] += y * y; }
            for (long long h = 0; h < nH; ++h) E[(size_t)s * nH + h] += sum[(size_t)h];
        }
    return E;
}

static void runSplit(int rate, int S, long long n, const std::vector<int>& calls, const char* label, unsigned seed)
{
    const int H = progHop((double)rate);
    CHECK(H == rate / 10, "hop of %d", rate);
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(-0.5, 0.5);
    std::vector<double> rows((size_t)2 * S * n);
    for (double& v : rows) v = u(rng);
    const int maxHops = (int)((n + H - 1) / H);
    Device d(S, H, maxHops);
    long long off = 0;
    for (int len : calls) {
        CHECK(process(d, rows, len + (off % 3), off, len), "%s: call of %d at %lld refused", label, len, off);
        off += len;
    }
    CHECK(off == n, "%s: the calls cover the programme", label);
    const std::vector<double> want = direct(rows, S, H, n);
    const long long nH = n / H;
    double worst = 0.0;
    for (int s = 0; s < S; ++s)
        for (long long h = 0; h < nH; ++h) {
            const double a = d.hops[(size_t)s * maxHops + h], b = want[(size_t)s * nH + h];
            worst = std::max(worst, std::fabs(a - b) / (4.0 * H * 0x1p-52 * b));
        }
    CHECK(worst <= 1.0, "%s: hop sums %.3f of the bar away", label, worst);
    std::printf("%s: rate %d, %d streams, %zu calls, %lld hops, worst %.4f of the bar\n", label, rate, S, calls.size(), nH, worst);
}

static std::vector<int> equalCalls(long long n, int piece)
{
    std::vector<int> c((size_t)(n / piece), piece);
    if (n % piece) c.push_back((int)(n % piece));
    return c;
}

static void planChecks()
{
    for (int rate : { 8000, 44100, 48000 }) {
        const int H = progHop((double)rate);
        const long long n = 3LL * H + 777;
        for (int piece : { 1, H - 1, H, H + 1, 2048, 2049 }) {
            if (piece == 1 && rate != 8000) continue;        // 1-sample calls once: each is a launch of its own here too
            runSplit(rate, 2, piece == 1 ? 2 * H + 5 : n, equalCalls(piece == 1 ? 2 * H + 5 : n, piece), ("calls of " + std::to_string(piece)).c_str(), 11u + (unsigned)piece);
        }
        std::mt19937 rng((unsigned)rate);
        for (int rep = 0; rep < 4; ++rep) {
            std::vector<int> calls;
            long long left = 4LL * H + 123;
            while (left > 0) { const int len = (int)std::min<long long>(left, 1 + (int)(rng() % 1500u)); calls.push_back(len); left -= len; }
            runSplit(rate, 3, 4LL * H + 123, calls, "random split", 100u + (unsigned)rep);
        }
        // a hop that straddles three calls
        runSplit(rate, 1, 2LL * H, { H / 3, H / 3, H - 2 * (H / 3) + H / 2, H - H / 2 }, "a hop over three calls", 7u);
    }
    CHECK(progHop(44100.5) == 0 && progHop(7990.0) == 0 && progHop(768010.0) == 0 && progHop(44105.0) == 0 && progHop(768000.0) == 76800, "rates");
    // the max_hops refusal: nothing is planned, and the state is as it was
    Device d(1, 800, 5);
    std::vector<double> rows(2 * 4001, 0.25);
    CHECK(process(d, rows, 3999, 0, 3999), "3999 of 4000 samples");
    ProgCall c;
    CHECK(!progPlan(d.pos, 2, d.H, d.maxHops, 1, 2, c) && d.pos == 3999, "2 samples more pass max_hops");
    CHECK(progPlan(d.pos, 1, d.H, d.maxHops, 1, 1, c) && c.h1 == 4 && c.fillOut == 0, "1 sample more ends on the grid");
    CHECK(progMaxHops(0.0) == 0 && progMaxHops(-1.0) == 0 && progMaxHops(0.05) == 1 && progMaxHops(20.0) == 200, "max hops");
    CHECK(progShortCount(29) == 0 && progShortCount(30) == 1 && progShortCount(39) == 1 && progShortCount(40) == 2 && progShortCount(81940) == 8192, "short-term blocks");
    CHECK(progPick10(11) == 1 && progPick95(11) == 10 && progPick10(21) == 2 && progPick95(21) == 19 && progPick10(1) == 0 && progPick95(1) == 0, "percentile rounding");
}

// recorded cases: "case name H nHops" / nHops hop sums / "want n_blocks n_abs n_rel n_short_kept z_gate z_int z_mom_max z_short_max z_lo z_hi"
static void finishChecks(const char* path, bool exact, int minCases)
{
    FILE* f = std::fopen(path, "r");
    CHECK(f != nullptr, "cannot open %s", path);
    if (!f) return;
    char name[128];
    int H = 0, nHops = 0, cases = 0;
    while (std::fscanf(f, " case %127s %d %d", name, &H, &nHops) == 3) {
        std::unique_ptr<double[]> E(new double[(size_t)std::max(nHops, 0)]);      // exactly the hops there are
        char tok[64];
        for (int i = 0; i < nHops; ++i) { if (std::fscanf(f, "%63s", tok) != 1) { CHECK(false, "%s: short", name); break; } E[i] = std::strtod(tok, nullptr); }
        int nb, na, nr, nk;
        double z[6];
        char zt[6][64];
        if (std::fscanf(f, " want %d %d %d %d %63s %63s %63s %63s %63s %63s", &nb, &na, &nr, &nk, zt[0], zt[1], zt[2], zt[3], zt[4], zt[5]) != 10) { CHECK(false, "%s: no want line", name); break; }
        for (int i = 0; i < 6; ++i) z[i] = std::strtod(zt[i], nullptr);
        ProgFinish fin;
        fin.nHops = nHops; fin.H = H; fin.maxHops = nHops; fin.zAbs = progAbsGate();
        const ProgRecord r = progFinishHost(E.get(), fin);
        const cpq_loudness_result o = progResult(r, nHops);
        const double tol = std::max(nb, 1) * 0x1p-52;
        auto near = [&](double a, double b) { return exact ? a == b : std::fabs(a - b) <= tol * std::fabs(b); };
        CHECK(o.n_blocks == nb && r.nAbs == na && r.nRel == nr && r.nShortKept == nk, "%s: counts %d %d %d %d, recorded %d %d %d %d", name, o.n_blocks, r.nAbs, r.nRel, r.nShortKept, nb, na, nr, nk);
        CHECK(near(r.zGate, z[0]) && near(r.zInt, z[1]), "%s: means %a %a, recorded %a %a", name, r.zGate, r.zInt, z[0], z[1]);
        CHECK(r.zMomMax == z[2] && r.zShortMax == z[3] && r.zLo == z[4] && r.zHi == z[5], "%s: maxima and picks", name);
        CHECK(nr ? std::isfinite(o.integrated) : o.integrated == -HUGE_VAL, "%s: integrated", name);
        CHECK(nk ? o.range >= 0.0 : o.range == 0.0, "%s: range", name);
        ++cases;
    }
    std::fclose(f);
    CHECK(cases >= minCases, "%d recorded cases in %s", cases, path);
    std::printf("finish: %d recorded cases in %s\n", cases, path);
    if (exact) return;
    // the longest programme the sort holds
    const int nLong = 81940;
    std::unique_ptr<double[]> E(new double[(size_t)nLong]);
    for (int i = 0; i < nLong; ++i) E[i] = 800.0 * (1.0 + (double)((i * 7919) % 1000) / 1000.0);
    ProgFinish fin;
    fin.nHops = nLong; fin.H = 800; fin.maxHops = nLong; fin.zAbs = progAbsGate();
    const ProgRecord r = progFinishHost(E.get(), fin);
    CHECK(progShortCount(nLong) == kProgSortMax && r.nShortKept == kProgSortMax && r.zLo <= r.zHi && r.nAbs == nLong - 3, "the longest programme: %d kept", r.nShortKept);
}

int main(int argc, char** argv)
{
    planChecks();
    if (argc > 2) { finishChecks(argv[1], false, 10); finishChecks(argv[2], true, 16); }
    else CHECK(false, "usage: prog_plan_check tests/golden/prog_finish_cases.txt tests/golden/prog_finish_edge_cases.txt");
    std::printf("%d checks\n%d failed checks\n", checks, failed);
    return failed ? 1 : 0;
}
