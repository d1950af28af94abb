// prog_peak_check.cpp -- the true-peak and gain part of csrc/prog_plan.hpp as a program of its own under ASan and UBSan: k_prog_peak
// and k_prog_apply of prog_kernels.hip restated as host loops over grid and lanes that call the header's functions, on heap blocks
// of exactly the sizes engine_prog.cpp and a caller allocate.  The maxima are held bit for bit against the numpy model's recorded
// values (argv[1]: tests/golden/prog_peak_cases.txt), for the programme in one call, in equal calls and in random splits, and against
// the sequential host pass behind cpq_loudness_peaks_host.  The inputs are an integer generator both sides state (caseRows).
#include "prog_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

static bool sameBits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// rows [rows][n]: a 64-bit congruential generator, 24 bits a sample in [-0.5, 0.5), with values the scrub takes out planted
static std::vector<double> caseRows(int rows, long long n, unsigned long long seed)
{
    std::vector<double> x((size_t)rows * (size_t)n);
    unsigned long long s = seed;
    for (size_t i = 0; i < x.size(); ++i) {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        double v = ((double)(long long)(s >> 40) - 8388608.0) / 16777216.0;
        if (i % 97 == 5) v = std::numeric_limits<double>::quiet_NaN();
        if (i % 101 == 7) v = 1.0e300;
        if (i % 103 == 3) v = -std::numeric_limits<double>::infinity();
        x[i] = v;
    }
    return x;
}

// k_prog_peak for one workgroup (a row): the phases between its barriers one after the other
static void peakKernel(const PeakCall& c, const double* in, double* pk, int row)
{
    std::unique_ptr<double[]> buf(new double[kPeakBufDoubles]);
    std::vector<double> tp(kPeakThreads, 0.0), sp(kPeakThreads, 0.0);
    const double* x = in + (long long)row * c.stride;
    double* st = pk + (long long)row * kPeakState;
    for (int t = 0; t < kPeakHist; ++t) buf[progPeakPad(t)] = st[t];
    int len = 0;
    for (int s0 = 0; s0 < c.n; s0 += kPeakTile) {
        len = progPeakTileLen(c, s0);
        CHECK(len >= 1 && len <= kPeakTile, "tile length %d", len);
        for (int t = 0; t < kPeakThreads; ++t)
            for (int i = t; i < kPeakTile; i += kPeakThreads) buf[progPeakPad(kPeakHist + i)] = i < len ? progPeakScrub(x[s0 + i]) : 0.0;
        for (int t = 0; t < kPeakThreads; ++t) {
            double w[kPeakWindow];
            for (int m = 0; m < kPeakWindow; ++m) w[m] = buf[progPeakPad(kPeakPer * t + m)];
            progPeakLane(w, len - kPeakPer * t, c.mask, tp[t], sp[t]);
        }
        if (s0 + kPeakTile < c.n) {
            double h[kPeakHist];
            for (int t = 0; t < kPeakHist; ++t) h[t] = buf[progPeakPad(kPeakTile + t)];
            for (int t = 0; t < kPeakHist; ++t) buf[progPeakPad(t)] = h[t];
        }
    }
    double a = st[kPeakTp], b = st[kPeakSp];
    for (int t = 0; t < kPeakThreads; ++t) {
        const double v = c.mask ? tp[t] : sp[t];
        a = v > a ? v : a;
        b = sp[t] > b ? sp[t] : b;
    }
    for (int t = 0; t < kPeakHist; ++t) st[t] = buf[progPeakPad(len + t)];
    st[kPeakTp] = a;
    st[kPeakSp] = b;
}

struct Device {
    int rows;
    std::unique_ptr<double[]> pk;                   // [rows][kPeakState]: exactly as allocated
    explicit Device(int r) : rows(r), pk(new double[(size_t)r * kPeakState]()) {}
};

// one call of n samples at offset off of the programmes x [rows][total], on a block of exactly the size the caller owns
static void process(Device& d, const std::vector<double>& x, long long total, long long off, int n, long long stride, int mask)
{
    std::unique_ptr<double[]> in(new double[(size_t)(d.rows - 1) * (size_t)stride + (size_t)n]);
    for (int r = 0; r < d.rows; ++r) std::copy_n(x.data() + (size_t)r * (size_t)total + off, n, in.get() + (size_t)r * (size_t)stride);
    PeakCall c;
    c.n = n; c.mask = mask; c.rows = d.rows; c.stride = stride;
    for (int r = 0; r < d.rows; ++r) peakKernel(c, in.get(), d.pk.get(), r);
}

static void runSplit(const std::vector<double>& x, int rows, long long n, int mask, const std::vector<int>& calls, const double* want,
                     const char* name, const char* label)
{
    Device d(rows);
    long long off = 0;
    for (int len : calls) {
        process(d, x, n, off, len, len + (off % 3), mask);
        off += len;
    }
    CHECK(off == n, "%s %s: the calls cover the programme", name, label);
    for (int r = 0; r < rows; ++r) {
        const double* st = d.pk.get() + (size_t)r * kPeakState;
        CHECK(sameBits(st[kPeakTp], want[2 * r]) && sameBits(st[kPeakSp], want[2 * r + 1]), "%s %s row %d: %a %a, recorded %a %a", name, label, r,
              st[kPeakTp], st[kPeakSp], want[2 * r], want[2 * r + 1]);
        // the history is the last 11 scrubbed samples of [zeros | programme]
        for (int j = 0; j < kPeakHist; ++j) {
            const long long i = n - kPeakHist + j;
            const double h = i >= 0 ? progPeakScrub(x[(size_t)r * (size_t)n + (size_t)i]) : 0.0;
            CHECK(sameBits(st[j], h), "%s %s row %d: history %d", name, label, r, j);
        }
    }
}

static std::vector<int> equalCalls(long long n, int piece)
{
    std::vector<int> c((size_t)(n / piece), piece);
    if (n % piece) c.push_back((int)(n % piece));
    return c;
}

// "case name rate rows n seed" / "want tp sp tp sp ..." (one pair per row, hex floats)
static void peakChecks(const char* path)
{
    FILE* f = std::fopen(path, "r");
    CHECK(f != nullptr, "cannot open %s", path);
    if (!f) return;
    char name[128];
    int rate = 0, rows = 0, cases = 0;
    long long n = 0;
    unsigned long long seed = 0;
    while (std::fscanf(f, " case %127s %d %d %lld %llu", name, &rate, &rows, &n, &seed) == 5) {
        std::vector<double> want((size_t)2 * rows);
        char tok[64];
        if (std::fscanf(f, " %63s", tok) != 1 || std::strcmp(tok, "want") != 0) { CHECK(false, "%s: no want line", name); break; }
        for (double& v : want) { if (std::fscanf(f, "%63s", tok) != 1) { CHECK(false, "%s: short", name); break; } v = std::strtod(tok, nullptr); }
        const int mask = progPeakMask((double)rate);
        CHECK(mask == (rate < 88200 ? 15 : rate < 176400 ? 5 : 0), "phases of %d", rate);
        const std::vector<double> x = caseRows(rows, n, seed);
        runSplit(x, rows, n, mask, { (int)n }, want.data(), name, "one call");
        for (int piece : { 1, 10, 11, 12, 4095, 4096, 4097 })
            if (piece < n && (piece > 12 || n <= 12)) runSplit(x, rows, n, mask, equalCalls(n, piece), want.data(), name, ("calls of " + std::to_string(piece)).c_str());
        std::mt19937 rng((unsigned)seed);
        for (int rep = n <= 4097 ? 0 : 1; rep < 3 && n > 1; ++rep) {       // rep 0: calls of 1 ... 20 samples
            std::vector<int> calls;
            long long left = n;
            while (left > 0) { const int len = (int)std::min<long long>(left, 1 + (int)(rng() % (rep == 0 ? 20u : 6000u))); calls.push_back(len); left -= len; }
            runSplit(x, rows, n, mask, calls, want.data(), name, "random split");
        }
        // the sequential pass behind cpq_loudness_peaks_host
        for (int r = 0; r < rows; ++r) {
            double st[kPeakState] = {};
            std::unique_ptr<double[]> row(new double[(size_t)n]);
            std::copy_n(x.data() + (size_t)r * (size_t)n, n, row.get());
            progPeakRowHost(row.get(), n, mask, st);
            CHECK(sameBits(st[kPeakTp], want[2 * r]) && sameBits(st[kPeakSp], want[2 * r + 1]), "%s row %d: the sequential pass", name, r);
        }
        ++cases;
    }
    std::fclose(f);
    CHECK(cases >= 24, "%d recorded cases", cases);
    std::printf("peaks: %d recorded cases\n", cases);
}

// k_prog_apply over its grid: blocks (x) of kApplyThreads lanes, rows (y)
static void applyKernel(const ApplyCall& c, const double* in, const double* gain, double* out)
{
    const int blocks = progApplyBlocks(c);
    CHECK(blocks >= 1 && blocks <= kApplyMaxBlocks, "%d blocks", blocks);
    for (int row = 0; row < c.rows; ++row)
        for (int bx = 0; bx < blocks; ++bx)
            for (int tid = 0; tid < kApplyThreads; ++tid) {
                const double g = gain[row >> 1];
                const double* x = in + (long long)row * c.inStride;
                double* y = out + (long long)row * c.outStride;
                const int step = blocks * kApplyThreads, first = bx * kApplyThreads + tid;
                if (c.wide) {
                    for (int i = first; i < (c.n >> 1); i += step) {
                        const double a = x[2 * i], b = x[2 * i + 1];
                        y[2 * i] = a * g;
                        y[2 * i + 1] = b * g;
                    }
                    if ((c.n & 1) && first == 0) y[c.n - 1] = x[c.n - 1] * g;
                } else {
                    for (int i = first; i < c.n; i += step) y[i] = x[i] * g;
                }
            }
}

static void applyChecks()
{
    std::mt19937 rng(5);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    int runs = 0;
    for (int S : { 1, 3 })
        for (int n : { 1, 2, 3, 255, 256, 257, 511, 513, 2 * kApplyThreads * kApplyMaxBlocks + 3 })
            for (int extraIn : { 0, 1, 2 })
                for (int extraOut : { 0, 1, 2 })
                    for (int inPlace = 0; inPlace < 2; ++inPlace) {
                        if (inPlace && extraIn != extraOut) continue;
                        if (n > 1000 && (S > 1 || extraIn + extraOut > 1)) continue;
                        ApplyCall c;
                        c.n = n; c.rows = 2 * S; c.inStride = n + extraIn; c.outStride = n + extraOut;
                        c.wide = c.inStride % 2 == 0 && c.outStride % 2 == 0;
                        const size_t nin = (size_t)(c.rows - 1) * (size_t)c.inStride + (size_t)n, nout = (size_t)(c.rows - 1) * (size_t)c.outStride + (size_t)n;
                        std::unique_ptr<double[]> in(new double[nin]), out(new double[nout]), gain(new double[(size_t)S]), ref(new double[nin]);
                        for (size_t i = 0; i < nin; ++i) in[i] = ref[i] = u(rng);
                        for (size_t i = 0; i < nout; ++i) out[i] = 77.0;
                        for (int s = 0; s < S; ++s) gain[s] = 0.3 + 0.2 * s;
                        CHECK(!progApplyOverlap(1000, c.inStride, inPlace ? 1000 : 1000 + nin, c.outStride, c.rows, n), "no overlap");
                        applyKernel(c, in.get(), gain.get(), inPlace ? in.get() : out.get());
                        const double* got = inPlace ? in.get() : out.get();
                        bool ok = true;
                        for (int r = 0; r < c.rows; ++r)
                            for (int i = 0; i < n; ++i)
                                ok = ok && sameBits(got[(size_t)r * (size_t)c.outStride + (size_t)i], ref[(size_t)r * (size_t)c.inStride + (size_t)i] * gain[r >> 1]);
                        // what lies between the rows is as it was
                        for (int r = 0; r + 1 < c.rows; ++r)
                            for (long long i = n; i < c.outStride; ++i)
                                ok = ok && sameBits(got[(size_t)r * (size_t)c.outStride + (size_t)i], inPlace ? ref[(size_t)r * (size_t)c.inStride + (size_t)i] : 77.0);
                        CHECK(ok, "apply: %d streams, n %d, strides %lld %lld, in place %d", S, n, c.inStride, c.outStride, inPlace);
                        ++runs;
                    }
    std::printf("apply: %d geometries\n", runs);
    CHECK(progApplyOverlap(1000, 10, 1004, 10, 4, 8) && progApplyOverlap(1000, 10, 1000, 12, 4, 8) && progApplyOverlap(1037, 10, 1000, 10, 4, 8),
          "rows that overlap in part");
    CHECK(!progApplyOverlap(1000, 10, 1000, 10, 4, 8) && !progApplyOverlap(1000, 10, 1038, 10, 4, 8) && !progApplyOverlap(1038, 10, 1000, 10, 4, 8),
          "the same rows, and rows apart");
}

static void gainChecks()
{
    bool lim = true;
    const double loud = progGainLimited(-20.0, 0.1, -23.0, -1.0, lim);
    CHECK(!lim && sameBits(loud, std::pow(10.0, -3.0 / 20.0)), "the loudness gain wins");
    const double peak = progGainLimited(-30.0, 0.9, -23.0, -1.0, lim);
    CHECK(lim && sameBits(peak, std::pow(10.0, -1.0 / 20.0) / 0.9), "the ceiling wins");
    const double free_ = progGainLimited(-30.0, 0.0, -23.0, -1.0, lim);
    CHECK(!lim && sameBits(free_, std::pow(10.0, 7.0 / 20.0)), "peak == 0 sets no limit");
    for (int p = 0; p < 4; ++p)
        for (int k = 0; k < kPeakTaps; ++k) CHECK(sameBits(progPeakCoef(p, k), progPeakCoef(3 - p, kPeakTaps - 1 - k)), "phase %d reversed", p);
    CHECK(kPeakBufDoubles == progPeakPad(kPeakHist + kPeakTile - 1) + 1 && kPeakWindow == 19 && kPeakTile == 4096, "the tile");
}

int main(int argc, char** argv)
{
    gainChecks();
    applyChecks();
    if (argc > 1) peakChecks(argv[1]);
    else CHECK(false, "usage: prog_peak_check tests/golden/prog_peak_cases.txt");
    std::printf("%d checks\n%d failed checks\n", checks, failed);
    return failed ? 1 : 0;
}
