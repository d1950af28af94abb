// Stand-alone check of the soft clipper's host code (convopeq_amd/csrc/softclip_design.cpp and the two arithmetic paths of
// softclip_design.hpp), built with the address and undefined-behaviour sanitizers and run as a program of its own: the
// parameter formulas and refusals, the table row, the block walk on exactly-sized heap rows -- which path a sample takes, the
// ragged last callback, a resting stream -- and the curve: identity below the clip start, continuity at its three corners,
// bounded output, the sign asymmetry, NaN and infinities.
#include "softclip_design.hpp"

#include "convopeq_mi355x.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int failed = 0;
#define CHECK(c) do { if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::vector<double> noise(int n, unsigned seed, double amp)
{
    std::vector<double> v((size_t)n);
    unsigned s = seed;
    for (auto& x : v) { s = s * 1664525u + 1013904223u; x = amp * ((double)(s >> 8) / 8388608.0 - 1.0); }
    return v;
}

static bool sameBits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0 || (std::isnan(a) && std::isnan(b)); }

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int T = cpq::kSoftClipTabDoubles;
    {   // parameters and refusals
        double t = -1.0, k = -1.0, a = -1.0;
        CHECK(cpq_soft_clip_params(0.0f, &t, &k, &a) == CPQ_OK && t == 0.95 && k == 0.05 && a == 0.0);
        CHECK(cpq_soft_clip_params(1.0f, &t, &k, &a) == CPQ_OK && t == 0.95 - 0.45 && k == 0.05 + 0.35 && a == 0.10);
        const double sat = (double)0.2f;
        CHECK(cpq_soft_clip_params(0.2f, &t, &k, &a) == CPQ_OK && t == 0.95 - 0.45 * sat && k == 0.05 + 0.35 * sat && a == 0.10 * sat);
        t = k = a = -1.0;
        for (float bad : { -0.001f, 1.001f, (float)nan, (float)inf, -(float)inf, -1.0f, 2.0f })
            CHECK(cpq_soft_clip_params(bad, &t, &k, &a) == CPQ_ERR_INVALID_ARG && !cpq::softClipAmountValid(bad));
        CHECK(t == -1.0 && k == -1.0 && a == -1.0);
        CHECK(cpq_soft_clip_params(0.5f, nullptr, &k, &a) == CPQ_ERR_INVALID_ARG);
        CHECK(cpq_soft_clip_params(0.5f, &t, nullptr, &a) == CPQ_ERR_INVALID_ARG);
        CHECK(cpq_soft_clip_params(0.5f, &t, &k, nullptr) == CPQ_ERR_INVALID_ARG);
        double one = 2.0;
        CHECK(cpq_soft_clip_host(nullptr, 1, 1, 0.5f) == CPQ_ERR_INVALID_ARG);
        CHECK(cpq_soft_clip_host(&one, 0, 1, 0.5f) == CPQ_ERR_INVALID_ARG && cpq_soft_clip_host(&one, 1, 0, 0.5f) == CPQ_ERR_INVALID_ARG);
        CHECK(cpq_soft_clip_host(&one, 1, 1, 1.5f) == CPQ_ERR_INVALID_ARG && one == 2.0);
        CHECK(cpq_soft_clip_latency(1) == 15.0);
        for (int f : { 0, 2, 3, 4, 8, 16, -1 }) CHECK(cpq_soft_clip_latency(f) == 0.0);
    }
    for (float amount : { 0.0f, 0.2f, 0.5f, 1.0f }) {
        std::vector<double> row((size_t)T);
        cpq::softClipTableRow(true, amount, row.data());
        const double thr = row[cpq::kScThreshold], knee = row[cpq::kScKnee], start = row[cpq::kScClipStart];
        CHECK(row[cpq::kScOn] == 1.0 && start == thr - knee && row[cpq::kScKneeEnd] == thr + knee);
        CHECK(row[cpq::kScRecipKnee] == 1.0 / knee && row[cpq::kScRecipKnee2] == 1.0 / (2.0 * knee));
        // identity up to the clip start, both paths, both signs; NaN passes; infinities become NaN
        for (double v : { 0.0, -0.0, 5.0e-324, 1.0e-310, 0.5 * start, std::nextafter(start, 0.0), start }) {
            for (double s : { 1.0, -1.0 }) {
                CHECK(sameBits(cpq::softClipBody(s * v, row.data()), s * v));
                CHECK(sameBits(cpq::softClipTail(s * v, row.data()), s * v));
            }
        }
        CHECK(std::isnan(cpq::softClipBody(nan, row.data())) && std::isnan(cpq::softClipTail(nan, row.data())));
        for (double v : { inf, -inf }) CHECK(std::isnan(cpq::softClipBody(v, row.data())) && std::isnan(cpq::softClipTail(v, row.data())));
        // continuity at the three corners, and the two paths within a few ulps of each other over the curve
        for (double c : { start, thr, thr + knee })
            for (int path = 0; path < 2; ++path) {
                auto f = [&](double v) { return path ? cpq::softClipTail(v, row.data()) : cpq::softClipBody(v, row.data()); };
                CHECK(std::fabs(f(std::nextafter(c, 4.0)) - f(std::nextafter(c, 0.0))) < 1.0e-14);
            }
        bool differ = false;
        for (int i = 0; i <= 4000; ++i) {
            const double v = 0.001 * i;
            const double b = cpq::softClipBody(v, row.data()), t = cpq::softClipTail(v, row.data());
            // the same curve rounded differently up to a tanh argument of 4.5; from there the scalar tanh is 1, the vector one its Pade value
            if ((v - thr) / knee < 4.5) CHECK(std::fabs(b - t) <= 1.0e-15);
            else CHECK(t == thr + knee && b < t && t - b < 1.0e-3 * knee);
            differ = differ || b != t;
            CHECK(b >= 0.0 && b <= thr + knee && (v < thr || b <= v));    // never above threshold + knee; above the threshold never louder than the input
            const double nb = cpq::softClipBody(-v, row.data());
            CHECK(nb <= 0.0 && -nb <= b && -nb >= b * (1.0 - row[cpq::kScAsym]) - 1.0e-15);   // the negative half is scaled down by at most the asymmetry
        }
        CHECK(differ);
        CHECK(cpq::softClipTail(100.0, row.data()) == thr + knee);  // tanh = 1 from 4.5 on: the scalar path reaches the ceiling ...
        CHECK(cpq::softClipBody(100.0, row.data()) < thr + knee);   // ... the body's clamped Pade value stays below it
        // the walk: exactly-sized rows, every callback length, against the per-sample functions
        for (int n : { 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 441, 883 })
            for (int cb : { 1, 2, 3, 4, 5, 7, 8, 64, 441, 882, 2048 }) {
                const std::vector<double> x = noise(n, 7u + (unsigned)n, 2.0);
                std::vector<double> y = x;
                CHECK(cpq_soft_clip_host(y.data(), n, cb, amount) == CPQ_OK);
                for (int i = 0; i < n; ++i) {
                    const int o = i / cb * cb, len = n - o < cb ? n - o : cb, k = i - o;
                    const double want = k < len / 4 * 4 ? cpq::softClipBody(x[(size_t)i], row.data()) : cpq::softClipTail(x[(size_t)i], row.data());
                    CHECK(sameBits(y[(size_t)i], want));
                    CHECK(sameBits(want, cpq::softClipSample(x[(size_t)i], k, len, row.data())));
                }
            }
    }
    {   // rows of two streams with a stride, the second stream resting; n <= 0 and a null table touch nothing
        const int n = 37, stride = 41, nCh = 4;
        std::vector<double> tab((size_t)(2 * T));
        cpq::softClipTableRow(true, 0.5f, tab.data());
        cpq::softClipTableRow(false, 1.0f, tab.data() + T);
        std::vector<double> rows((size_t)((nCh - 1) * stride + n));          // the last row ends with its last sample
        const std::vector<double> src = noise((int)rows.size(), 99u, 2.0);
        rows = src;
        cpq::softClipRows(rows.data(), stride, nCh, n, 8, tab.data());
        bool changed = false;
        for (int c = 0; c < nCh; ++c)
            for (int i = 0; i < stride && c * stride + i < (int)rows.size(); ++i) {
                const size_t at = (size_t)(c * stride + i);
                if (c >= 2 || i >= n) CHECK(sameBits(rows[at], src[at]));
                else {
                    const int o = i / 8 * 8, len = n - o < 8 ? n - o : 8;
                    CHECK(sameBits(rows[at], cpq::softClipSample(src[at], i - o, len, tab.data())));
                    changed = changed || rows[at] != src[at];
                }
            }
        CHECK(changed);
        rows = src;
        cpq::softClipRows(rows.data(), stride, nCh, 0, 8, tab.data());
        cpq::softClipRows(rows.data(), stride, nCh, -5, 8, tab.data());
        cpq::softClipRows(rows.data(), stride, nCh, n, 0, tab.data());
        cpq::softClipRows(nullptr, stride, nCh, n, 8, tab.data());
        cpq::softClipRows(rows.data(), stride, nCh, n, 8, nullptr);
        CHECK(std::memcmp(rows.data(), src.data(), rows.size() * sizeof(double)) == 0);
    }
    std::printf("softclip_design_check: %d failed checks\n", failed);
    return failed ? 1 : 0;
}
