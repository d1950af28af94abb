// Stand-alone check of the output stage's host code (convopeq_amd/csrc/out_design.cpp), built with the address and
// undefined-behaviour sanitizers and run as a program of its own: design and fallbacks, the scan tables, and OutStageHost on
// exactly-sized heap rows -- split invariance, the state guards, the scrub, the limiter's attack and release, the clamp.
#include "host_design.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int failed = 0;
#define CHECK(c) do { if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::vector<double> noise(int n, unsigned seed, double amp, double dcOffset)
{
    std::vector<double> v((size_t)n);
    unsigned s = seed;
    for (auto& x : v) { s = s * 1664525u + 1013904223u; x = dcOffset + amp * ((double)(s >> 8) / 8388608.0 - 1.0); }
    return v;
}

static bool sameBits(const std::vector<double>& a, const std::vector<double>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    {   // design
        double a[2], r;
        cpq::outDesign(48000.0, a, &r);
        CHECK(a[0] > 0.0 && a[0] < a[1] && a[1] < 1.0e-3);
        CHECK(std::fabs(a[0] - 2.0 * 3.14159265358979323846 * 2.7 / 48000.0) < 1.0e-7);
        CHECK(std::fabs(r - std::exp(-1.0 / 4800.0)) == 0.0);
        for (double bad : { 0.0, -48000.0, nan, inf, -inf }) {
            cpq::outDesign(bad, a, &r);
            CHECK(a[0] == 1.0e-6 && a[1] == 1.0e-6);
            CHECK(r == (bad == inf ? 1.0 : 0.0));
        }
        int32_t rc = cpq_out_design(48000.0, nullptr, &r);
        CHECK(rc == CPQ_ERR_INVALID_ARG);
        rc = cpq_out_design(48000.0, a, nullptr);
        CHECK(rc == CPQ_ERR_INVALID_ARG);
        CHECK(cpq_out_design(44100.0, a, &r) == CPQ_OK);
    }
    {   // tables: powers of a = 1 - alpha
        std::vector<double> t((size_t)cpq::kOutSectionDoubles);
        const double alpha = 3.5e-4;
        cpq::outSectionTable(alpha, t.data());
        CHECK(t[0] == alpha);
        for (int k = 0; k < cpq::kOutScanSteps; ++k)
            CHECK(std::fabs(t[1 + k] - (double)std::pow(1.0L - (long double)alpha, 8.0L * (1 << k))) < 2.5e-16);
        CHECK(t[1 + cpq::kOutScanSteps] == 1.0);
        for (int l = 0; l < 64; ++l) CHECK(std::fabs(t[1 + cpq::kOutScanSteps + l] - (double)std::pow(1.0L - (long double)alpha, 8.0L * l)) < 2.5e-16);
    }
    const int n = 3001;
    for (double rate : { 8000.0, 44100.0, 48000.0 }) {
        // one callback against callbacks of 64 / 441 / 512: bit-equal (no guard trips, the limiter has no callback)
        const std::vector<double> l = noise(n, 1u, 1.4, 0.3), r = noise(n, 2u, 0.7, -0.2);
        cpq::OutStageHost ref;
        ref.prepare(rate);
        std::vector<double> rl = l, rr = r;
        ref.process(rl.data(), rr.data(), n, CPQ_OUT_ALL);
        bool limited = false;
        for (int i = 0; i < n; ++i) {
            CHECK(std::fabs(rl[i]) <= cpq::kOutHeadroom && std::fabs(rr[i]) <= cpq::kOutHeadroom);
            limited = limited || std::fabs(rl[i]) > 0.5;
        }
        CHECK(limited && ref.envelope < 1.0);
        for (int cb : { 64, 441, 512, 1 }) {
            cpq::OutStageHost st;
            st.prepare(rate);
            std::vector<double> yl, yr;
            for (int o = 0; o < n; o += cb) {
                const int len = std::min(cb, n - o);
                std::vector<double> bl(l.begin() + o, l.begin() + o + len), br(r.begin() + o, r.begin() + o + len);   // exact size
                st.process(bl.data(), br.data(), len, CPQ_OUT_ALL);
                yl.insert(yl.end(), bl.begin(), bl.end());
                yr.insert(yr.end(), br.begin(), br.end());
            }
            CHECK(sameBits(yl, rl) && sameBits(yr, rr));
            CHECK(st.envelope == ref.envelope && st.dc[0][0] == ref.dc[0][0] && st.dc[1][1] == ref.dc[1][1]);
        }
    }
    {   // zeros stay zeros; n <= 0 touches nothing
        cpq::OutStageHost st;
        st.prepare(48000.0);
        std::vector<double> z(100, 0.0), z2(100, 0.0);
        st.process(z.data(), z2.data(), 100, CPQ_OUT_ALL);
        for (double v : z) CHECK(v == 0.0 && !std::signbit(v));
        st.process(nullptr, nullptr, 0, CPQ_OUT_ALL);
        st.process(nullptr, nullptr, -3, CPQ_OUT_ALL);
        CHECK(st.envelope == 1.0);
    }
    {   // guards: a NaN callback and a 1e16 callback reset the DC states; the scrub writes zeros
        cpq::OutStageHost st;
        st.prepare(48000.0);
        std::vector<double> a(512, 0.25), b(512, 0.25);
        a[100] = nan;
        st.process(a.data(), b.data(), 512, CPQ_OUT_DC_BLOCK | CPQ_OUT_HEADROOM);
        CHECK(st.dc[0][0] == 0.0 && st.dc[0][1] == 0.0 && st.dc[1][0] != 0.0);
        for (int i = 100; i < 512; ++i) CHECK(a[i] == 0.0);
        CHECK(a[99] != 0.0);
        std::vector<double> c(512, 1.0e16), d(512, 0.0);
        st.reset();
        st.process(c.data(), d.data(), 512, CPQ_OUT_DC_BLOCK);
        CHECK(st.dc[0][0] == 0.0 && st.dc[1][0] == 0.0);
        std::vector<double> e = { inf, -inf, 1.0e300 / cpq::kOutHeadroom * 1.01, 0.99e300, -0.0 }, f(5, 0.0);
        st.reset();
        st.process(e.data(), f.data(), 5, CPQ_OUT_HEADROOM);
        CHECK(e[0] == 0.0 && e[1] == 0.0 && e[2] == 0.0 && e[3] == 0.99e300 * cpq::kOutHeadroom && std::signbit(e[4]));
    }
    {   // limiter: immediate attack, release stalls at a fixed point just below 1.0 and stays there
        cpq::OutStageHost st;
        st.prepare(8000.0);
        std::vector<double> l(40000, 0.0), r(40000, 0.0);
        l[0] = 2.0;
        st.process(l.data(), r.data(), 1, CPQ_OUT_LIMITER);
        CHECK(st.envelope == cpq::kOutLimiterThreshold / 2.0 && l[0] == 2.0 * st.envelope);
        st.process(l.data() + 1, r.data() + 1, 39999, CPQ_OUT_LIMITER);
        const double e = st.envelope;
        CHECK(e < 1.0 && 1.0 - e < 1.0e-12 && 1.0 + (e - 1.0) * st.releaseCoeff == e);
        CHECK(cpq::outDesiredGain(0.0, 0.0) == 1.0 && cpq::outDesiredGain(nan, 0.1) == 1.0);
        CHECK(cpq::outClamp(nan) == -cpq::kOutHeadroom && cpq::outClamp(2.0) == cpq::kOutHeadroom && cpq::outClamp(-inf) == -cpq::kOutHeadroom);
    }
    std::printf("out_design_check: %d failed checks\n", failed);
    return failed ? 1 : 0;
}
