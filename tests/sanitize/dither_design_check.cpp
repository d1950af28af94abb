// Stand-alone check of the dither stage's host code (convopeq_amd/csrc/dither_design.cpp), built with the address and
// undefined-behaviour sanitizers and run as a program of its own: the design and its refusals, the seeds, and DitherHost on
// exactly-sized heap rows -- against the reference's recorded codes when a dump of the fixture is given
// (argv[1]: the cases as text, written by tests/test_dither_model_cpu.py), split invariance, reset and prepare.
//   case <shaper> <bits> <rate> <n1> <n2>, then 2 n input doubles as hex bit patterns, then 2 n expected outputs likewise
#include "host_design.hpp"

#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static int failed = 0;
#define CHECK(c) do { if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static bool sameBitsOrNan(const std::vector<double>& a, const std::vector<double>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (std::isnan(a[i]) != std::isnan(b[i])) return false;
        if (!std::isnan(a[i]) && std::memcmp(&a[i], &b[i], sizeof(double)) != 0) return false;
    }
    return true;
}

static bool readDoubles(FILE* f, std::vector<double>& v)
{
    for (auto& x : v) {
        uint64_t bits;
        if (std::fscanf(f, "%" SCNx64, &bits) != 1) return false;
        std::memcpy(&x, &bits, sizeof(x));
    }
    return true;
}

static std::vector<double> noise(int n, unsigned seed, double amp)
{
    std::vector<double> v((size_t)n);
    unsigned s = seed;
    for (auto& x : v) { s = s * 1664525u + 1013904223u; x = amp * ((double)(s >> 8) / 8388608.0 - 1.0); }
    return v;
}

int main(int argc, char** argv)
{
    {   // design: refusals, presets, interpolation, the 4-tap sum check
        double c[16], sc;
        CHECK(!cpq::ditherDesign(48000.0, 0, 16, c, &sc) && !cpq::ditherDesign(48000.0, 3, 16, c, &sc));
        CHECK(!cpq::ditherDesign(48000.0, CPQ_DITHER_FIXED4, 0, c, &sc) && !cpq::ditherDesign(48000.0, CPQ_DITHER_FIXED15, 33, c, &sc));
        CHECK(cpq_dither_design(48000.0, CPQ_DITHER_FIXED4, 16, nullptr, &sc) == CPQ_ERR_INVALID_ARG);
        CHECK(cpq_dither_design(48000.0, CPQ_DITHER_FIXED4, 16, c, nullptr) == CPQ_ERR_INVALID_ARG);
        CHECK(cpq_dither_design(48000.0, 7, 16, c, &sc) == CPQ_ERR_INVALID_ARG);
        CHECK(cpq_dither_design(48000.0, CPQ_DITHER_FIXED4, 16, c, &sc) == CPQ_OK);
        CHECK(c[0] == 0.46 && c[3] == 0.09 && c[4] == 0.0 && c[15] == 0.0 && sc == 1.0 / 32768.0);
        CHECK(cpq::ditherDesign(44100.0, CPQ_DITHER_FIXED4, 24, c, &sc) && c[0] == 0.46 && sc == 1.0 / 8388608.0);     // refused set
        CHECK(cpq::ditherDesign(96000.0, CPQ_DITHER_FIXED4, 1, c, &sc) && c[0] == 0.742333 && sc == 1.0);
        CHECK(cpq::ditherDesign(1.0e6, CPQ_DITHER_FIXED15, 32, c, &sc) && c[0] == 0.390229 && c[14] == 0.152692 && c[15] == 0.0);
        CHECK(cpq::ditherDesign(10.0, CPQ_DITHER_FIXED15, 16, c, &sc) && c[0] == 2.157553);
        CHECK(cpq::ditherDesign(std::nan(""), CPQ_DITHER_FIXED15, 16, c, &sc) && c[0] == 2.157553);
        CHECK(cpq::ditherDesign(64000.0, CPQ_DITHER_FIXED15, 16, c, &sc) && c[0] < 2.172009 && c[0] > 1.458665);
        unsigned long long s[4], t[4];
        cpq::ditherSeed(CPQ_DITHER_FIXED4, 48000.0, 16, 0, s);
        CHECK(s[0] == 0x123456789ABCDEF0ULL);
        cpq::ditherSeed(CPQ_DITHER_FIXED4, 96000.0, 24, 1, t);
        CHECK(t[0] == 0x89ABCDEF01234567ULL);
        cpq::ditherSeed(CPQ_DITHER_FIXED15, 48000.0, 16, 0, s);
        cpq::ditherSeed(CPQ_DITHER_FIXED15, 48000.0, 24, 0, t);
        CHECK(std::memcmp(s, t, sizeof(s)) != 0);
        cpq::ditherSeed(CPQ_DITHER_FIXED15, -1.0, 16, 0, t);
        CHECK(std::memcmp(s, t, sizeof(s)) == 0);                   // a rate that is not positive seeds as 48 kHz
    }
    int cases = 0;
    if (argc > 1) {     // the reference's recorded outputs
        FILE* f = std::fopen(argv[1], "r");
        CHECK(f != nullptr);
        int shaper, bits, n1, n2;
        double rate;
        while (f && std::fscanf(f, " case %d %d %lf %d %d", &shaper, &bits, &rate, &n1, &n2) == 5) {
            const size_t n = (size_t)n1 + (size_t)n2;
            std::vector<double> in(2 * n), want(2 * n);
            if (!readDoubles(f, in) || !readDoubles(f, want)) { CHECK(!"short case"); break; }
            cpq::DitherHost h;
            CHECK(h.configure(rate, shaper, bits));
            std::vector<double> l1(in.begin(), in.begin() + n1), l2(in.begin() + n1, in.begin() + n);         // exact sizes
            std::vector<double> r1(in.begin() + n, in.begin() + n + n1), r2(in.begin() + n + n1, in.end());
            h.process(l1.data(), r1.data(), n1, cpq::kOutHeadroom);
            h.process(l2.data(), r2.data(), n2, cpq::kOutHeadroom);
            std::vector<double> got;
            for (auto* v : { &l1, &l2, &r1, &r2 }) got.insert(got.end(), v->begin(), v->end());
            const bool same = sameBitsOrNan(got, want);
            if (!same) std::printf("case %d %d %g differs\n", shaper, bits, rate);
            CHECK(same);
            ++cases;
        }
        if (f) std::fclose(f);
        CHECK(cases > 0);
    }
    for (int shaper : { CPQ_DITHER_FIXED4, CPQ_DITHER_FIXED15 }) {
        const int n = 777;
        const std::vector<double> l = noise(n, 1u, 0.5), r = noise(n, 2u, 1.3);
        cpq::DitherHost ref;
        CHECK(ref.configure(48000.0, shaper, 16));
        std::vector<double> rl = l, rr = r;
        ref.process(rl.data(), rr.data(), n, 1.0);
        for (int i = 0; i < n; ++i) CHECK(rl[i] * 32768.0 == std::nearbyint(rl[i] * 32768.0) && std::fabs(rl[i]) <= 1.0 + 1.0 / 32768.0);
        for (int cut : { 1, 63, 64, 65 }) {         // split invariance
            cpq::DitherHost st;
            st.configure(48000.0, shaper, 16);
            std::vector<double> yl, yr;
            for (int o = 0; o < n; o += cut) {
                const int len = std::min(cut, n - o);
                std::vector<double> bl(l.begin() + o, l.begin() + o + len), br(r.begin() + o, r.begin() + o + len);
                st.process(bl.data(), br.data(), len, 1.0);
                yl.insert(yl.end(), bl.begin(), bl.end());
                yr.insert(yr.end(), br.begin(), br.end());
            }
            CHECK(sameBitsOrNan(yl, rl) && sameBitsOrNan(yr, rr));
            CHECK(std::memcmp(st.err, ref.err, sizeof(st.err)) == 0 && std::memcmp(st.rng, ref.rng, sizeof(st.rng)) == 0);
        }
        // reset clears the errors and leaves the generators; prepare reseeds the 15-tap shaper only
        cpq::DitherHost a;
        a.configure(48000.0, shaper, 16);
        unsigned long long fresh[2][4];
        std::memcpy(fresh, a.rng, sizeof(fresh));
        std::vector<double> z(50, 0.0), z2(50, 0.0);
        a.process(z.data(), z2.data(), 50, 1.0);
        bool any = false;
        for (double v : z) any = any || v != 0.0;
        CHECK(any && std::memcmp(z.data(), z2.data(), 50 * sizeof(double)) != 0);      // the pure dither pattern, L unlike R
        CHECK(a.err[0][0] != 0.0 && std::memcmp(fresh, a.rng, sizeof(fresh)) != 0);
        unsigned long long run[2][4];
        std::memcpy(run, a.rng, sizeof(run));
        a.reset();
        CHECK(a.err[0][0] == 0.0 && a.err[1][3] == 0.0 && std::memcmp(run, a.rng, sizeof(run)) == 0);
        a.prepare(48000.0);
        CHECK((std::memcmp(fresh, a.rng, sizeof(fresh)) == 0) == (shaper == CPQ_DITHER_FIXED15));
        a.process(nullptr, nullptr, 0, 1.0);
        a.process(nullptr, nullptr, -2, 1.0);
    }
    std::printf("dither_design_check: %d cases, %d failed checks\n", cases, failed);
    return failed ? 1 : 0;
}
