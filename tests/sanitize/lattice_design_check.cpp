// Stand-alone check of the adaptive shaper's host code (convopeq_amd/csrc/dither_design.cpp: the design, ditherClampAdaptive,
// DitherHost's lattice path and setAdaptiveCoeffs), built with the address and undefined-behaviour sanitizers and run as a
// program of its own on exactly-sized heap rows -- against expected rows when a dump is given (argv[1]: the cases as text,
// written by tests/test_lattice_model_cpu.py), then split invariance, reset, prepare and the refusals.
//   case <bits> <n1> <n2> <nA> <nB>   (nB < 0: no second set), then nA and nB coefficients, 2 n input doubles and 2 n expected
//   outputs, all as hex bit patterns
#include "host_design.hpp"

#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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
    const double def[9] = { -0.003796, -0.006752, 0.008418, -0.010546, 0.004716, -0.007624, -0.020750, -0.002049, -0.003632 };
    const double strong[9] = { 0.82, -0.68, 0.55, -0.43, 0.33, -0.25, 0.18, -0.12, 0.07 };
    {   // design, clamp, seeds
        double c[16], sc;
        CHECK(cpq::ditherOrder(CPQ_DITHER_ADAPTIVE9) == 9 && cpq::ditherOrder(3) == 0 && CPQ_DITHER_ADAPTIVE9 == 4);
        CHECK(!cpq::ditherDesign(48000.0, 3, 16, c, &sc) && !cpq::ditherDesign(48000.0, CPQ_DITHER_ADAPTIVE9, 0, c, &sc));
        CHECK(!cpq::ditherDesign(48000.0, CPQ_DITHER_ADAPTIVE9, 33, c, &sc));
        CHECK(cpq_dither_design(48000.0, CPQ_DITHER_ADAPTIVE9, 16, nullptr, &sc) == CPQ_ERR_INVALID_ARG);
        for (double rate : { 44100.0, 1.0e6, -3.0, std::nan("") }) {       // the rate is ignored
            for (auto& v : c) v = 7.0;
            CHECK(cpq_dither_design(rate, CPQ_DITHER_ADAPTIVE9, 24, c, &sc) == CPQ_OK && sc == 1.0 / 8388608.0);
            CHECK(std::memcmp(c, def, sizeof(def)) == 0);
            for (int i = 9; i < 16; ++i) CHECK(c[i] == 0.0);
        }
        const double odd[6] = { 1.5, -3.0, std::nan(""), std::numeric_limits<double>::infinity(), 0.25, -0.125 };
        std::vector<double> heap(odd, odd + 6);                             // exactly six: a read past n is a sanitizer report
        double k[9];
        cpq::ditherClampAdaptive(heap.data(), 6, k);
        const double want[9] = { 0.85, -0.85, 0.0, 0.0, 0.25, -0.125, 0.0, 0.0, 0.0 };
        CHECK(std::memcmp(k, want, sizeof(want)) == 0);
        cpq::ditherClampAdaptive(nullptr, 0, k);
        for (double v : k) CHECK(v == 0.0);
        unsigned long long s[4], t[4];
        cpq::ditherSeed(CPQ_DITHER_ADAPTIVE9, 48000.0, 16, 0, s);
        cpq::ditherSeed(CPQ_DITHER_FIXED4, 96000.0, 24, 0, t);
        CHECK(s[0] == 0x123456789ABCDEF0ULL && std::memcmp(s, t, sizeof(s)) == 0);
        cpq::ditherSeed(CPQ_DITHER_ADAPTIVE9, 48000.0, 16, 1, s);
        CHECK(s[0] == 0x89ABCDEF01234567ULL);
    }
    int cases = 0;
    if (argc > 1) {
        FILE* f = std::fopen(argv[1], "r");
        CHECK(f != nullptr);
        int bits, n1, n2, nA, nB;
        while (f && std::fscanf(f, " case %d %d %d %d %d", &bits, &n1, &n2, &nA, &nB) == 5) {
            const size_t n = (size_t)n1 + (size_t)n2;
            std::vector<double> a((size_t)nA), b((size_t)(nB < 0 ? 0 : nB)), in(2 * n), want(2 * n);
            if (!readDoubles(f, a) || !readDoubles(f, b) || !readDoubles(f, in) || !readDoubles(f, want)) { CHECK(!"short case"); break; }
            cpq::DitherHost h;
            CHECK(h.configure(48000.0, CPQ_DITHER_ADAPTIVE9, bits));
            CHECK(h.setAdaptiveCoeffs(a.data(), nA));
            std::vector<double> l1(in.begin(), in.begin() + n1), l2(in.begin() + n1, in.begin() + n);         // exact sizes
            std::vector<double> r1(in.begin() + n, in.begin() + n + n1), r2(in.begin() + n + n1, in.end());
            h.process(l1.data(), r1.data(), n1, cpq::kOutHeadroom);
            if (nB >= 0) CHECK(h.setAdaptiveCoeffs(b.data(), nB));
            h.process(l2.data(), r2.data(), n2, cpq::kOutHeadroom);
            std::vector<double> got;
            for (auto* v : { &l1, &l2, &r1, &r2 }) got.insert(got.end(), v->begin(), v->end());
            const bool same = sameBitsOrNan(got, want);
            if (!same) std::printf("case %d (%d) differs\n", cases, bits);
            CHECK(same);
            for (int ch = 0; ch < 2; ++ch)
                for (int i = 0; i < 9; ++i) CHECK(std::fabs(h.err[ch][i]) <= 2.0);     // a NaN fails this too
            ++cases;
        }
        if (f) std::fclose(f);
        CHECK(cases > 0);
    }
    {
        const int n = 777;
        const std::vector<double> l = noise(n, 1u, 0.5), r = noise(n, 2u, 1.3);
        cpq::DitherHost ref;
        CHECK(ref.configure(48000.0, CPQ_DITHER_ADAPTIVE9, 16) && std::memcmp(ref.coeffs, def, sizeof(def)) == 0);
        CHECK(ref.setAdaptiveCoeffs(strong, 9));
        std::vector<double> rl = l, rr = r;
        ref.process(rl.data(), rr.data(), n, 1.0);
        for (int i = 0; i < n; ++i) CHECK(rl[i] * 32768.0 == std::nearbyint(rl[i] * 32768.0) && rl[i] >= -1.0 && rl[i] <= 1.0 - 1.0 / 32768.0);
        for (int cut : { 1, 63, 64, 65 }) {         // split invariance
            cpq::DitherHost st;
            st.configure(48000.0, CPQ_DITHER_ADAPTIVE9, 16);
            st.setAdaptiveCoeffs(strong, 9);
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
        // reset and prepare clear the states, keep the coefficients and leave the generators; a new set clears the states too
        unsigned long long run[2][4];
        std::memcpy(run, ref.rng, sizeof(run));
        CHECK(ref.err[0][0] != 0.0 && ref.err[1][8] != 0.0);
        ref.reset();
        CHECK(ref.err[0][0] == 0.0 && ref.err[1][8] == 0.0 && std::memcmp(run, ref.rng, sizeof(run)) == 0 && ref.coeffs[0] == 0.82);
        std::vector<double> z(50, 0.0), z2(50, 0.0);
        ref.process(z.data(), z2.data(), 50, 1.0);
        CHECK(ref.err[0][0] != 0.0);
        std::memcpy(run, ref.rng, sizeof(run));
        ref.prepare(96000.0);
        CHECK(ref.err[0][0] == 0.0 && std::memcmp(run, ref.rng, sizeof(run)) == 0 && std::memcmp(ref.coeffs, strong, sizeof(strong)) == 0);
        ref.process(z.data(), z2.data(), 50, 1.0);
        CHECK(ref.setAdaptiveCoeffs(def, 3) && ref.err[0][0] == 0.0 && ref.coeffs[2] == def[2] && ref.coeffs[3] == 0.0 && ref.coeffs[8] == 0.0);
        CHECK(!ref.setAdaptiveCoeffs(def, 10) && !ref.setAdaptiveCoeffs(def, -1) && !ref.setAdaptiveCoeffs(nullptr, 1));
        CHECK(ref.setAdaptiveCoeffs(nullptr, 0) && ref.coeffs[0] == 0.0);
        cpq::DitherHost fixed;
        fixed.configure(48000.0, CPQ_DITHER_FIXED4, 16);
        CHECK(!fixed.setAdaptiveCoeffs(def, 9) && fixed.coeffs[0] == 0.46);
        ref.process(nullptr, nullptr, 0, 1.0);
        ref.process(nullptr, nullptr, -2, 1.0);
    }
    std::printf("lattice_design_check: %d cases, %d failed checks\n", cases, failed);
    return failed ? 1 : 0;
}
