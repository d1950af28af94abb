// Records what the reference's own FixedNoiseShaper / Fixed15TapNoiseShaper compute, for tests/golden/dither_ref.npz
// (make_dither_ref.py drives it).  Build, with REF the reference's source tree:
//   g++ -std=c++20 -O2 -ffp-contract=off -msse4.1 -mavx2 -Itests/golden/juce_shim -I$REF/src tests/golden/dither_probe.cpp -o dither_probe
// -mavx2 selects the branch of saturateAVX2 (DspNumericPolicy.h) that the reference's own build (AVX2 on every target) takes:
// max_sd / min_sd, which turn a NaN error into -2 scale.  Without it the header falls back to two comparisons that keep the NaN.
// No FMA is enabled and nothing is contracted.
//   dither_probe <shaper 1|2> <bits> <rate> <in> <out> <n1> <n2>
// in: L then R, n1 + n2 doubles each; a fresh shaper, prepare(rate, bits), processStereoBlock of n1 then of n2 samples with
// kOutputHeadroom; out: the same layout.
#include <JuceHeader.h>
#include "DspNumericPolicy.h"
#include "FixedNoiseShaper.h"
#include "Fixed15TapNoiseShaper.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

template <typename Shaper>
static void run(double rate, int bits, double* l, double* r, int n1, int n2)
{
    auto sh = std::make_unique<Shaper>();
    sh->prepare(rate, bits);
    const double headroom = 0.8912509381337456;
    sh->processStereoBlock(l, r, n1, headroom);
    sh->processStereoBlock(l + n1, r + n1, n2, headroom);
}

int main(int argc, char** argv)
{
    if (argc != 8) return 2;
    const int shaper = std::atoi(argv[1]), bits = std::atoi(argv[2]), n1 = std::atoi(argv[6]), n2 = std::atoi(argv[7]);
    const double rate = std::atof(argv[3]);
    const size_t n = (size_t)n1 + (size_t)n2;
    std::vector<double> buf(2 * n);
    FILE* f = std::fopen(argv[4], "rb");
    if (!f || std::fread(buf.data(), sizeof(double), buf.size(), f) != buf.size()) return 3;
    std::fclose(f);
    if (shaper == 1) run<convo::FixedNoiseShaper>(rate, bits, buf.data(), buf.data() + n, n1, n2);
    else if (shaper == 2) run<convo::Fixed15TapNoiseShaper>(rate, bits, buf.data(), buf.data() + n, n1, n2);
    else return 2;
    f = std::fopen(argv[5], "wb");
    if (!f || std::fwrite(buf.data(), sizeof(double), buf.size(), f) != buf.size()) return 3;
    std::fclose(f);
    return 0;
}
