// Records what the reference's own LatticeNoiseShaper computes, for tests/golden/lattice_ref.npz (make_lattice_ref.py drives
// it).  Build, with REF the reference's source tree:
//   g++ -std=c++20 -O2 -ffp-contract=off -msse4.1 -mavx2 -mfma -Itests/golden/juce_shim -I$REF/src tests/golden/lattice_probe.cpp -o lattice_probe
// -mfma: computeFeedback is written with _mm256_fmadd_pd.  Nothing else is contracted.  The header calls
// replaceNonFiniteWithZero unqualified, so DspNumericPolicy.h and a using-directive come first.
//   lattice_probe <bits> <in> <out> <n1> <n2> <nA> <A ...> [<nB> <B ...>]
// in: L then R, n1 + n2 doubles each; a fresh shaper, prepare(bits), setCoefficients(A, nA) (DSPCore::prepare's order),
// processStereoBlock of n1 samples with kOutputHeadroom, applyMatchedCoefficients(B, nB) when a second set is given, then
// processStereoBlock of n2 samples; out: the same layout.
#include <JuceHeader.h>
#include "DspNumericPolicy.h"
using namespace convo::numeric_policy;
#include "LatticeNoiseShaper.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

static bool readSet(int argc, char** argv, int& at, std::vector<double>& set)
{
    if (at >= argc) return false;
    const int n = std::atoi(argv[at++]);
    if (n < 0 || at + n > argc) return false;
    set.clear();
    for (int i = 0; i < n; ++i) set.push_back(std::strtod(argv[at++], nullptr));     // "nan" and "inf" parse
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    const int bits = std::atoi(argv[1]), n1 = std::atoi(argv[4]), n2 = std::atoi(argv[5]);
    int at = 6;
    std::vector<double> a, b;
    if (!readSet(argc, argv, at, a)) return 2;
    const bool swap = at < argc;
    if (swap && (!readSet(argc, argv, at, b) || at != argc)) return 2;
    const size_t n = (size_t)n1 + (size_t)n2;
    std::vector<double> buf(2 * n);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f || std::fread(buf.data(), sizeof(double), buf.size(), f) != buf.size()) return 3;
    std::fclose(f);
    double* l = buf.data();
    double* r = buf.data() + n;
    auto sh = std::make_unique<LatticeNoiseShaper>();
    const double headroom = 0.8912509381337456;
    sh->prepare(bits);
    sh->setCoefficients(a.data(), (int)a.size());
    sh->processStereoBlock(l, r, n1, headroom);
    if (swap) sh->applyMatchedCoefficients(b.data(), (int)b.size());
    sh->processStereoBlock(l + n1, r + n1, n2, headroom);
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(buf.data(), sizeof(double), buf.size(), f) != buf.size()) return 3;
    std::fclose(f);
    return 0;
}
