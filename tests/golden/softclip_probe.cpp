// Records what the reference's own soft clipper computes, for tests/golden/softclip_ref.npz (make_softclip_ref.py drives it).
// The two functions, musicalSoftClipScalar and softClipBlockAVX2, live in an anonymous namespace of
// src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp, a translation unit that drags in the whole engine.  The make script
// cuts that stretch of the file, at generation time only, into a scratch directory as softclip_cut.inc, and this driver includes
// it there.  Nothing cut or compiled is kept.  Build, with REF the reference's source tree and CUT the scratch directory:
//   g++ -std=c++20 -O2 -ffp-contract=off -msse4.1 -mavx2 -mfma -Itests/golden/juce_shim -I$REF/src -I$CUT tests/golden/softclip_probe.cpp -o softclip_probe
// -mfma: the 4-wide loop is written with _mm256_fmadd_pd / _mm256_fnmadd_pd.  Nothing else is contracted.
//   softclip_probe <amount> <block length> <in> <out> <n>
// in: n doubles.  The parameters are formed as DSPCore::processDouble forms them from the float amount (:474-477), then
// softClipBlockAVX2 runs in place over the n samples block by block (the last block shorter).  out: threshold, knee, asymmetry,
// then the n samples.
#include <JuceHeader.h>
#include <immintrin.h>
#include "dsp/math/FastTanhApprox.h"

#include <bit>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

// what the stretch uses from headers this driver cannot include (AudioEngine.h, JUCE): |x| by clearing the sign bit, and jlimit
inline double absNoLibm(double x) noexcept { return std::bit_cast<double>(std::bit_cast<std::uint64_t>(x) & 0x7FFFFFFFFFFFFFFFULL); }
namespace juce {
template <typename T> T jlimit(T lo, T hi, T v) { return v < lo ? lo : (hi < v ? hi : v); }
}  // namespace juce

namespace {
#include "softclip_cut.inc"
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const float amount = (float)std::atof(argv[1]);
    const int block = std::atoi(argv[2]), n = std::atoi(argv[5]);
    if (block <= 0 || n <= 0) return 2;
    std::vector<double> buf((size_t)n);
    FILE* f = std::fopen(argv[3], "rb");
    if (!f || std::fread(buf.data(), sizeof(double), buf.size(), f) != buf.size()) return 3;
    std::fclose(f);
    const double sat = static_cast<double>(amount);
    const double par[3] = { 0.95 - 0.45 * sat, 0.05 + 0.35 * sat, 0.10 * sat };
    double prev = 0.0;
    for (int o = 0; o < n; o += block) softClipBlockAVX2(buf.data() + o, n - o < block ? n - o : block, par[0], par[1], par[2], prev);
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(par, sizeof(double), 3, f) != 3 || std::fwrite(buf.data(), sizeof(double), buf.size(), f) != buf.size()) return 3;
    std::fclose(f);
    return 0;
}
