// Records what the reference's sample-rate converter (r8b::CDSPResampler, as ConvolverProcessorInternal::resampleIR configures it:
// transition band 2.0 %, stop band 140.0 dB, fprLinearPhase, oneshot) makes of one row, for tests/golden/resample_ref.npz
// (make_resample_ref.py drives it).  Build, with REF the reference's source tree:
//   g++ -std=c++17 -O2 -I$REF/r8brain-free-src tests/golden/resample_probe.cpp -o resample_probe -lpthread
//   resample_probe <in rate> <out rate> <in> <out>
// in: the row as doubles (the file's size gives n).  out (doubles): getMaxOutLen(n), then that many outputs of oneshot().
#include "CDSPResampler.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: resample_probe <in rate> <out rate> <in> <out>\n"); return 2; }
    const double inRate = std::atof(argv[1]), outRate = std::atof(argv[2]);
    std::vector<double> x;
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) return 1;
    std::fseek(f, 0, SEEK_END);
    x.resize((size_t)std::ftell(f) / sizeof(double));
    std::fseek(f, 0, SEEK_SET);
    const bool read = std::fread(x.data(), sizeof(double), x.size(), f) == x.size();
    std::fclose(f);
    if (!read || x.empty()) return 1;

    const int n = (int)x.size();
    r8b::CDSPResampler resampler(inRate, outRate, n, 2.0, 140.0, r8b::fprLinearPhase);
    const int maxOut = resampler.getMaxOutLen(n);
    if (maxOut <= 0) return 1;
    std::vector<double> y((size_t)maxOut + 1, 0.0);
    y[0] = (double)maxOut;
    resampler.oneshot(x.data(), n, y.data() + 1, maxOut);

    f = std::fopen(argv[4], "wb");
    if (!f) return 1;
    const bool wrote = std::fwrite(y.data(), sizeof(double), y.size(), f) == y.size();
    std::fclose(f);
    std::printf("n %d maxOut %d\n", n, maxOut);
    return wrote ? 0 : 1;
}
