// Stand-alone check of resample_design.cpp under AddressSanitizer and UBSan: the filter design at the extreme rate pairs, the
// host path at rows shorter than, as long as and longer than the filter, the refusals, the tail trim and the copy.
//   g++ -O1 -g -std=c++20 -fsanitize=address,undefined -Iconvopeq_amd/csrc -Iinclude tests/sanitize/resample_design_check.cpp
//       convopeq_amd/csrc/resample_design.cpp convopeq_amd/csrc/ir_ingest.cpp -o resample_design_check -lpthread
// Every output of the host path is compared with a long double sum over the whole filter with explicit zero extension.
#include "resample_design.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int g_failed = 0;

void check(bool ok, const char* what, double a = 0.0, double b = 0.0)
{
    if (ok) return;
    ++g_failed;
    std::printf("FAILED %s (%g, %g)\n", what, a, b);
}

double noise(unsigned& s)
{
    s = s * 1664525u + 1013904223u;
    return (double)(int)(s >> 8) / 8388608.0 - 1.0;
}

// one row through cpq_ir_resample_host against the definition; decay makes the tail trim cut something
void checkRow(double inRate, double outRate, int n, double decay)
{
    cpq::ResampleDesign d;
    check(cpq::resampleDesign(inRate, outRate, d, nullptr) == CPQ_OK, "design");
    unsigned seed = 12345u + (unsigned)n;
    std::vector<double> x((size_t)n);
    for (int i = 0; i < n; ++i) x[(size_t)i] = noise(seed) * std::exp(-decay * i);
    x[0] = 0.75;
    cpq_ir_buffer in{ 1, n, inRate, x.data() }, out;
    check(cpq_ir_resample_host(&in, outRate, CPQ_RESAMPLE_LINEAR_PHASE, &out) == CPQ_OK, "host path");
    const int64_t nOut = cpq::resampleOutLen(n, d.L, d.M);
    check(out.n_channels == 1 && out.n_samples >= 1 && out.n_samples <= nOut && out.sample_rate == outRate, "output shape", out.n_samples, (double)nOut);
    for (int64_t j = 0; j < out.n_samples; ++j) {
        const int64_t centre = j * d.M / d.L + d.T / 2;
        const double* h = d.taps.data() + (size_t)(j * d.M % d.L) * (size_t)d.T;
        long double sum = 0.0L, mag = 0.0L;
        for (int k = 0; k < d.T; ++k) {
            const int64_t idx = centre - k;
            const long double v = (idx >= 0 && idx < n) ? (long double)x[(size_t)idx] : 0.0L;
            sum += (long double)h[k] * v;
            mag += fabsl((long double)h[k] * v);
        }
        const long double limit = (long double)d.T * 1.2e-16L * mag;
        if (fabsl((long double)out.data[j] - sum) > limit) { check(false, "output against the definition", out.data[j], (double)sum); break; }
    }
    // a share of the row computed alone is the same bits
    std::vector<double> part((size_t)nOut, -1.0);
    const int64_t a = nOut / 3, b = nOut - nOut / 4;
    cpq::resampleRowHost(d, x.data(), n, part.data(), a, b);
    for (int64_t j = a; j < b && j < out.n_samples; ++j)
        if (std::memcmp(&part[(size_t)j], &out.data[j], sizeof(double)) != 0) { check(false, "share of a row", part[(size_t)j], out.data[j]); break; }
    check(part[0] == -1.0 || a == 0, "share stays inside its range");
    std::printf("%g -> %g, n %d: L %d M %d T %d, kept %d of %lld\n", inRate, outRate, n, d.L, d.M, d.T, out.n_samples, (long long)nOut);
    cpq_ir_buffer_free(&out);
}

}  // namespace

int main()
{
    // design: extreme pairs, refusals
    cpq::ResampleDesign d;
    const char* why = nullptr;
    check(cpq::resampleDesign(8000, 768000, d, &why) == CPQ_OK && d.L == 96 && d.M == 1, "8000 -> 768000");
    check(cpq::resampleDesign(768000, 8000, d, &why) == CPQ_OK && d.L == 1 && d.M == 96 && (int)d.taps.size() == d.T, "768000 -> 8000");
    check(cpq::resampleDesign(8008, 10240, d, &why) == CPQ_OK && d.L == 1280 && d.M == 1001, "1280 : 1001");
    check(cpq::resampleDesign(44100.5, 48000, d, &why) == CPQ_ERR_UNSUPPORTED && why, "non-integer rate");
    check(cpq::resampleDesign(48000, 44101, d, &why) == CPQ_ERR_UNSUPPORTED, "L above 1280");
    check(cpq::resampleDesign(7999, 48000, d, &why) == CPQ_ERR_UNSUPPORTED, "rate below 8000");
    check(cpq::resampleDesign(NAN, 48000, d, &why) == CPQ_ERR_UNSUPPORTED, "NaN rate");
    cpq_resample_info info;
    const int32_t count = cpq_resample_design(44100, 48000, &info, nullptr, 0);
    std::vector<double> table((size_t)count);
    check(count == info.l * info.taps && cpq_resample_design(44100, 48000, nullptr, table.data(), count) == count, "table copy");
    check(cpq_resample_design(44100, 48000, nullptr, table.data(), count - 1) == CPQ_ERR_INVALID_ARG, "capacity");

    // host path: rows around the filter length (T = 600 at 44100 -> 48000), both directions, the widest ratios
    for (int n : { 1, 2, 300, 599, 600, 601, 5000 }) checkRow(44100, 48000, n, 0.01);
    for (int n : { 1, 653, 2000 }) checkRow(48000, 44100, n, 0.02);
    checkRow(96000, 48000, 1500, 0.02);
    checkRow(48000, 96000, 700, 0.05);
    checkRow(768000, 8000, 300, 0.0);
    checkRow(8000, 768000, 40, 0.0);
    checkRow(44100, 48000, 400000, 1e-4);       // enough work for every thread

    // refusals, copy, stereo trim
    double buf[8] = { 0.5, 0.25, 0, 0, 0, 0, 0, 0 };
    cpq_ir_buffer in{ 2, 4, 44100.0, buf }, out;
    check(cpq_ir_resample_host(nullptr, 48000, 0, &out) == CPQ_ERR_INVALID_ARG && !out.data, "null input");
    check(cpq_ir_resample_host(&in, 48000, 0, nullptr) == CPQ_ERR_INVALID_ARG, "null output");
    check(cpq_ir_resample_host(&in, 48000, CPQ_RESAMPLE_MINIMUM_PHASE, &out) == CPQ_ERR_UNSUPPORTED && !out.data, "minimum phase");
    check(cpq_ir_resample_host(&in, 48000, 5, &out) == CPQ_ERR_INVALID_ARG, "unknown phase");
    cpq_ir_buffer none{ 0, 4, 44100.0, buf }, empty{ 2, 0, 44100.0, buf };
    check(cpq_ir_resample_host(&none, 48000, 0, &out) == CPQ_ERR_INVALID_ARG, "no channels");
    check(cpq_ir_resample_host(&empty, 48000, 0, &out) == CPQ_ERR_INVALID_ARG, "no samples");
    double quiet[4] = { 9e-13, 0, -9e-13, 0 };
    cpq_ir_buffer silent{ 1, 4, 44100.0, quiet };
    check(cpq_ir_resample_host(&silent, 48000, 0, &out) == CPQ_ERR_SILENT_IR && !out.data, "silent IR");
    check(cpq_ir_resample_host(&in, 44100.0 + 5e-7, 0, &out) == CPQ_OK && out.n_samples == 4 && std::memcmp(out.data, buf, sizeof(buf)) == 0, "copy");
    cpq_ir_buffer_free(&out);
    // 5 outputs cannot hold a run of 8: the reference's rule keeps one sample
    check(cpq_ir_resample_host(&in, 48000, 0, &out) == CPQ_OK && out.n_channels == 2 && out.n_samples == 1, "stereo", out.n_samples);
    if (out.data) check(out.data[0] != 0.0 && out.data[1] == 0.0, "silent channel is zeros");
    cpq_ir_buffer_free(&out);

    std::printf("%d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
