// resample_design.cpp -- host side of the IR sample-rate conversion (ConvolverProcessorInternal::resampleIR,
// src/convolver/ConvolverProcessor.ResampleAndFallback.cpp:18-108).  Plain host code, no GPU.
//
// The reference hands the work to r8brain's CDSPResampler (2 % transition band, 140 dB, linear phase), a cascade of half-band
// stages and a fractional interpolator.  Here the same class of filter is one Kaiser-windowed sinc, sampled L times per input
// sample and stored as L phases of T taps:
//     g(t) = c sinc(c t) I0(beta sqrt(1 - (2 t / T)^2)) / I0(beta),    |t| <= T / 2  (t in input samples)
//     taps[p][k] = g(k - T / 2 + p / L) / (sum over k of the same)
// c = 0.98 min(in, out) / in puts the -6 dB point at 0.98 of the lower Nyquist frequency, and T is Kaiser's length for a
// transition of 0.02 of that frequency to either side: flat to 0.96, stopped from 1.0.  beta is Kaiser's for 180 dB, not for the
// nominal 140: r8brain itself leaves 2e-10 of a stop-band signal and 1.5e-10 of error on a pass-band one, and a Kaiser design's
// pass-band ripple is as large as its stop-band ripple.  Everything up to the final rounding is long double.  g is even and the
// argument is formed from the integer (k - T / 2) L + p, so phase L - p is phase p reversed, bit for bit; the table stores it so.
#include "resample_design.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <thread>

namespace cpq {

namespace {

constexpr long double kPiL = 3.14159265358979323846264338327950288L;
constexpr double kMinRate = 8000.0, kMaxRate = 768000.0;

long double besselI0(long double x)
{
    long double sum = 1.0L, term = 1.0L;
    const long double q = x * x / 4.0L;
    for (int n = 1; n < 1000; ++n) {
        term *= q / ((long double)n * (long double)n);
        sum += term;
        if (term < sum * 1.0e-22L) break;
    }
    return sum;
}

}  // namespace

int resampleDesign(double inRate, double outRate, ResampleDesign& d, const char** why)
{
    const char* unused;
    if (!why) why = &unused;
    for (double r : { inRate, outRate }) {
        if (!std::isfinite(r) || r != std::floor(r)) { *why = "sample rates must be whole numbers of Hz"; return CPQ_ERR_UNSUPPORTED; }
        if (r < kMinRate || r > kMaxRate) { *why = "sample rate outside 8000 ... 768000 Hz"; return CPQ_ERR_UNSUPPORTED; }
    }
    const int64_t in = (int64_t)inRate, out = (int64_t)outRate, g = std::gcd(in, out);
    if (out / g > CPQ_RESAMPLE_MAX_FACTOR || in / g > CPQ_RESAMPLE_MAX_FACTOR) {
        *why = "the rate pair does not reduce to factors of 1280 or less";
        return CPQ_ERR_UNSUPPORTED;
    }
    d.L = (int)(out / g);
    d.M = (int)(in / g);
    const long double lower = (long double)std::min(in, out) / (long double)in;        // lower Nyquist / input Nyquist
    const long double c = (long double)kResampleEdge * lower;
    const long double beta = 0.1102L * ((long double)kResampleAttenDb - 8.7L);
    const long double width = 2.0L * (long double)kResampleHalfBand * lower * kPiL;      // transition, rad per input sample
    const int half = (int)std::ceil((double)(((long double)kResampleAttenDb - 7.95L) / (2.285L * width) / 2.0L));
    d.T = 2 * half;
    d.groupDelay = (double)half;
    d.cutoff = (double)c;
    d.taps.assign((size_t)d.L * d.T, 0.0);

    const int L = d.L, T = d.T;
    const long double i0Beta = besselI0(beta);
    std::vector<long double> row((size_t)T);
    for (int p = 0; 2 * p <= L; ++p) {
        long double sum = 0.0L;
        for (int k = 0; k < T; ++k) {
            const int64_t m = (int64_t)(k - half) * L + p;             // t = m / L
            const long double t = (long double)m / (long double)L;
            const long double u = t / (long double)half;
            long double v = 0.0L;
            if (u > -1.0L && u < 1.0L) {
                const long double arg = kPiL * c * t;
                const long double sinc = (m == 0) ? 1.0L : sinl(arg) / arg;
                v = c * sinc * besselI0(beta * sqrtl(1.0L - u * u)) / i0Beta;
            }
            row[k] = v;
            sum += v;
        }
        double* dst = d.taps.data() + (size_t)p * T;
        for (int k = 0; k < T; ++k) dst[k] = (double)(row[k] / sum);
    }
    // g(-t) = g(t): taps[L - p][T - 1 - k] = taps[p][k]
    for (int p = L / 2 + 1; p < L; ++p) {
        const double* src = d.taps.data() + (size_t)(L - p) * T;
        double* dst = d.taps.data() + (size_t)p * T;
        for (int k = 0; k < T; ++k) dst[k] = src[T - 1 - k];
    }
    return CPQ_OK;
}

int resampleCheck(const cpq_ir_buffer* in, double targetRate, int phase, bool& copy, ResampleDesign& d, const char** why, bool designKnown)
{
    const char* unused;
    if (!why) why = &unused;
    copy = false;
    if (!in || !in->data) { *why = "null buffer"; return CPQ_ERR_INVALID_ARG; }
    if (in->n_channels <= 0 || in->n_samples <= 0) { *why = "an IR needs at least one channel and one sample"; return CPQ_ERR_INVALID_ARG; }
    if (phase != CPQ_RESAMPLE_LINEAR_PHASE && phase != CPQ_RESAMPLE_MINIMUM_PHASE) { *why = "unknown phase response"; return CPQ_ERR_INVALID_ARG; }
    if (!(in->sample_rate > 0.0) || !std::isfinite(in->sample_rate) || !(targetRate > 0.0) || !std::isfinite(targetRate)) {
        *why = "sample rates must be finite and > 0";
        return CPQ_ERR_INVALID_ARG;
    }
    if (phase == CPQ_RESAMPLE_MINIMUM_PHASE) { *why = "the minimum-phase resampler is not built"; return CPQ_ERR_UNSUPPORTED; }
    if (std::fabs(in->sample_rate - targetRate) <= 1e-6) { copy = true; return CPQ_OK; }
    double peak = 0.0;
    const size_t total = (size_t)in->n_channels * (size_t)in->n_samples;
    for (size_t i = 0; i < total; ++i) peak = std::max(peak, std::fabs(in->data[i]));
    if (peak < 1e-12) { *why = "silent IR: peak below 1e-12"; return CPQ_ERR_SILENT_IR; }
    if (!designKnown) {
        const int rc = resampleDesign(in->sample_rate, targetRate, d, why);
        if (rc != CPQ_OK) return rc;
    }
    if (resampleOutLen(in->n_samples, d.L, d.M) > 0x7fffffff) { *why = "the converted IR would exceed 2^31 - 1 samples"; return CPQ_ERR_UNSUPPORTED; }
    return CPQ_OK;
}

void resampleRowHost(const ResampleDesign& d, const double* x, int n, double* y, int64_t j0, int64_t j1)
{
    const int T = d.T, half = d.T / 2;
    for (int64_t j = j0; j < j1; ++j) {
        const int64_t at = j * d.M, centre = at / d.L + half;
        const double* h = d.taps.data() + (size_t)(at % d.L) * T;
        // the terms outside the row multiply a zero and leave the sum as it is: they are passed over
        const int k0 = (int)std::max<int64_t>(0, centre - (n - 1)), k1 = (int)std::min<int64_t>(T - 1, centre);
        double acc = 0.0;
        for (int k = k0; k <= k1; ++k) acc = std::fma(h[k], x[centre - k], acc);
        y[j] = acc;
    }
}

int resampleFinish(const double* rows, int channels, int nOut, double rate, cpq_ir_buffer* out)
{
    std::vector<int> length((size_t)channels);
    int maxLen = 0;
    for (int ch = 0; ch < channels; ++ch) {
        const double* buf = rows + (size_t)ch * (size_t)nOut;
        double peak = 0.0;
        for (int i = 0; i < nOut; ++i) peak = std::max(peak, std::fabs(buf[i]));
        int effective = 1;
        if (!(peak < 1e-12)) {
            const double threshold = peak * std::pow(10.0, -160.0 / 20.0);
            int consecutive = 0;
            for (int i = nOut - 1; i >= 0; --i) {
                if (std::fabs(buf[i]) > threshold) {
                    if (++consecutive >= 8) { effective = i + 8; break; }
                } else {
                    consecutive = 0;
                }
            }
        }
        length[ch] = effective;
        maxLen = std::max(maxLen, effective);
    }
    out->data = static_cast<double*>(std::calloc((size_t)channels * (size_t)maxLen, sizeof(double)));
    if (!out->data) return CPQ_ERR_OOM;
    out->n_channels = channels;
    out->n_samples = maxLen;
    out->sample_rate = rate;
    for (int ch = 0; ch < channels; ++ch)
        std::memcpy(out->data + (size_t)ch * (size_t)maxLen, rows + (size_t)ch * (size_t)nOut, sizeof(double) * (size_t)length[ch]);
    return CPQ_OK;
}

int resampleCopy(const cpq_ir_buffer* in, cpq_ir_buffer* out)
{
    const size_t total = (size_t)in->n_channels * (size_t)in->n_samples;
    out->data = static_cast<double*>(std::malloc(total * sizeof(double)));
    if (!out->data) return CPQ_ERR_OOM;
    std::memcpy(out->data, in->data, total * sizeof(double));
    out->n_channels = in->n_channels;
    out->n_samples = in->n_samples;
    out->sample_rate = in->sample_rate;
    return CPQ_OK;
}

}  // namespace cpq

extern "C" {

int32_t cpq_resample_design(double in_rate, double out_rate, cpq_resample_info* info, double* table, int32_t capacity)
{
    cpq::ResampleDesign d;
    const int rc = cpq::resampleDesign(in_rate, out_rate, d, nullptr);
    if (rc != CPQ_OK) return rc;
    const int32_t count = (int32_t)d.taps.size();
    if (table && capacity < count) return CPQ_ERR_INVALID_ARG;
    if (info) {
        info->l = d.L;
        info->m = d.M;
        info->taps = d.T;
        info->reserved = 0;
        info->group_delay = d.groupDelay;
        info->cutoff = d.cutoff;
        info->attenuation_db = cpq::kResampleAttenDb;
    }
    if (table) std::copy(d.taps.begin(), d.taps.end(), table);
    return count;
}

int32_t cpq_ir_resample_host(const cpq_ir_buffer* in, double target_rate, int32_t phase, cpq_ir_buffer* out)
{
    if (!out) return CPQ_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    try {
        cpq::ResampleDesign d;
        bool copy = false;
        const int rc = cpq::resampleCheck(in, target_rate, phase, copy, d, nullptr, false);
        if (rc != CPQ_OK) return rc;
        if (copy) return cpq::resampleCopy(in, out);
        const int channels = in->n_channels, n = in->n_samples;
        const int64_t nOut = cpq::resampleOutLen(n, d.L, d.M);
        std::vector<double> rows((size_t)channels * (size_t)nOut);
        const int64_t total = (int64_t)channels * nOut, fmas = total * d.T;
        const int nThreads = (int)std::max<int64_t>(1, std::min<int64_t>({ 16, (int64_t)std::thread::hardware_concurrency(), fmas >> 22 }));
        auto work = [&](int t) {
            // thread t takes the t-th share of every channel: a row's outputs do not depend on who computes them
            for (int ch = 0; ch < channels; ++ch)
                cpq::resampleRowHost(d, in->data + (size_t)ch * (size_t)n, n, rows.data() + (size_t)ch * (size_t)nOut, nOut * t / nThreads,
                                     nOut * (t + 1) / nThreads);
        };
        std::vector<std::thread> pool;
        int started = 1;
        try {
            pool.reserve((size_t)nThreads);
            for (; started < nThreads; ++started) pool.emplace_back(work, started);
        } catch (const std::exception&) {}                  // no more threads to be had: this one does the remaining shares
        work(0);
        for (int t = started; t < nThreads; ++t) work(t);
        for (auto& th : pool) th.join();
        return cpq::resampleFinish(rows.data(), channels, (int)nOut, target_rate, out);
    } catch (const std::exception&) {
        cpq_ir_buffer_free(out);
        std::memset(out, 0, sizeof(*out));
        return CPQ_ERR_OOM;
    }
}

}  // extern "C"
