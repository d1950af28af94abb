// os_design.cpp -- host-side design of the half-band oversampler (CustomInputOversampler, src/CustomInputOversampler.cpp)
// and the oversampling factor policy (OversamplingPolicy, src/audioengine/OversamplingPolicy.h).  Plain host code, no GPU.
#include "host_design.hpp"

#include <algorithm>
#include <cmath>

namespace cpq {

namespace {

// CustomInputOversampler::tapsForStage / attenuationForStage (:87-106)
constexpr int kOsTaps[2][3] = { { 511, 127, 31 }, { 1023, 255, 63 } };
constexpr double kOsAtten[2][3] = { { 140.0, 110.0, 90.0 }, { 160.0, 140.0, 120.0 } };

// CustomInputOversampler::besselI0 (:144-157), series in the reference's operation order
double besselI0(double x)
{
    double sum = 1.0;
    double term = 1.0;
    const double xx = x * x;
    for (int n = 1; n < 100; ++n) {
        term *= xx / (4.0 * (double)n * (double)n);
        sum += term;
        if (term < sum * 1.0e-18) break;
    }
    return sum;
}

}  // namespace

bool osDesignStage(int stage, int type, OsStage& out)
{
    if (stage < 0 || stage > 2 || (type != CPQ_OS_IIR && type != CPQ_OS_LINEAR_PHASE)) return false;
    osDesignHalfband(kOsTaps[type][stage], kOsAtten[type][stage], out);
    return true;
}

// prepareStage (:287-390) in the reference's operation order; TruePeakDetector::prepareStage (src/TruePeakDetector.cpp) is
// the same text with its own tap counts and attenuation
void osDesignHalfband(int taps, double atten, OsStage& out)
{
    const double pi = 3.141592653589793238;       // juce::MathConstants<double>::pi
    OsStage s{};
    s.taps = std::max(3, taps | 1);
    s.centerTap = (s.taps - 1) / 2;
    s.centerParity = s.centerTap & 1;
    s.convParity = 1 - s.centerParity;
    s.attenuationDb = atten;
    std::vector<double>& raw = s.raw;
    raw.assign((size_t)s.taps, 0.0);
    const double beta = (atten > 50.0) ? (0.1102 * (atten - 8.7))
                      : ((atten >= 21.0) ? (0.5842 * std::pow(atten - 21.0, 0.4) + 0.07886 * (atten - 21.0)) : 0.0);
    const double i0Beta = besselI0(beta);
    const int M = s.centerTap;
    for (int n = 0; n < s.taps; ++n) {
        const double t = (double)(n - M);
        const double sinc = (n == M) ? 0.5 : (std::sin(pi * 0.5 * t) / (pi * t));
        const double frac = (double)(n - M) / (double)M;
        const double window = besselI0(beta * std::sqrt(std::max(0.0, 1.0 - frac * frac))) / i0Beta;
        raw[n] = sinc * window;
    }
    for (int n = 0; n < s.taps; ++n)
        if (n != s.centerTap && ((n & 1) == s.centerParity)) raw[n] = 0.0;
    double sum = 0.0;
    for (int i = 0; i < s.taps; ++i) sum += raw[i];
    if (std::abs(sum) > 1.0e-20) {
        const double inv = 1.0 / sum;
        for (int i = 0; i < s.taps; ++i) raw[i] *= inv;
    }
    raw[s.centerTap] = 0.5;
    double nonCenterSum = 0.0;
    for (int i = 0; i < s.taps; ++i)
        if (i != s.centerTap) nonCenterSum += raw[i];
    if (std::abs(nonCenterSum) > 1.0e-20) {
        const double scale = 0.5 / nonCenterSum;
        for (int i = 0; i < s.taps; ++i)
            if (i != s.centerTap) raw[i] *= scale;
    }
    raw[s.centerTap] = 0.5;
    s.convCount = (s.taps - s.convParity + 1) / 2;
    s.conv.assign((size_t)s.convCount, 0.0);
    for (int r = 0; r < s.convCount; ++r) {
        const int k = s.convParity + (r << 1);
        s.conv[r] = (k < s.taps) ? raw[k] : 0.0;
    }
    s.centerCoeff = raw[s.centerTap];
    s.centerDelayInput = (s.centerTap - s.centerParity) / 2;
    s.historyUpKeep = std::max(s.convCount - 1, s.centerDelayInput);
    s.historyDownKeep = std::max(s.centerTap, s.convParity + ((s.convCount - 1) << 1) + 6);
    out = std::move(s);
}

int osStagesFor(int factor) { return factor == 8 ? 3 : factor == 4 ? 2 : factor == 2 ? 1 : factor == 1 ? 0 : -1; }

}  // namespace cpq

extern "C" {

int32_t cpq_os_resolve_factor(double baseRate, int32_t requested)
{
    if (!(baseRate > 0.0) || !std::isfinite(baseRate)) return CPQ_ERR_INVALID_ARG;
    // OversamplingPolicy::maxAllowedFactor / resolve
    const int maxF = baseRate <= 96000.0 ? 8 : baseRate <= 192000.0 ? 4 : baseRate <= 384000.0 ? 2 : baseRate <= 768000.0 ? 1 : 0;
    if (maxF == 0) return 0;        // DSPCore: targetFactor = supported ? resolved : 0
    int eff = requested;
    if (eff != 0 && eff != 1 && eff != 2 && eff != 4 && eff != 8) eff = 0;
    return eff > 0 ? std::min(eff, maxF) : maxF;
}

int32_t cpq_os_design_stage(int32_t stage, int32_t type, cpq_os_stage_info* info, double* taps, int32_t capacity)
{
    cpq::OsStage s;
    if (!cpq::osDesignStage(stage, type, s)) return CPQ_ERR_INVALID_ARG;
    if (taps && capacity < s.taps) return CPQ_ERR_INVALID_ARG;
    if (info) {
        info->taps = s.taps;
        info->center_tap = s.centerTap;
        info->center_parity = s.centerParity;
        info->conv_parity = s.convParity;
        info->conv_count = s.convCount;
        info->center_delay_input = s.centerDelayInput;
        info->history_up_keep = s.historyUpKeep;
        info->history_down_keep = s.historyDownKeep;
        info->attenuation_db = s.attenuationDb;
        info->center_coeff = s.centerCoeff;
    }
    if (taps) std::copy(s.raw.begin(), s.raw.end(), taps);
    return s.taps;
}

double cpq_os_latency(int32_t factor, int32_t type)
{
    const int n = cpq::osStagesFor(factor);
    if (n < 0 || (type != CPQ_OS_IIR && type != CPQ_OS_LINEAR_PHASE)) return (double)CPQ_ERR_INVALID_ARG;
    // up and down each delay stage i by center_tap samples at its high rate, 2^(i+1) x the base rate
    double lat = 0.0;
    for (int i = 0; i < n; ++i) {
        cpq::OsStage s;
        cpq::osDesignStage(i, type, s);
        lat += 2.0 * s.centerTap / (double)(2 << i);
    }
    return lat;
}

}  // extern "C"
