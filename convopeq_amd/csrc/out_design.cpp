// out_design.cpp -- host side of DSPCore's output stage (DSPCore::processOutputDouble with dither off,
// src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:577-744): the design of the 3 Hz UltraHighRateDCBlocker
// (src/UltraHighRateDCBlocker.h) and of the SimplePeakLimiter's release (src/audioengine/SimplePeakLimiter.h), the tables of
// the time-parallel DC kernel, and the five steps themselves, sequentially, in the reference's operation order.  No GPU.
// killDenormal is the identity, as in the reference's release build (src/DspNumericPolicy.h:189-204) and in ir_ingest.cpp.
#include "host_design.hpp"

#include <cmath>

namespace cpq {

// UltraHighRateDCBlocker::init(fs, 3.0) and SimplePeakLimiter::prepare(fs, 100.0), fallbacks included
void outDesign(double fs, double alpha[2], double* releaseCoeff)
{
    const double pi = 3.14159265358979323846;     // juce::MathConstants<double>::pi
    const double cutoffHz = 3.0;
    alpha[0] = alpha[1] = 1.0e-6;
    if (std::isfinite(fs) && fs > 0.0) {
        const double ratios[2] = { 1.0 - 0.1, 1.0 + 0.1 };
        for (int i = 0; i < 2; ++i) {
            const double fc = cutoffHz * ratios[i];
            const double omega = 2.0 * pi * fc / fs;
            double a = -std::expm1(-omega);
            if (!std::isfinite(a) || a <= 0.0 || a >= 1.0) a = 1.0e-6;
            alpha[i] = a;
        }
    }
    const double releaseSec = 100.0 * 0.001;
    *releaseCoeff = (releaseSec > 0.0 && fs > 0.0) ? std::exp(-1.0 / (fs * releaseSec)) : 0.0;
}

// a = 1 - alpha and its powers in long double, rounded once
void outSectionTable(double alpha, double* out)
{
    const long double a = 1.0L - (long double)alpha;
    out[0] = alpha;
    long double ac = 1.0L;
    for (int i = 0; i < kOutChunk; ++i) ac *= a;                        // a^chunk
    long double p = ac;
    for (int k = 0; k < kOutScanSteps; ++k) { out[1 + k] = (double)p; p *= p; }
    long double q = 1.0L;
    for (int l = 0; l < 64; ++l) { out[1 + kOutScanSteps + l] = (double)q; q *= ac; }
}

void OutStageHost::prepare(double fs)
{
    outDesign(fs, alpha, &releaseCoeff);
    reset();
}

void OutStageHost::reset()
{
    for (auto& ch : dc) ch[0] = ch[1] = 0.0;
    envelope = 1.0;
}

namespace {

bool finiteBelow(double v, double limit) { return std::isfinite(v) && std::fabs(v) < limit; }
double jmax(double a, double b) { return a < b ? b : a; }

}  // namespace

double outDesiredGain(double l, double r)
{
    const double clipStart = kOutLimiterThreshold - kOutLimiterKnee * 0.5;
    const double peak = jmax(std::fabs(l), std::fabs(r));
    const double safePeak = jmax(peak, 1.0e-12);
    double d = 1.0;
    if (safePeak > clipStart) {
        if (safePeak <= kOutLimiterThreshold) {
            const double t = (safePeak - clipStart) / kOutLimiterKnee;
            const double kneeShape = t * t * (3.0 - 2.0 * t);
            d = 1.0 - (1.0 - kOutLimiterThreshold / safePeak) * kneeShape;
        } else {
            d = kOutLimiterThreshold / safePeak;
        }
    }
    return d;
}

// the vector body of the reference's clamp: max_pd / min_pd return their second operand for a NaN
double outClamp(double v)
{
    const double t = v > -kOutHeadroom ? v : -kOutHeadroom;
    return t < kOutHeadroom ? t : kOutHeadroom;
}

void OutStageHost::process(double* l, double* r, int n, int flags)
{
    if (n <= 0) return;
    double* rows[2] = { l, r };
    if (flags & CPQ_OUT_DC_BLOCK)
        for (int ch = 0; ch < 2; ++ch) {
            double s0 = dc[ch][0], s1 = dc[ch][1];
            for (int i = 0; i < n; ++i) {
                double x = rows[ch][i];
                s0 = s0 + alpha[0] * (x - s0);
                x = x - s0;
                s1 = s1 + alpha[1] * (x - s1);
                x = x - s1;
                rows[ch][i] = x;
            }
            dc[ch][0] = finiteBelow(s0, 1.0e15) ? s0 : 0.0;
            dc[ch][1] = finiteBelow(s1, 1.0e15) ? s1 : 0.0;
        }
    if (flags & CPQ_OUT_HEADROOM)
        for (int ch = 0; ch < 2; ++ch)
            for (int i = 0; i < n; ++i) {
                const double v = rows[ch][i] * kOutHeadroom;
                rows[ch][i] = std::fabs(v) < 1.0e300 ? v : 0.0;
            }
    if (flags & CPQ_OUT_LIMITER)
        for (int i = 0; i < n; ++i) {
            const double d = outDesiredGain(l[i], r[i]);
            if (d < envelope) envelope = d;
            else envelope = 1.0 + (envelope - 1.0) * releaseCoeff;
            l[i] *= envelope;
            r[i] *= envelope;
        }
    if (flags & CPQ_OUT_CLAMP)
        for (int ch = 0; ch < 2; ++ch)
            for (int i = 0; i < n; ++i) rows[ch][i] = outClamp(rows[ch][i]);
}

}  // namespace cpq

extern "C" {

int32_t cpq_out_design(double rate, double alpha[2], double* releaseCoeff)
{
    if (!alpha || !releaseCoeff) return CPQ_ERR_INVALID_ARG;
    cpq::outDesign(rate, alpha, releaseCoeff);
    return CPQ_OK;
}

}  // extern "C"
