// meter_design.cpp -- host-side design of the meters (LoudnessMeter::updateCoefficients, src/LoudnessMeter.cpp;
// TruePeakDetector::prepare, src/TruePeakDetector.cpp) and the tables of the time-parallel K-weighting kernel.  No GPU.
#include "host_design.hpp"

#include <algorithm>
#include <cmath>

namespace cpq {

// updateCoefficients(fs) in the reference's operation order (RBJ cookbook high-pass and high shelf, normalised by 1 / a0)
void meterKWeighting(double fs, double pre[5], double rlb[5])
{
    const double pi = 3.14159265358979323846;     // M_PI
    {
        const double w0 = 2.0 * pi * 38.0 / fs;
        const double cosW0 = std::cos(w0);
        const double sinW0 = std::sin(w0);
        const double alpha = sinW0 / (2.0 * 0.50);
        const double b0 = (1.0 + cosW0) / 2.0;
        const double b1 = -(1.0 + cosW0);
        const double b2 = (1.0 + cosW0) / 2.0;
        const double a0 = 1.0 + alpha;
        const double a1 = -2.0 * cosW0;
        const double a2 = 1.0 - alpha;
        const double invA0 = 1.0 / a0;
        rlb[0] = b0 * invA0;
        rlb[1] = b1 * invA0;
        rlb[2] = b2 * invA0;
        rlb[3] = a1 * invA0;
        rlb[4] = a2 * invA0;
    }
    {
        const double w0 = 2.0 * pi * 1500.0 / fs;
        const double cosW0 = std::cos(w0);
        const double sinW0 = std::sin(w0);
        const double A = std::pow(10.0, 4.0 / 40.0);
        const double alpha = sinW0 / (2.0 * 0.7071067811865476);
        const double sqrtA = std::sqrt(A);
        const double b0 = A * ((A + 1.0) + (A - 1.0) * cosW0 + 2.0 * sqrtA * alpha);
        const double b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cosW0);
        const double b2 = A * ((A + 1.0) + (A - 1.0) * cosW0 - 2.0 * sqrtA * alpha);
        const double a0 = (A + 1.0) - (A - 1.0) * cosW0 + 2.0 * sqrtA * alpha;
        const double a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cosW0);
        const double a2 = (A + 1.0) - (A - 1.0) * cosW0 - 2.0 * sqrtA * alpha;
        const double invA0 = 1.0 / a0;
        pre[0] = b0 * invA0;
        pre[1] = b1 * invA0;
        pre[2] = b2 * invA0;
        pre[3] = a1 * invA0;
        pre[4] = a2 * invA0;
    }
}

// TruePeakDetector::prepare: stage 0 = kDefaultTaps (63), stage 1 = max(15, 63 / 2), both at kDefaultAttenuationDb (100 dB)
bool meterTpDesignStage(int stage, OsStage& out)
{
    if (stage != 0 && stage != 1) return false;
    osDesignHalfband(stage == 0 ? 63 : std::max(15, 63 / 2), 100.0, out);
    return true;
}

void meterSectionTables(const double coef[5], double* out)
{
    for (int i = 0; i < 5; ++i) out[i] = coef[i];
    const long double c = 1.0L + (long double)coef[3] + (long double)coef[4];      // exact to the last bit of a1, a2
    out[5] = (double)c;
    out[6] = out[7] = 0.0;
    struct M2 { long double a, b, c, d; };
    auto mul = [](const M2& x, const M2& y) { return M2{ x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d }; };
    auto put = [](double* p, const M2& m) { p[0] = (double)m.a; p[1] = (double)m.b; p[2] = (double)m.c; p[3] = (double)m.d; };
    const M2 m1{ 1.0L - c, (long double)coef[4], -c, (long double)coef[4] };
    M2 mc{ 1.0L, 0.0L, 0.0L, 1.0L };
    for (int i = 0; i < kMeterChunk; ++i) mc = mul(m1, mc);           // M^chunk
    M2 p = mc;
    for (int k = 0; k < kMeterScanSteps; ++k) { put(out + 8 + 4 * k, p); p = mul(p, p); }
    M2 q{ 1.0L, 0.0L, 0.0L, 1.0L };
    for (int l = 0; l < 64; ++l) { put(out + 8 + 4 * kMeterScanSteps + 4 * l, q); q = mul(mc, q); }
}

}  // namespace cpq

extern "C" {

int32_t cpq_meter_kweighting(double rate, double pre[5], double rlb[5])
{
    if (!(rate > 0.0) || !std::isfinite(rate) || !pre || !rlb) return CPQ_ERR_INVALID_ARG;
    cpq::meterKWeighting(rate, pre, rlb);
    return CPQ_OK;
}

int32_t cpq_meter_tp_design_stage(int32_t stage, cpq_os_stage_info* info, double* taps, int32_t capacity)
{
    cpq::OsStage s;
    if (!cpq::meterTpDesignStage(stage, s)) return CPQ_ERR_INVALID_ARG;
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

}  // extern "C"
