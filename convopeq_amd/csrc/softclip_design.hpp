// softclip_design.hpp -- DSPCore's soft clipper (softClipBlockAVX2 / musicalSoftClipScalar,
// src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:107-224; parameters :474-477), memoryless.  The reference runs it per
// channel and per callback with two arithmetic paths, chosen by the sample's index i inside the callback of len samples:
//   body  i <  len / 4 * 4   the 4-wide loop: reciprocals of the knee, t clamped to [0, 1], three fused multiply-adds, the Pade
//                            tanh on an argument clamped to +-4.5, the result selected over x where |x| > threshold - knee
//   tail  i >= len / 4 * 4   the scalar loop: true divisions, no fused operation, the knee shape only below threshold + knee,
//                            tanh = +-1 beyond 4.5
// Both paths of one sample are stated once, here, for the kernel (softclip_kernels.hip) and the host walk (softclip_design.cpp);
// the build keeps -ffp-contract=off, so a fused multiply-add exists exactly where fma() is written.  softClipPrevSample of the
// reference is written and never read and is not built.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CPQ_SC_FN __host__ __device__ inline
#else
#define CPQ_SC_FN inline
#endif

namespace cpq {

// a stream's row of the parameter table: what both paths read, formed once on the host
constexpr int kSoftClipTabDoubles = 8;
enum { kScOn = 0, kScThreshold, kScKnee, kScAsym, kScClipStart, kScRecipKnee, kScRecipKnee2, kScKneeEnd };

// the 4-wide body; max_pd / min_pd return their second operand unless the first compares greater / less (so for a NaN)
CPQ_SC_FN double softClipBody(double x, const double* p)
{
    const double absX = fabs(x);
    if (!(absX > p[kScClipStart])) return x;                    // _CMP_GT_OQ: a NaN passes through
    const double sign = x > 0.0 ? 1.0 : -1.0;
    double t = (absX - p[kScClipStart]) * p[kScRecipKnee2];
    t = t > 0.0 ? t : 0.0;
    t = t < 1.0 ? t : 1.0;
    const double t2 = t * t;
    const double ks = t2 * fma(-2.0, t, 3.0);
    double a = (absX - p[kScThreshold]) * p[kScRecipKnee];
    a = a > -4.5 ? a : -4.5;
    a = a < 4.5 ? a : 4.5;
    const double a2 = a * a;
    const double num = a * (10395.0 + a2 * (1260.0 + a2 * 21.0));
    const double den = 10395.0 + a2 * (4725.0 + a2 * (210.0 + a2));
    const double clipped = fma(p[kScKnee], num / den, p[kScThreshold]);
    const double mixed = fma(clipped - absX, ks, absX);
    const double factor = p[kScAsym] * (1.0 - sign) * 0.5 * ks;
    return sign * (mixed * (1.0 - factor));
}

// the scalar tail: musicalSoftClipScalar behind the loop's own |x| > clip_start test (its knee < 1e-9 branch needs a knee the
// parameter formulas cannot give, its |x| < clip_start return cannot be reached from that loop)
CPQ_SC_FN double softClipTail(double x, const double* p)
{
    const double absX = fabs(x);
    if (!(absX > p[kScClipStart])) return x;
    const double sign = x > 0.0 ? 1.0 : -1.0;
    double ks = 1.0;
    if (absX < p[kScKneeEnd]) {
        const double t = (absX - p[kScClipStart]) / (2.0 * p[kScKnee]);
        ks = t * t * (3.0 - 2.0 * t);
    }
    const double a = (absX - p[kScThreshold]) / p[kScKnee];
    double th;
    if (a >= 4.5) th = 1.0;
    else if (a <= -4.5) th = -1.0;
    else {
        const double a2 = a * a;
        th = a * (10395.0 + a2 * (1260.0 + a2 * 21.0)) / (10395.0 + a2 * (4725.0 + a2 * (210.0 + a2)));
    }
    const double clipped = p[kScThreshold] + p[kScKnee] * th;
    const double gain = 1.0 - p[kScAsym] * (1.0 - sign) * 0.5 * ks;
    return sign * (absX * (1.0 - ks) + clipped * ks) * gain;
}

// sample i of a callback of len samples
CPQ_SC_FN double softClipSample(double x, int i, int len, const double* p)
{
    return i < len / 4 * 4 ? softClipBody(x, p) : softClipTail(x, p);
}

// setSaturationAmount admits [0, 1] (AudioEngine.Parameters.cpp:521-523); not finite or outside it: false
bool softClipAmountValid(float amount);
// threshold, knee and asymmetry of an amount, then what the two paths derive from them; on = false: the row of a stream that rests
void softClipTableRow(bool on, float amount, double row[kSoftClipTabDoubles]);
// rows [nCh][stride], n samples each, walked in callbacks of cb samples (the last one shorter); channel c reads row c / 2 of tab
void softClipRows(double* rows, int64_t stride, int nCh, int n, int cb, const double* tab);

}  // namespace cpq
