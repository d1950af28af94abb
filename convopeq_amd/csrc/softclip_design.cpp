// softclip_design.cpp -- host side of DSPCore's soft clipper: the parameters of a saturation amount
// (src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:474-477), the table row the kernel reads, and the block walk of
// softClipBlockAVX2 (:133-224) over rows, sequentially; the two arithmetic paths are softclip_design.hpp's.  No GPU.
#include "softclip_design.hpp"

#include "convopeq_mi355x.h"

namespace cpq {

bool softClipAmountValid(float amount) { return std::isfinite(amount) && amount >= 0.0f && amount <= 1.0f; }

void softClipTableRow(bool on, float amount, double row[kSoftClipTabDoubles])
{
    const double sat = (double)amount;
    const double threshold = 0.95 - 0.45 * sat;
    const double knee = 0.05 + 0.35 * sat;
    row[kScOn] = on ? 1.0 : 0.0;
    row[kScThreshold] = threshold;
    row[kScKnee] = knee;
    row[kScAsym] = 0.10 * sat;
    row[kScClipStart] = threshold - knee;
    row[kScRecipKnee] = 1.0 / knee;
    row[kScRecipKnee2] = 1.0 / (2.0 * knee);
    row[kScKneeEnd] = threshold + knee;
}

void softClipRows(double* rows, int64_t stride, int nCh, int n, int cb, const double* tab)
{
    if (!rows || !tab || n <= 0 || cb <= 0) return;
    for (int c = 0; c < nCh; ++c) {
        const double* p = tab + (int64_t)(c / 2) * kSoftClipTabDoubles;
        if (p[kScOn] == 0.0) continue;
        double* x = rows + c * stride;
        for (int o = 0; o < n; o += cb) {
            const int len = n - o < cb ? n - o : cb;
            for (int i = 0; i < len; ++i) x[o + i] = softClipSample(x[o + i], i, len, p);
        }
    }
}

}  // namespace cpq

extern "C" {

int32_t cpq_soft_clip_params(float amount, double* threshold, double* knee, double* asymmetry)
{
    if (!threshold || !knee || !asymmetry || !cpq::softClipAmountValid(amount)) return CPQ_ERR_INVALID_ARG;
    double row[cpq::kSoftClipTabDoubles];
    cpq::softClipTableRow(true, amount, row);
    *threshold = row[cpq::kScThreshold];
    *knee = row[cpq::kScKnee];
    *asymmetry = row[cpq::kScAsym];
    return CPQ_OK;
}

int32_t cpq_soft_clip_host(double* data, int32_t nSamples, int32_t callbackLen, float amount)
{
    if (!data || nSamples <= 0 || callbackLen <= 0 || !cpq::softClipAmountValid(amount)) return CPQ_ERR_INVALID_ARG;
    double row[cpq::kSoftClipTabDoubles];
    cpq::softClipTableRow(true, amount, row);
    cpq::softClipRows(data, nSamples, 1, nSamples, callbackLen, row);
    return CPQ_OK;
}

double cpq_soft_clip_latency(int32_t factor) { return factor == 1 ? 15.0 : 0.0; }

}  // extern "C"
