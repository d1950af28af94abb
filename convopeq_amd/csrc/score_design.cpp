// score_design.cpp -- host side of the shaper scorer: MklFftEvaluator::configureForSampleRate (src/MklFftEvaluator.h:143-242) and
// the per-bin constants evaluate() recomputes for every call (:351-365, :613-628), buildTrainingSegments' window selection
// (src/NoiseShaperLearner.cpp:1185-1270), the generator start states of every (candidate, segment), and the two small tests of a
// candidate (isStable, the tanh / clampCoeff mapping).  No GPU.  Every expression is the reference's, in its order.
#include "host_design.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace cpq {

namespace {

constexpr double kReferenceSplDb = 90.0, kCalibrationOffsetDb = 0.0;

double dbToPower(double db) { return std::pow(10.0, db / 10.0); }

double freqToBark(double hz)
{
    const double f = std::max(0.0, hz);
    return 13.0 * std::atan(0.00076 * f) + 3.5 * std::atan(std::pow(f / 7500.0, 2.0));
}

double athSplDb(double hz)
{
    const double fKHz = std::max(0.01, hz / 1000.0);
    const double f2 = fKHz * fKHz;
    const double term1 = 3.64 * std::pow(fKHz, -0.8);
    const double term2 = -6.5 * std::exp(-0.6 * std::pow(fKHz - 3.3, 2.0));
    const double term3 = 0.001 * f2 * f2;
    return term1 + term2 + term3;
}

double jndDb(double hz)
{
    const double f = std::max(0.0, hz / 1000.0);
    const double lowPeak = 1.0 * std::exp(-0.5 * (f - 0.5) * (f - 0.5));
    const double highShape = 0.2 * (f - 3.0) * (f - 3.0);
    return std::clamp(0.5 + lowPeak + highShape, 0.5, 3.0);
}

int neighborRange(double hz, double binWidthHz)
{
    const double fKHz = std::max(0.0, hz / 1000.0);
    const double bandwidth = 25.0 + 75.0 * std::pow(1.0 + 1.4 * fKHz * fKHz, 0.69);
    const int range = static_cast<int>((bandwidth / std::max(1.0, binWidthHz)) * 0.5);
    return std::clamp(range, 1, 24);
}

void spreadTable(double downDbPerBark, std::vector<double>& table)
{
    table.resize(kScoreSpreadBins);
    for (int i = 0; i < kScoreSpreadBins; ++i) {
        const double deltaBark = -8.0 + static_cast<double>(i) * 0.01;
        if (deltaBark >= 0.0) { table[i] = -27.0 * deltaBark; continue; }
        const double x = deltaBark + 0.474;
        const double nonLinear = 15.81 + 7.5 * x - 17.5 * std::sqrt(1.0 + (x * x));
        table[i] = nonLinear + (downDbPerBark + 27.0) * std::abs(deltaBark);
    }
}

unsigned long long rotl(unsigned long long x, int k) { return (x << k) | (x >> (64 - k)); }

void step(unsigned long long s[4])
{
    const unsigned long long t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = rotl(s[3], 45);
}

}  // namespace

bool scoreTables(double rate, ScoreTables& t)
{
    constexpr int nBins = kScoreBins;
    const double safeRate = std::max(1.0, rate);
    const double nyquistHz = 0.5 * safeRate;
    const double binWidthHz = nyquistHz / static_cast<double>(nBins - 1);
    auto hzToBin = [binWidthHz](double hz) {
        if (binWidthHz <= 0.0) return 0;
        return std::clamp(static_cast<int>(std::lround(hz / binWidthHz)), 0, nBins - 1);
    };
    t.rate = safeRate;
    t.flatWeight = 0.35;
    t.hfWeight = std::clamp(0.20 * std::sqrt(48000.0 / safeRate), 0.05, 0.20);

    double flatnessStartHz = std::min(12000.0, nyquistHz * 0.60);
    double flatnessEndHz = std::min(18000.0, nyquistHz * 0.82);
    if (flatnessEndHz <= flatnessStartHz + (binWidthHz * 8.0)) {
        flatnessStartHz = nyquistHz * 0.50;
        flatnessEndHz = nyquistHz * 0.80;
    }
    t.flatStart = hzToBin(flatnessStartHz);
    t.flatEnd = std::max(t.flatStart + 1, hzToBin(flatnessEndHz));

    double highBandStartHz = std::max(14000.0, nyquistHz * 0.60);
    if (highBandStartHz >= nyquistHz) highBandStartHz = nyquistHz * 0.60;
    double ultraHighStartHz = nyquistHz * 0.85;
    if (ultraHighStartHz <= highBandStartHz + (binWidthHz * 8.0)) ultraHighStartHz = highBandStartHz + (binWidthHz * 8.0);
    t.highStart = hzToBin(highBandStartHz);
    t.ultraStart = std::max(t.highStart + 1, hzToBin(ultraHighStartHz));
    const int highBandBins = std::max(1, nBins - t.highStart);
    const int ultraHighBins = std::max(1, nBins - t.ultraStart);
    t.ultraShare = static_cast<double>(ultraHighBins) / static_cast<double>(highBandBins);

    auto bandWeightForHz = [nyquistHz](double f) {
        if (f < 1.0) f = 1.0;
        const double f2 = f * f;
        const double h1 = -4.737338981378384e-24 * f2 * f2 * f2 + 2.043828333606125e-15 * f2 * f2 - 1.363894795463638e-7 * f2 + 1.0;
        const double h2 = 1.306612257402824e-19 * f2 * f2 * f - 2.118150887541247e-11 * f2 * f + 5.559488023498642e-4 * f;
        const double r_f = (1.246332637532143e-4 * f) / std::sqrt(h1 * h1 + h2 * h2);
        double w = r_f * r_f;
        if (f > 18000.0) {
            const double rollOff = std::pow(10.0, -12.0 * (f - 18000.0) / std::max(1000.0, nyquistHz - 18000.0) / 20.0);
            w *= rollOff * rollOff;
        }
        return std::max(1.0e-6, w);
    };

    const double maxBark = freqToBark(nyquistHz);
    const double barkStep = std::max(1.0e-9, maxBark / static_cast<double>(kScoreBands));
    std::vector<double> freq(nBins);
    for (auto* v : { &t.weight, &t.bark, &t.athDb, &t.athPow, &t.width, &t.thrSpread }) v->assign(nBins, 0.0);
    t.band.assign(nBins, 0);
    t.range.assign(nBins, 0);
    t.weightSum = 0.0;
    for (int bin = 0; bin < nBins; ++bin) {
        const double hz = static_cast<double>(bin) * binWidthHz;
        const double bark = freqToBark(hz);
        const double athDb = athSplDb(hz) - kReferenceSplDb + kCalibrationOffsetDb;
        freq[bin] = hz;
        t.bark[bin] = bark;
        t.athDb[bin] = athDb;
        t.athPow[bin] = dbToPower(athDb);
        t.range[bin] = neighborRange(hz, binWidthHz);
        t.band[bin] = std::clamp(static_cast<int>(bark / barkStep), 0, kScoreBands - 1);
        // evaluate(): weight = weights[idx] * jndWeight, psychoWeightSum += weight
        const double jndWeight = 1.0 / std::max(1.0e-6, jndDb(hz) + 0.3);
        t.weight[bin] = bandWeightForHz(hz) * jndWeight;
        t.weightSum += t.weight[bin];
        // precomputeMaskingThresholds: freq = k * ((sampleRate * 0.5) / 2048), the same product; computeMaskingThreshold
        t.thrSpread[bin] = dbToPower(-12.0 - (0.6 * bark));
    }
    for (int bin = 0; bin < nBins; ++bin)          // getBinWidth
        t.width[bin] = bin <= 0 ? freq[1] - freq[0] : bin >= nBins - 1 ? freq[nBins - 1] - freq[nBins - 2] : 0.5 * (freq[bin + 1] - freq[bin - 1]);
    for (int bin = 1; bin < nBins; ++bin)
        if (t.band[bin] < t.band[bin - 1]) return false;
    for (int b = 0, bin = 0; b <= kScoreBands; ++b) {
        while (bin < nBins && t.band[bin] < b) ++bin;
        t.bandStart[b] = bin;
    }
    spreadTable(-24.0, t.spreadTonal);
    spreadTable(-27.0, t.spreadNoise);
    return true;
}

int scoreSelectSegments(const double* l, const double* r, int n, ScoreSegment out[kScoreMaxSegments], int counts[kScoreLevels])
{
    for (int i = 0; i < kScoreLevels; ++i) counts[i] = 0;
    const int usable = std::min(n, kScoreRecent);
    if (usable < kScoreLen || !l || !r) return 0;
    l += n - usable;                                        // copyLatest: the most recent samples, oldest first
    r += n - usable;
    ScoreSegment bucket[kScoreLevels][kScorePerLevel];
    int total = 0;
    for (int start = 0; start + kScoreLen <= usable && total < kScoreMaxSegments; start += kScoreHop) {
        double sumSquares = 0.0, maxPeak = 0.0;
        for (int i = 0; i < kScoreLen; ++i) {
            const double a = l[start + i], b = r[start + i];
            sumSquares += 0.5 * (a * a + b * b);
            maxPeak = std::max(maxPeak, std::max(std::abs(a), std::abs(b)));
        }
        const double rms = std::sqrt(sumSquares / static_cast<double>(kScoreLen));
        if (rms < 1.0e-5) continue;                         // kMinRMS
        const double crestFactor = (rms > 1e-9) ? (maxPeak / rms) : 1.0;
        int type = CPQ_SEGMENT_BROADBAND;
        if (crestFactor > 5.0) type = CPQ_SEGMENT_TRANSIENT;
        else if (crestFactor < 1.6) type = CPQ_SEGMENT_TONAL;
        for (int i = 0; i < kScoreLevels; ++i) {
            if (counts[i] >= kScorePerLevel) continue;
            const double targetRMS = std::pow(10.0, kScoreLevelsDb[i] / 20.0);
            double gain = targetRMS / rms;
            if (maxPeak * gain > 0.95) gain = 0.95 / maxPeak;       // kPeakHeadroom
            bucket[i][counts[i]++] = ScoreSegment{ start, i, type, gain, targetRMS };
            ++total;
        }
    }
    int at = 0;
    for (int i = 0; i < kScoreLevels; ++i)
        for (int j = 0; j < counts[i]; ++j) out[at++] = bucket[i][j];
    return total;
}

void scoreRngTable(const unsigned long long start[2][4], int count, std::vector<unsigned long long>& table)
{
    table.assign((size_t)std::max(count, 0) * 8, 0ULL);
    for (int ch = 0; ch < 2; ++ch) {
        unsigned long long s[4];
        std::memcpy(s, start[ch], sizeof(s));
        for (int j = 0; j < count; ++j) {
            std::memcpy(&table[((size_t)j * 2 + ch) * 4], s, sizeof(s));
            for (int k = 0; k < kScoreWordsPerSegment; ++k) step(s);
        }
    }
}

bool scoreStable(const double* k, int n)
{
    for (int i = 0; i < n; ++i)
        if (std::abs(k[i]) >= 1.0 - 1e-12) return false;     // a NaN is not refused here, as in the reference; clampCoeff zeroes it
    return true;
}

void scoreMapRaw(const double* raw, double margin, double out[kLatticeOrder])
{
    for (int i = 0; i < kLatticeOrder; ++i) {
        const double k = std::tanh(raw[i]);
        out[i] = !std::isfinite(k) ? 0.0 : k > margin ? margin : k < -margin ? -margin : k;
    }
}

}  // namespace cpq
