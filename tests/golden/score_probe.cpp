// Records what the reference's own LatticeNoiseShaper and MklFftEvaluator compute along NoiseShaperLearner's fitness function,
// for tests/golden/score_ref.npz (make_score_ref.py drives it).  Build, with REF the reference's source tree:
//   g++ -std=c++20 -O2 -ffp-contract=off -msse4.1 -mavx2 -mfma -Itests/golden/score_shim -Itests/golden/juce_shim -I$REF/src
//       tests/golden/score_probe.cpp -o score_probe
// The two headers are the reference's; the transform behind ippsFFTFwd_RToCCS_64f is score_shim/ipp.h's (long double, rounded
// once).  The learner itself needs the whole application, so its two loops are told again here: the windows of
// buildTrainingSegments (hop 2048, RMS gate 1e-5, four target levels, peak headroom 0.95, four segments a level) with
// precomputeMaskingThresholds, and the level / bucket walk of evaluateCandidateMapped with its blend and weights.
//   score_probe <rate> <bits> <mode> <stability> <audio> <candidates> <nCand> <out> <rows>
// audio: L then R (the file's size gives n); candidates: nCand x 9 mapped coefficients; mode 0: a fresh shaper for every
// candidate, 1: one shaper for all of them in order.  out (doubles): nSeg; per segment start, level, gain, type; per segment 2049
// thresholds; per candidate the score; per candidate and segment the five Result members.  rows: per candidate and segment the
// two error rows.
// Evaluate-only mode, for tests/golden/score_edges_ref.npz (make_score_edges_ref.py):
//   score_probe eval <rate> <in> <out> <echo>
// in (doubles): per pair a flag, the two error rows (L, R), and with flag != 0 the 2049 masking thresholds handed to evaluate()
// (flag 0: evaluate() gets none).  out: per pair the five Result members, then computeMaskingThreshold of every bin of the pair's
// 0.5 (|L|^2 + |R|^2).  echo: the rows as they were read.
#include <JuceHeader.h>
#include "DspNumericPolicy.h"
using namespace convo::numeric_policy;
#include "LatticeNoiseShaper.h"
#include "MklFftEvaluator.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr int kLen = MklFftEvaluator::kFftLength, kBins = MklFftEvaluator::kSpectrumBins;
constexpr int kLevels = 4, kPerLevel = 4;
constexpr double kLevelDb[kLevels] = { -40.0, -30.0, -20.0, -10.0 };
constexpr double kWeights[kLevels] = { 0.4, 0.3, 0.2, 0.1 };
constexpr double kHeadroom = 0.8912509381337456;

struct Segment {
    std::vector<double> l, r;
    std::array<double, kBins> thr;
    int start, level, type;
    double gain;
};

std::vector<double> readAll(const char* path)
{
    std::vector<double> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    v.resize((size_t)std::ftell(f) / sizeof(double));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(v.data(), sizeof(double), v.size(), f) != v.size()) v.clear();
    std::fclose(f);
    return v;
}

int evaluateOnly(int argc, char** argv)
{
    if (argc != 6) return 2;
    const double rate = std::strtod(argv[2], nullptr);
    const std::vector<double> in = readAll(argv[3]);
    auto evaluator = std::make_unique<MklFftEvaluator>();
    evaluator->configureForSampleRate(rate);
    const double binWidth = (rate * 0.5) / (kBins - 1);
    std::vector<double> out, echo;
    auto thr = std::make_unique<std::array<double, kBins>>();
    std::vector<MklFftEvaluator::CcsComplex> specL(kBins), specR(kBins);
    size_t at = 0;
    while (at < in.size()) {
        const bool withThr = in[at] != 0.0;
        const size_t need = 1 + 2 * (size_t)kLen + (withThr ? kBins : 0);
        if (in.size() - at < need) return 3;
        const double* l = in.data() + at + 1;
        const double* r = l + kLen;
        if (withThr) std::copy(r + kLen, r + kLen + kBins, thr->begin());
        const auto res = evaluator->evaluate(l, r, withThr ? thr.get() : nullptr);
        for (double v : { res.noisePower, res.spectralFlatnessPenalty, res.hfPenalty, res.timeDomainRms, res.compositeScore }) out.push_back(v);
        evaluator->computeFft(l, r, specL.data(), specR.data());
        for (int k = 0; k < kBins; ++k) {
            const double magSqL = specL[k].real * specL[k].real + specL[k].imag * specL[k].imag;
            const double magSqR = specR[k].real * specR[k].real + specR[k].imag * specR[k].imag;
            out.push_back(evaluator->computeMaskingThreshold(0.5 * (magSqL + magSqR), k * binWidth));
        }
        echo.insert(echo.end(), l, l + 2 * kLen);
        at += need;
    }
    FILE* f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 3;
    std::fclose(f);
    f = std::fopen(argv[5], "wb");
    if (!f || std::fwrite(echo.data(), sizeof(double), echo.size(), f) != echo.size()) return 3;
    std::fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && std::string(argv[1]) == "eval") return evaluateOnly(argc, argv);
    if (argc != 10) return 2;
    const double rate = std::strtod(argv[1], nullptr);
    const int bits = std::atoi(argv[2]), mode = std::atoi(argv[3]), stability = std::atoi(argv[4]), nCand = std::atoi(argv[7]);
    const std::vector<double> audio = readAll(argv[5]), cands = readAll(argv[6]);
    if (audio.empty() || (audio.size() & 1) || cands.size() != (size_t)nCand * 9) return 3;
    const int n = (int)(audio.size() / 2);
    const double* left = audio.data();
    const double* right = audio.data() + n;

    auto evaluator = std::make_unique<MklFftEvaluator>();
    evaluator->configureForSampleRate(rate);

    // the windows, oldest first, over at most the last 4096 + 2048 * 15 samples
    const int usable = std::min(n, kLen + (kLen / 2) * (kLevels * kPerLevel - 1));
    left += n - usable;
    right += n - usable;
    std::vector<std::vector<Segment>> buckets(kLevels);
    int total = 0;
    for (int start = 0; usable >= kLen && start + kLen <= usable && total < kLevels * kPerLevel; start += kLen / 2) {
        double sumSquares = 0.0, maxPeak = 0.0;
        for (int i = 0; i < kLen; ++i) {
            const double a = left[start + i], b = right[start + i];
            sumSquares += 0.5 * (a * a + b * b);
            maxPeak = std::max(maxPeak, std::max(std::abs(a), std::abs(b)));
        }
        const double rms = std::sqrt(sumSquares / static_cast<double>(kLen));
        if (rms < 1.0e-5) continue;
        const double crest = (rms > 1e-9) ? (maxPeak / rms) : 1.0;
        const int type = crest > 5.0 ? 2 : crest < 1.6 ? 1 : 0;          // Broadband 0, Tonal 1, Transient 2
        for (int lv = 0; lv < kLevels; ++lv) {
            if ((int)buckets[lv].size() >= kPerLevel) continue;
            const double target = std::pow(10.0, kLevelDb[lv] / 20.0);
            double gain = target / rms;
            if (maxPeak * gain > 0.95) gain = 0.95 / maxPeak;
            Segment sg;
            sg.start = start; sg.level = lv; sg.type = type; sg.gain = gain;
            sg.l.resize(kLen);
            sg.r.resize(kLen);
            for (int i = 0; i < kLen; ++i) { sg.l[i] = left[start + i] * gain; sg.r[i] = right[start + i] * gain; }
            std::vector<MklFftEvaluator::CcsComplex> specL(kBins), specR(kBins);
            evaluator->computeFft(sg.l.data(), sg.r.data(), specL.data(), specR.data());
            const double binWidth = (rate * 0.5) / (kBins - 1);
            for (int k = 0; k < kBins; ++k) {
                const double magSqL = specL[k].real * specL[k].real + specL[k].imag * specL[k].imag;
                const double magSqR = specR[k].real * specR[k].real + specR[k].imag * specR[k].imag;
                sg.thr[k] = evaluator->computeMaskingThreshold(0.5 * (magSqL + magSqR), k * binWidth);
            }
            buckets[lv].push_back(std::move(sg));
            ++total;
        }
    }

    std::vector<double> out;
    out.push_back(total);
    for (auto& b : buckets)
        for (auto& sg : b) { out.push_back(sg.start); out.push_back(sg.level); out.push_back(sg.gain); out.push_back(sg.type); }
    for (auto& b : buckets)
        for (auto& sg : b) out.insert(out.end(), sg.thr.begin(), sg.thr.end());

    FILE* rows = std::fopen(argv[9], "wb");
    if (!rows) return 3;
    std::vector<double> scores, results;
    std::vector<double> shapedL(kLen), shapedR(kLen), errL(kLen), errR(kLen);
    auto shared = std::make_unique<LatticeNoiseShaper>();
    const auto t0 = std::chrono::steady_clock::now();
    for (int c = 0; c < nCand; ++c) {
        const double* k = cands.data() + (size_t)c * 9;
        if (stability && !LatticeNoiseShaper::isStable(k, 9)) { scores.push_back(1e18); continue; }
        auto fresh = std::make_unique<LatticeNoiseShaper>();
        LatticeNoiseShaper& shaper = mode == 1 ? *shared : *fresh;
        shaper.prepare(bits);
        shaper.setCoefficients(k, 9);
        double totalWeighted = 0.0, totalWeight = 0.0;
        for (int lv = 0; lv < kLevels; ++lv) {
            const int count = (int)buckets[lv].size();
            if (count == 0) continue;
            double sum = 0.0;
            for (auto& sg : buckets[lv]) {
                shaper.reset();
                shapedL = sg.l;
                shapedR = sg.r;
                shaper.processStereoBlock(shapedL.data(), shapedR.data(), kLen, kHeadroom);
                for (int i = 0; i < kLen; ++i) {
                    errL[i] = shapedL[i] - (sg.l[i] * kHeadroom);
                    errR[i] = shapedR[i] - (sg.r[i] * kHeadroom);
                }
                std::fwrite(errL.data(), sizeof(double), kLen, rows);
                std::fwrite(errR.data(), sizeof(double), kLen, rows);
                const auto res = evaluator->evaluate(errL.data(), errR.data(), &sg.thr);
                for (double v : { res.noisePower, res.spectralFlatnessPenalty, res.hfPenalty, res.timeDomainRms, res.compositeScore }) results.push_back(v);
                double alpha = 0.5;
                if (kLevelDb[lv] < -30.0) alpha = 0.3;
                else if (kLevelDb[lv] > -15.0) alpha = 0.7;
                const double timeScore = res.timeDomainRms * 1000.0;
                const double freqScore = std::sqrt(res.compositeScore / MklFftEvaluator::kFftLength) * 1000.0;
                sum += (alpha * freqScore + (1.0 - alpha) * timeScore);
            }
            const double average = sum / count;
            totalWeighted += average * kWeights[lv];
            totalWeight += kWeights[lv];
        }
        scores.push_back(totalWeight <= 0.0 ? std::numeric_limits<double>::max() : totalWeighted / totalWeight);
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fclose(rows);
    std::printf("candidates %d segments %d seconds %.6f\n", nCand, total, seconds);
    out.insert(out.end(), scores.begin(), scores.end());
    out.insert(out.end(), results.begin(), results.end());
    FILE* f = std::fopen(argv[8], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 3;
    std::fclose(f);
    return 0;
}
