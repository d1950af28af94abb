// host_design.hpp -- host-side design math (layer plan, h_eff, SVF coefficients). See host_design.cpp.
#pragma once

#include <vector>

#include "convopeq_mi355x.h"

namespace cpq {

// geometry of the time-parallel SVF kernels (svf_kernels.hip), shared with buildSvfTpTables()
// chunk lengths with a table block each: 16 (spans of 8192 / 1024 x waves samples: k_svf_cascade_tpv), 8 (spans below 1024
// samples on one or two waves: k_svf_cascade_short)
constexpr int kSvfTpLcCount = 2;
constexpr int kSvfTpLc[kSvfTpLcCount] = { 16, 8 };
// the tables of one (stream, band), as the builder fills them and the kernels read them; A = the band's 2x2 state matrix
struct TpLcTables {         // one per chunk length LC
    double Mk[6][4];        // A^(LC 2^k), row-major 2x2: in-wave scan steps
    double Mw[4];           // A^(LC 64): one whole wave of chunks
    double P[64][4];        // A^(LC (c+1)): carries the wave's start state to the end of chunk c
};
struct TpBandTables {
    TpLcTables t[kSvfTpLcCount];
    double e[2][16];        // e[:, k] = A^(15-k) B: end state of a 16-sample chunk's zero-state run (its last LC columns serve a chunk of LC)
};
constexpr int kSvfTpTableDoubles = (int)(sizeof(TpBandTables) / sizeof(double));

int    computeNucPlan(int irLen, int blockSize, bool enableDirectHead, const cpq_filter_spec* spec,
                      cpq_nuc_plan* out);
int    buildHeff(const double* ir, int irLen, int blockSize, double scale, const cpq_filter_spec* spec,
                 std::vector<double>& heff, cpq_nuc_plan* planOut);
void   spectrumFilterGains(const cpq_filter_spec& spec, int N, std::vector<double>& gains);
bool   airAbsorptionGains(const cpq_filter_spec& spec, int layer, int complexSize, std::vector<double>& gains);
void   designSvf(int type, float freq, float gainDb, float q, double sr, cpq_svf_coeffs* c);
void   defaultEqParams(cpq_eq_params* p);
double totalGainLinear(float db);
// Tables of the time-parallel SVF kernels for one band (out: one TpBandTables, kSvfTpTableDoubles doubles).
// Returns false when the state guards of the reference could
// trip for inputs / carried states below 1e9 (or the filter does not decay), i.e. the kernel must not be used.
bool   buildSvfTpTables(const cpq_svf_coeffs& c, double* out);
bool   buildBiquadTpTables(const cpq_biquad_coeffs& q, double* out);
void   designOutputFilter(int convIsLast, int hcMode, int lcMode, int lpMode, double fs, cpq_biquad_coeffs out[3]);

// one half-band stage of the oversampler (os_design.cpp; CustomInputOversampler::prepareStage)
struct OsStage {
    int taps = 0, centerTap = 0, centerParity = 0, convParity = 0, convCount = 0;
    int centerDelayInput = 0, historyUpKeep = 0, historyDownKeep = 0;
    double attenuationDb = 0.0, centerCoeff = 0.0;
    std::vector<double> raw;        // [taps]
    std::vector<double> conv;       // [convCount] raw[convParity + 2 r]
};
bool   osDesignStage(int stage, int type, OsStage& out);
void   osDesignHalfband(int taps, double attenuationDb, OsStage& out);     // the design behind it, for any tap count
// meters (meter_design.cpp): LoudnessMeter::updateCoefficients, TruePeakDetector's two stages, and the tables of the
// time-parallel K-weighting kernel
void   meterKWeighting(double fs, double pre[5], double rlb[5]);
bool   meterTpDesignStage(int stage, OsStage& out);
constexpr int kMeterChunk = 8;          // samples a lane of the K-weighting kernel holds
constexpr int kMeterScanSteps = 7;      // powers M^(chunk * 2^k): k < 6 the scan inside a wave, k = 6 one whole wave (64 lanes)
// per section: {b0, b1, b2, a1, a2, c = 1 + a1 + a2, -, -}, then M^(chunk * 2^k) for k < 7, then M^(chunk * lane) for lane < 64
// (row-major 2x2, M = [[1 - c, a2], [-c, a2]] acting on (y[n-1], y[n-1] - y[n-2])), computed in long double
constexpr int kMeterSectionDoubles = 8 + 4 * kMeterScanSteps + 4 * 64;
void   meterSectionTables(const double coef[5], double* out);
int    osStagesFor(int factor);     // 1/2/4/8 -> 0/1/2/3 stages, else -1
// output stage (out_design.cpp): the base-rate steps of DSPCore::processOutputDouble with dither off
constexpr double kOutHeadroom = 0.8912509381337456;             // kOutputHeadroom, -1 dBFS
constexpr double kOutLimiterThreshold = 0.8413951287507587;     // kPLThreshold
constexpr double kOutLimiterKnee = 0.108748;                    // kPLKnee
void   outDesign(double fs, double alpha[2], double* releaseCoeff);     // UltraHighRateDCBlocker::init(fs, 3), SimplePeakLimiter::prepare(fs, 100)
constexpr int kOutChunk = 8;            // samples a lane of the DC kernel holds
constexpr int kOutScanSteps = 7;        // powers a^(chunk * 2^k): k < 6 the scan inside a wave, k = 6 one whole wave
// per one-pole section: {alpha, a^(chunk * 2^k) for k < 7, a^(chunk * lane) for lane < 64}, a = 1 - alpha, in long double
constexpr int kOutSectionDoubles = 1 + kOutScanSteps + 64;
void   outSectionTable(double alpha, double* out);
double outDesiredGain(double l, double r);      // SimplePeakLimiter's desiredGain of one stereo sample
double outClamp(double v);
// one stream of the stage, sequential, in the reference's operation order; a call of process() is one callback
struct OutStageHost {
    double alpha[2] = { 1.0e-6, 1.0e-6 }, releaseCoeff = 0.0;
    double dc[2][2] = { { 0.0, 0.0 }, { 0.0, 0.0 } };       // [channel][section]
    double envelope = 1.0;
    void prepare(double fs);
    void reset();
    void process(double* l, double* r, int n, int flags);   // flags: CPQ_OUT_*
};

// dither stage (dither_design.cpp): FixedNoiseShaper / Fixed15TapNoiseShaper / LatticeNoiseShaper of the reference
constexpr int kDitherMaxOrder = 16;
constexpr int kLatticeOrder = 9;        // LatticeNoiseShaper::kOrder
inline int ditherOrder(int shaper)
{
    return shaper == CPQ_DITHER_FIXED4 ? 4 : shaper == CPQ_DITHER_FIXED15 ? 16 : shaper == CPQ_DITHER_ADAPTIVE9 ? kLatticeOrder : 0;
}
// prepare(rate, bits): coeffs[16] (unused taps 0.0), scale = 2^-(bits - 1); false for an unknown shaper or bits outside 1..32.
// The adaptive shaper: kDefaultAdaptiveNoiseShaperCoeffs whatever the rate
bool   ditherDesign(double rate, int shaper, int bits, double coeffs[kDitherMaxOrder], double* scale);
// xoshiro256++ state of channel ch (0 = L, 1 = R): the 4-tap and the lattice header's constants, or initializeRandomStates(rate, bits)
void   ditherSeed(int shaper, double rate, int bits, int ch, unsigned long long s[4]);
// LatticeNoiseShaper::setCoefficients: out[9] = clampCoeff of k[0 .. n - 1] (not finite -> 0, else clamped to +-0.85), the rest 0
void   ditherClampAdaptive(const double* k, int n, double out[kLatticeOrder]);
// one stream of the stage, sequential, in the reference's operation order: processStereoBlock(l, r, n, headroom)
struct DitherHost {
    int shaper = CPQ_DITHER_OFF, order = 0, bits = 0;
    double coeffs[kDitherMaxOrder] = {}, scale = 1.0, invScale = 1.0;
    double err[2][kDitherMaxOrder] = {};        // [channel][k], k = 0 the newest; the lattice's states in k = 0 .. 8
    unsigned long long rng[2][4] = {};
    bool configure(double rate, int shaperId, int bitDepth);    // a new shaper object + prepare(): errors cleared, seeded
    // prepare() again: errors cleared, the 15-tap shaper reseeded; the adaptive shaper keeps its coefficients (the published set
    // is applied again at the first callback)
    void prepare(double rate);
    void reset();                                               // errors only
    bool setAdaptiveCoeffs(const double* k, int n);             // applyMatchedCoefficients; false unless adaptive, n in 0..9
    void process(double* l, double* r, int n, double headroom);
};

// shaper scorer (score_design.cpp): the deterministic host parts of NoiseShaperLearner's fitness function
constexpr int kScoreLen = 4096;                 // AudioSegment::kLength = MklFftEvaluator::kFftLength
constexpr int kScoreBins = kScoreLen / 2 + 1;   // kSpectrumBins
constexpr int kScoreHop = kScoreLen / 2;        // kSegmentHop
constexpr int kScoreLevels = 4, kScorePerLevel = 4, kScoreMaxSegments = kScoreLevels * kScorePerLevel;
constexpr int kScoreRecent = kScoreLen + kScoreHop * (kScoreMaxSegments - 1);       // kRecentSampleRequest
constexpr int kScoreBands = 24;                 // kBarkBandCount
constexpr int kScoreSpreadBins = 1601;          // kSpreadTableBins
constexpr int kScoreWordsPerSegment = 2 * kScoreLen;    // generator words one channel draws over one segment
constexpr double kScoreLevelsDb[kScoreLevels] = { -40.0, -30.0, -20.0, -10.0 };    // kTargetLevelsDB
// MklFftEvaluator::configureForSampleRate (src/MklFftEvaluator.h:143-242) and what evaluate() derives from it per bin
struct ScoreTables {
    double rate = 0.0;
    std::vector<double> weight;         // weights[bin] * computeJndWeight(computeJndDb(freqHz[bin])): the factor of the psycho sum
    std::vector<double> bark, athDb, athPow, width;     // barkHz, athThresholdDb, athThresholdPower, getBinWidth(bin)
    std::vector<double> thrSpread;      // computeMaskingThreshold's dbToPower(-12 - 0.6 bark) at bin * binWidth
    std::vector<int> band, range;       // binToBand, neighborRangeBins
    std::vector<double> spreadTonal, spreadNoise;       // kSpreadTableTonal / kSpreadTableNoise
    int bandStart[kScoreBands + 1] = {};        // bins of band b: [bandStart[b], bandStart[b + 1]); binToBand never decreases
    int flatStart = 0, flatEnd = 0, highStart = 0, ultraStart = 0;
    double ultraShare = 0.0, flatWeight = 0.35, hfWeight = 0.2;
    double weightSum = 0.0;             // the psycho sum's psychoWeightSum, added bin after bin as evaluate() does
};
bool scoreTables(double rate, ScoreTables& t);   // false: binToBand is not monotonic (no rate above 1 Hz gives that)
// buildTrainingSegments (src/NoiseShaperLearner.cpp:1185-1270) on the last min(n, kScoreRecent) samples, without the levelling
// itself: which windows enter which level bucket, with what gain.  out is in evaluation order (level-major, then bucket order)
struct ScoreSegment { int start, level, type; double gain, targetRms; };      // start counts from the first sample used; type: cpq_segment_type
int scoreSelectSegments(const double* l, const double* r, int n, ScoreSegment out[kScoreMaxSegments], int counts[kScoreLevels]);
// table[j][ch][4]: start[ch] advanced by j * kScoreWordsPerSegment draws, j < count
void scoreRngTable(const unsigned long long start[2][4], int count, std::vector<unsigned long long>& table);
// index into that table of segment s of nSeg of the candidate with c candidates run before it
inline int scoreRngIndex(int mode, int c, int nSeg, int s) { return mode == CPQ_SCORE_RNG_CHAINED ? c * nSeg + s : s; }
inline double scoreAlpha(int level) { return kScoreLevelsDb[level] < -30.0 ? 0.3 : kScoreLevelsDb[level] > -15.0 ? 0.7 : 0.5; }
// LatticeNoiseShaper::isStable
bool scoreStable(const double* k, int n);
// evaluateCandidate's mapping: clampCoeff(std::tanh(raw[i]), margin)
void scoreMapRaw(const double* raw, double margin, double out[kLatticeOrder]);

}  // namespace cpq
