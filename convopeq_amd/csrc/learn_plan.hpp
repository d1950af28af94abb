// learn_plan.hpp -- the arithmetic of cpq_learner (the reference's CmaEsOptimizer, src/CmaEsOptimizer.h, and the best tracking of
// NoiseShaperLearner's generation loop), stated once for the kernels (learn_kernels.hip: k_learn_ask, k_learn_tell), for the host
// entries of engine_learn.cpp (cpq_learn_*_host) and for tests/sanitize/learn_plan_check.cpp, which restates both kernels as host
// loops.  No HIP include: what both sides call is CPQ_HD.  Every function is written per element (one variate pair, one factor,
// one candidate entry, one covariance entry), so that a kernel may deal the elements to lanes and the host may loop over them:
// the operations of an element, and their order, are the same text.  Only learnLog and learnTanh differ between the sides (each
// side's math library); everything else is + - * /, sqrt and comparisons, correctly rounded on both under -ffp-contract=off.
//
// Layouts: z, candidates, mapped [18][9] candidate-major; the covariance as cpq_learn_state keeps it, the 45 entries of the upper
// triangle by rows.  update() computes its 81 entries each on its own from products yRow * yColumn summed over the elite in one
// order; a product does not depend on the order of its factors, so entry (r, c) and entry (c, r) are the same bits and the 45 are
// all there is to keep.
#pragma once

#include "convopeq_mi355x.h"

#include <cfloat>
#include <cmath>
#include <cstdint>

#if !defined(CPQ_HD)
#if defined(__HIPCC__)
#define CPQ_HD __host__ __device__
#else
#define CPQ_HD
#endif
#endif

namespace cpq {

constexpr int kLearnDim = CPQ_LEARN_DIM;
constexpr int kLearnPop = CPQ_LEARN_POPULATION;
constexpr int kLearnElite = CPQ_LEARN_ELITE;
constexpr int kLearnVars = kLearnPop * kLearnDim;           // 162
constexpr int kLearnPairs = kLearnVars / 2;                 // 81
constexpr int kLearnCov = kLearnDim * (kLearnDim + 1) / 2;  // 45
constexpr int kLearnMaxTries = CPQ_LEARN_MAX_TRIES;
static_assert(kLearnVars % 2 == 0, "the polar method fills z in pairs");

CPQ_HD inline double learnLog(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ::log(x);
#else
    return std::log(x);
#endif
}

CPQ_HD inline double learnTanh(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ::tanh(x);
#else
    return std::tanh(x);
#endif
}

CPQ_HD inline double learnSqrt(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ::sqrt(x);
#else
    return std::sqrt(x);
#endif
}

CPQ_HD inline double learnAbs(double x) { return x < 0.0 ? -x : x; }      // of a NaN: the NaN
// CmaEsOptimizer::sanitize
CPQ_HD inline double learnSanitize(double x)
{
    const double a = learnAbs(x);
    return (!(a <= DBL_MAX) || a < 1e-15) ? 0.0 : x;
}
// std::clamp, std::min, std::max as the library defines them (a NaN v stays)
CPQ_HD inline double learnClamp(double v, double lo, double hi) { return v < lo ? lo : (hi < v ? hi : v); }
CPQ_HD inline double learnMin(double a, double b) { return b < a ? b : a; }
CPQ_HD inline double learnMax(double a, double b) { return a < b ? b : a; }

// entry (r, c) of the symmetric covariance in the 45
CPQ_HD inline int learnCovIndex(int r, int c)
{
    if (c < r) { const int t = r; r = c; c = t; }
    return r * kLearnDim - (r * (r - 1)) / 2 + (c - r);
}

// ---- generator: xoshiro256++ (the dither stage's, lattice_device.hpp) and splitmix64 for seeds
CPQ_HD inline uint64_t learnRotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
CPQ_HD inline uint64_t learnWord(uint64_t* s)
{
    const uint64_t result = learnRotl(s[0] + s[3], 23) + s[0];
    const uint64_t t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = learnRotl(s[3], 45);
    return result;
}
CPQ_HD inline double learnUniform(uint64_t* s) { return (double)(learnWord(s) >> 11) * (1.0 / 9007199254740992.0); }

inline void learnSeed(uint64_t seed, uint64_t rng[4])
{
    for (int i = 0; i < 4; ++i) {
        seed += 0x9E3779B97F4A7C15ULL;
        uint64_t z = seed;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        rng[i] = z ^ (z >> 31);
    }
}

// One pair by Marsaglia's polar method; returns the words drawn.  After kLearnMaxTries refused tries: (0, 0), *rejected + 1.
CPQ_HD inline int learnNormalPair(uint64_t* rng, double* z0, double* z1, int* rejected)
{
    for (int t = 1; t <= kLearnMaxTries; ++t) {
        const double v1 = 2.0 * learnUniform(rng) - 1.0;
        const double v2 = 2.0 * learnUniform(rng) - 1.0;
        const double s = v1 * v1 + v2 * v2;
        if (0.0 < s && s < 1.0) {
            const double m = learnSqrt((-2.0 * learnLog(s)) / s);
            *z0 = v1 * m;
            *z1 = v2 * m;
            return 2 * t;
        }
    }
    *z0 = 0.0;
    *z1 = 0.0;
    *rejected += 1;
    return 2 * kLearnMaxTries;
}

// z[162] in the reference's order of use (candidate-major); returns the words drawn
CPQ_HD inline int learnNormals(uint64_t* rng, double* z, int* rejected)
{
    int words = 0;
    for (int i = 0; i < kLearnPairs; ++i) words += learnNormalPair(rng, z + 2 * i, z + 2 * i + 1, rejected);
    return words;
}

// ---- ask: CmaEsOptimizer::computeCholesky and sample
// lower[9][9]; only row >= column is written and read
CPQ_HD inline void learnCholesky(const double* covUpper, double* lower)
{
    for (int row = 0; row < kLearnDim; ++row) {
        for (int column = 0; column <= row; ++column) {
            double sum = covUpper[learnCovIndex(row, column)];
            for (int k = 0; k < column; ++k) sum -= lower[row * kLearnDim + k] * lower[column * kLearnDim + k];
            if (row == column) lower[row * kLearnDim + column] = learnSqrt(learnMax(sum, 1.0e-9));
            else lower[row * kLearnDim + column] = sum / learnMax(lower[column * kLearnDim + column], 1.0e-9);
        }
    }
}

// candidates[p][dim]
CPQ_HD inline double learnCandidate(const double* mean, double sigma, const double* lower, const double* z, int p, int dim)
{
    double correlated = 0.0;
    for (int column = 0; column <= dim; ++column) correlated += lower[dim * kLearnDim + column] * z[p * kLearnDim + column];
    return learnSanitize(mean[dim] + sigma * correlated);
}

// evaluatePopulation's mapping: LatticeNoiseShaper::clampCoeff(tanh(candidate), margin)
CPQ_HD inline double learnMap(double candidate, double margin)
{
    const double k = learnTanh(candidate);
    return !(learnAbs(k) <= DBL_MAX) ? 0.0 : (k > margin ? margin : (k < -margin ? -margin : k));
}
// LatticeNoiseShaper::setCoefficients' clampCoeff of a mapped value (host_design's ditherClampAdaptive, per entry)
CPQ_HD inline double learnShaperCoeff(double mapped)
{
    return !(learnAbs(mapped) <= DBL_MAX) ? 0.0 : (mapped > 0.85 ? 0.85 : (mapped < -0.85 ? -0.85 : mapped));
}
// NoiseShaperLearner::isStable's refusal of one value (score_design's scoreStable)
CPQ_HD inline bool learnRefused(double mapped) { return learnAbs(mapped) >= 1.0 - 1e-12; }

inline void learnAsk(const cpq_learn_state& st, const double* z, double* candidates)
{
    double lower[kLearnDim * kLearnDim] = {};
    learnCholesky(st.cov_upper, lower);
    for (int p = 0; p < kLearnPop; ++p)
        for (int dim = 0; dim < kLearnDim; ++dim) candidates[p * kLearnDim + dim] = learnCandidate(st.mean, st.sigma, lower, z, p, dim);
}

// ---- tell: CmaEsOptimizer::update
// a comes before b: ascending fitness, a NaN after everything else, ties by the lower index
CPQ_HD inline bool learnBefore(const double* fitness, int a, int b)
{
    const double fa = fitness[a], fb = fitness[b];
    const bool na = fa != fa, nb = fb != fb;
    if (na || nb) return na == nb ? a < b : nb;
    if (fa < fb) return true;
    if (fb < fa) return false;
    return a < b;
}

// insertion sort of 0 .. 17: a fixed sequence of comparisons for a given input, no library behind it
CPQ_HD inline void learnOrder(const double* fitness, int* order)
{
    for (int i = 0; i < kLearnPop; ++i) {
        int at = i;
        while (at > 0 && learnBefore(fitness, i, order[at - 1])) { order[at] = order[at - 1]; --at; }
        order[at] = i;
    }
}

CPQ_HD inline double learnRetention(double current, const cpq_learn_params& p) { return learnMin(p.cov_retention_target, current + p.cov_retention_step); }

CPQ_HD inline double learnNewMean(const double* candidates, const int* order, int dim)
{
    double m = 0.0;
    for (int e = 0; e < kLearnElite; ++e) m += candidates[order[e] * kLearnDim + dim];
    return m / (double)kLearnElite;
}

// the new covariance entry (row, column); oldMean, sigma and old are the values before the update, retention the one after
CPQ_HD inline double learnCovEntry(const double* candidates, const int* order, const double* oldMean, double sigma, double retention,
                                   double old, int row, int column)
{
    double eliteCov = 0.0;
    for (int e = 0; e < kLearnElite; ++e) {
        const double* c = candidates + order[e] * kLearnDim;
        const double yRow = (c[row] - oldMean[row]) / sigma;
        const double yColumn = (c[column] - oldMean[column]) / sigma;
        eliteCov += yRow * yColumn;
    }
    return learnSanitize((retention * old) + (((1.0 - retention) / (double)kLearnElite) * eliteCov));
}

// newMean: before sanitize
CPQ_HD inline double learnSigma(const double* candidates, const int* order, const double* newMean, const cpq_learn_params& p)
{
    double variance = 0.0;
    for (int e = 0; e < kLearnElite; ++e) {
        const double* c = candidates + order[e] * kLearnDim;
        for (int row = 0; row < kLearnDim; ++row) {
            const double deltaRow = c[row] - newMean[row];
            variance += deltaRow * deltaRow;
        }
    }
    return learnClamp(learnSqrt(variance / (double)(kLearnElite * kLearnDim)), p.sigma_min, p.sigma_max);
}

// evaluatePopulation's final pass (:716-729): the first strict minimum below DBL_MAX, else candidate 0 with DBL_MAX
CPQ_HD inline int learnBestCandidate(const double* fitness, double* score)
{
    int best = 0;
    double bestScore = DBL_MAX;
    for (int p = 0; p < kLearnPop; ++p)
        if (fitness[p] < bestScore) { bestScore = fitness[p]; best = p; }
    *score = bestScore;
    return best;
}

// the generation loop's bookkeeping (:975-986): true when the running best is replaced by candidate `best`
CPQ_HD inline bool learnReplacesBest(double candidateBest, double runningBest) { return candidateBest < runningBest && candidateBest < DBL_MAX; }

// mapped may be null (best_scored stays); order: 18 ints of work space, the sort on return; returns the generation's best score
inline double learnTell(cpq_learn_state& st, const cpq_learn_params& p, const double* candidates, const double* mapped, const double* fitness,
                        int* order)
{
    const double retention = learnRetention(st.cov_retention, p);
    learnOrder(fitness, order);
    double newMean[kLearnDim], cov[kLearnCov];
    for (int dim = 0; dim < kLearnDim; ++dim) newMean[dim] = learnNewMean(candidates, order, dim);
    for (int row = 0; row < kLearnDim; ++row)
        for (int column = row; column < kLearnDim; ++column) {
            const int i = learnCovIndex(row, column);
            cov[i] = learnCovEntry(candidates, order, st.mean, st.sigma, retention, st.cov_upper[i], row, column);
        }
    const double sigma = learnSigma(candidates, order, newMean, p);
    for (int i = 0; i < kLearnCov; ++i) st.cov_upper[i] = cov[i];
    for (int dim = 0; dim < kLearnDim; ++dim) st.mean[dim] = learnSanitize(newMean[dim]);
    st.sigma = sigma;
    st.cov_retention = retention;
    double score;
    const int best = learnBestCandidate(fitness, &score);
    if (learnReplacesBest(score, st.best_score)) {
        st.best_score = score;
        for (int dim = 0; dim < kLearnDim; ++dim) {
            st.best_raw[dim] = candidates[best * kLearnDim + dim];
            if (mapped) st.best_scored[dim] = mapped[best * kLearnDim + dim];
        }
    }
    st.generations += 1;
    return score;
}

// ---- host only
constexpr double kLearnSigma0 = 0.12;
inline cpq_learn_params learnDefaultParams(const double* levelWeights)
{
    cpq_learn_params p{ 0.03, 0.30, 0.92, 0.0, { 0.4, 0.3, 0.2, 0.1 } };
    if (levelWeights)
        for (int i = 0; i < 4; ++i) p.level_weights[i] = levelWeights[i];
    return p;
}

// initFromParcor, with the generator from the seed and the bookkeeping cleared
inline void learnInit(const double* parcor, uint64_t seed, const cpq_learn_params& p, cpq_learn_state& st)
{
    st = cpq_learn_state{};
    for (int i = 0; i < kLearnDim; ++i) {
        const double clamped = learnClamp(parcor[i], -0.995, 0.995);
        st.mean[i] = 0.5 * std::log((1.0 + clamped) / (1.0 - clamped));
    }
    st.sigma = kLearnSigma0;
    st.cov_retention = p.cov_retention_target;
    for (int r = 0; r < kLearnDim; ++r) st.cov_upper[learnCovIndex(r, r)] = 1.0;
    learnSeed(seed, st.rng);
    st.best_score = DBL_MAX;
}

// computePhase; 0: unknown mode
inline int learnPhase(int mode, double seconds)
{
    static const double first[6] = { 5.0, 10.0, 30.0, 60.0, 120.0, 30.0 };
    if (mode < 0 || mode > 5) return 0;
    return seconds < first[mode] ? 1 : (seconds < 2.0 * first[mode] ? 2 : 3);
}

// applyPhaseParams; false: unknown mode or phase
inline bool learnPhaseParams(int mode, int phase, cpq_learn_params& p, double& interval)
{
    static const double intervals[6][3] = { { 0.25, 0.5, 1.0 }, { 0.5, 1.0, 2.0 }, { 1.0, 2.0, 4.0 }, { 2.0, 4.0, 8.0 }, { 4.0, 8.0, 16.0 }, { 1.0, 2.0, 4.0 } };
    static const double targets[6][3] = { { 0.80, 0.85, 0.90 }, { 0.85, 0.90, 0.95 }, { 0.90, 0.95, 0.98 }, { 0.95, 0.98, 0.99 }, { 0.98, 0.99, 0.995 }, { 0.90, 0.95, 0.98 } };
    static const double steps[6] = { 0.02, 0.01, 0.005, 0.002, 0.001, 0.005 };
    static const double weights[3][4] = { { 0.1, 0.2, 0.3, 0.4 }, { 0.25, 0.25, 0.25, 0.25 }, { 0.5, 0.3, 0.1, 0.1 } };
    if (mode < 0 || mode > 5 || phase < 1 || phase > 3) return false;
    p = learnDefaultParams(weights[phase - 1]);
    p.cov_retention_target = targets[mode][phase - 1];
    p.cov_retention_step = steps[mode];
    interval = intervals[mode][phase - 1];
    return true;
}

inline bool learnParamsValid(const cpq_learn_params& p)
{
    const double v[4] = { p.sigma_min, p.sigma_max, p.cov_retention_target, p.cov_retention_step };
    for (double x : v)
        if (!(learnAbs(x) <= DBL_MAX)) return false;
    for (double w : p.level_weights)
        if (!(w >= 0.0) || !(w <= DBL_MAX)) return false;
    return p.sigma_min > 0.0 && p.sigma_min <= p.sigma_max && p.cov_retention_target >= 0.0 && p.cov_retention_target <= 1.0 && p.cov_retention_step >= 0.0;
}

inline bool learnStateValid(const cpq_learn_state& s)
{
    for (double x : s.mean)
        if (!(learnAbs(x) <= DBL_MAX)) return false;
    for (double x : s.cov_upper)
        if (!(learnAbs(x) <= DBL_MAX)) return false;
    if (!(learnAbs(s.sigma) <= DBL_MAX) || !(learnAbs(s.cov_retention) <= DBL_MAX)) return false;
    if ((s.rng[0] | s.rng[1] | s.rng[2] | s.rng[3]) == 0) return false;
    return s.generations >= 0 && s.rejected_pairs >= 0;
}

// the reference's published set: tanh of toParcor(best_raw)
inline void learnPublished(const double* bestRaw, double* k)
{
    for (int i = 0; i < kLearnDim; ++i) k[i] = std::tanh(learnSanitize(std::tanh(bestRaw[i])));
}

}  // namespace cpq
