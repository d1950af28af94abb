// score_kernels.hip -- the shaper scorer on gfx950: NoiseShaperLearner::evaluateCandidateMapped (src/NoiseShaperLearner.cpp:1289-1375)
// and precomputeMaskingThresholds (:1377-1398) with MklFftEvaluator::evaluate / computeMaskingThreshold
// (src/MklFftEvaluator.h:244-405) for many learners and candidates in one call.
//
// k_score_lattice: a lane is one chain -- (learner, candidate, segment, channel) -- of 4096 dependent steps of dLatticeSample
// (lattice_device.hpp, the dither stage's own), so the only parallelism is across chains: one wave per workgroup, one chain per
// lane, ceil(chains / 64) workgroups, which spreads a generation of one learner (576 chains) over 9 CUs and puts no second
// chain into any lane.  Chains name their rows through a table, so a learner's segments are stored once and read by every
// candidate.  The rows go through an LDS tile as in k_dither_lattice: the wave reads 64 samples of each of its rows with lane =
// sample (one 512-byte line per instruction), each lane walks its own row of the tile in place (pitch 65 doubles: no bank
// conflict), and the tile is stored the way it came -- as the error yq - x * headroom, x * headroom being the very product the
// shaper was given.  The file is built with -ffp-contract=off; the feedback sum's four fused terms are written as fma.
//
// k_score_spectrum: a workgroup of 256 threads is one evaluation.  The two rows are transformed one after the other, each as a
// 2048-point complex radix-2 transform of its even / odd samples in 32 KiB of LDS followed by the real-input split; only squared
// magnitudes leave it (no scaling; the sign convention is immaterial).  |L|^2 waits in a second array of 2049 doubles, which
// then holds 0.5 (|L|^2 + |R|^2); with the transform done its 32 KiB hold the per-bin dB values and the two flag arrays of
// evaluate().  52 KiB of LDS in all: three workgroups per CU.  Sums over bins are trees (wave shuffles, then the four waves in
// order); everything evaluate() decides -- the > 6 localAvg peak test, the 7 dB tonal test over neighborRangeBins, the 0.5-Bark
// absorb radius, consumed, the caps of 128 maskers, the 8-Bark spread cut -- is the reference's comparison on the reference's
// quantity, and everything it sums per masker (a tonal masker's <= 17 bins, a bin's <= 128 contributions) is summed in its order.
#include "kernels.hpp"
#include "lattice_device.hpp"

#include <cfloat>

namespace cpq {
namespace {

constexpr int kLatStep = 64;                    // samples of a row per tile
constexpr int kLatPitch = kLatStep + 1;

// grid: ceil(nChains / 64) workgroups of one wave
__global__ void __launch_bounds__(64)
k_score_lattice(const double* __restrict__ seg, double* __restrict__ err, const ScoreChain* __restrict__ chains, int nChains,
                const double* __restrict__ coef, const unsigned long long* __restrict__ rng, DitherParams p)
{
    __shared__ double tile[64 * kLatPitch];
    __shared__ int srcRow[64], dstRow[64];
    const int lane = threadIdx.x;
    const int row0 = blockIdx.x * 64;
    const int rows = min(64, nChains - row0);                       // >= 1
    const bool live = lane < rows;
    ScoreChain ch{ 0, 0, 0, 0 };
    if (live) ch = chains[row0 + lane];
    srcRow[lane] = ch.src;
    dstRow[lane] = ch.dst;
    double st[kLatticeOrder], c[kLatticeOrder];
    unsigned long long s[4];
#pragma unroll
    for (int k = 0; k < kLatticeOrder; ++k) {
        st[k] = 0.0;                                                // reset(): every segment starts from cleared states
        c[k] = live ? coef[(size_t)ch.coef * kLatticeOrder + k] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = live ? rng[(size_t)ch.rng * 4 + k] : 1ull;
    __syncthreads();
    double* mine = tile + lane * kLatPitch;
    for (int t0 = 0; t0 < kScoreLen; t0 += kLatStep) {
#pragma unroll 8
        for (int r = 0; r < rows; ++r) tile[r * kLatPitch + lane] = seg[(size_t)srcRow[r] * kScoreLen + t0 + lane];
        __syncthreads();
        if (live) {
            for (int t = 0; t < kLatStep; ++t) {
                const double xh = mine[t] * p.headroom;
                const double yq = dLatticeSample(xh, st, c, s, p);
                mine[t] = yq - xh;
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int r = 0; r < rows; ++r) err[(size_t)dstRow[r] * kScoreLen + t0 + lane] = tile[r * kLatPitch + lane];
        __syncthreads();                                            // the tile is free again
    }
}

// grid: 2 nSegments workgroups (a row each)
__global__ void __launch_bounds__(256)
k_score_level(const double* __restrict__ recent, int64_t stride, const int* __restrict__ start, const double* __restrict__ gain,
              double* __restrict__ seg)
{
    const int row = blockIdx.x, sg = row >> 1;
    const double* src = recent + (size_t)(row & 1) * stride + start[sg];
    const double g = gain[sg];
    for (int i = threadIdx.x; i < kScoreLen; i += 256) seg[(size_t)row * kScoreLen + i] = src[i] * g;
}

constexpr int kThreads = 256;
constexpr int kHalf = kScoreLen / 2;            // 2048: points of the complex transform
constexpr int kMaxMaskers = 128;
constexpr double kMinPower = 1.0e-24;
constexpr double kDbPerLn = 10.0 * 0.43429448190325182765;          // powerToDb's kLog10Factor

__device__ __forceinline__ double powerToDb(double power) { return log(fmax(power, kMinPower)) * kDbPerLn; }

// the block's sum of v, the same in every thread: lanes by shuffles, then the four waves in order
__device__ __forceinline__ double blockSum(double v, double* scratch)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                                // scratch is free
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

__device__ __forceinline__ double blockMax(double v, double* scratch)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(scratch[0], scratch[1]), fmax(scratch[2], scratch[3]));
}

// |X[k]|^2, k <= 2048, of the 4096 real samples at x: into mag (first = true) or averaged with what mag holds
__device__ void rowSpectrum(const double* __restrict__ x, double2* z, double* mag, const double2* __restrict__ tw, bool first)
{
    const int tid = threadIdx.x;
    const double2* x2 = reinterpret_cast<const double2*>(x);
    for (int n = tid; n < kHalf; n += kThreads) z[__brev((unsigned)n) >> 21] = x2[n];      // 11-bit reversal
    __syncthreads();
    for (int s = 1; s <= 11; ++s) {
        const int half = 1 << (s - 1);
        for (int b = tid; b < kHalf / 2; b += kThreads) {
            const int j = b & (half - 1);
            const int i0 = ((b >> (s - 1)) << s) + j, i1 = i0 + half;
            const double2 w = tw[j << (12 - s)];
            const double2 a = z[i0], q = z[i1];
            const double tr = w.x * q.x - w.y * q.y, ti = w.x * q.y + w.y * q.x;
            z[i0] = make_double2(a.x + tr, a.y + ti);
            z[i1] = make_double2(a.x - tr, a.y - ti);
        }
        __syncthreads();
    }
    for (int k = tid; k <= kHalf; k += kThreads) {
        const double2 a = z[k & (kHalf - 1)], m = z[(kHalf - k) & (kHalf - 1)];
        const double er = 0.5 * (a.x + m.x), ei = 0.5 * (a.y - m.y);               // even samples' spectrum
        const double orr = 0.5 * (a.y + m.y), oi = -0.5 * (a.x - m.x);             // odd samples' spectrum
        double wr = -1.0, wi = 0.0;
        if (k < kHalf) { const double2 w = tw[k]; wr = w.x; wi = w.y; }
        const double xr = er + (wr * orr - wi * oi), xi = ei + (wr * oi + wi * orr);
        const double m2 = xr * xr + xi * xi;
        mag[k] = first ? m2 : 0.5 * (mag[k] + m2);
    }
    __syncthreads();
}

__device__ __forceinline__ double spreadDb(double deltaBark, int type, const ScoreDeviceTables& t)
{
    const double idx = (deltaBark / 0.01) + 800.0;
    const int i = (int)round(idx);
    if (i < 0 || i >= kScoreSpreadBins) return 0.0;
    return type == 0 ? t.spreadTonal[i] : t.spreadNoise[i];
}

// the tonal masker of peak bin i: false when its energy does not pass kMinPower.  kMark: marks the bins it absorbs (detection);
// without it consumed is not touched (compaction, while the other waves already read consumed for the noise maskers)
template <bool kMark>
__device__ __forceinline__ bool tonalMasker(int i, const double* raw, const ScoreDeviceTables& t, unsigned char* consumed, double& energy,
                                            double& bark)
{
    const double centerBark = t.bark[i];
    double sumEnergy = 0.0, sumBarkWeighted = 0.0;
    const int start = max(0, i - 8), end = min(kScoreBins - 1, i + 8);
    for (int j = start; j <= end; ++j) {
        if (fabs(t.bark[j] - centerBark) > 0.5) continue;
        const double e = fmax(kMinPower, raw[j]) * t.width[j];
        sumEnergy += e;
        sumBarkWeighted += t.bark[j] * e;
        if (kMark) consumed[j] = 1;
    }
    energy = sumEnergy;
    bark = sumBarkWeighted / sumEnergy;
    return !(sumEnergy <= kMinPower);
}

// grid: nEvals workgroups
__global__ void __launch_bounds__(kThreads)
k_score_spectrum(const double* __restrict__ rows, double* __restrict__ thr, const ScoreEval* __restrict__ evals, ScoreDeviceTables t,
                 cpq_score_parts* __restrict__ parts, double* __restrict__ blended, int thresholdsOnly)
{
    __shared__ double2 z[kHalf];
    __shared__ double raw[kScoreBins + 1];
    __shared__ double scratch[4];
    __shared__ double mLevel[kMaxMaskers], mBark[kMaxMaskers];
    __shared__ int mType[kMaxMaskers];
    __shared__ double bandBark[kScoreBands], bandLevel[kScoreBands];
    __shared__ int bandValid[kScoreBands], peakCount[64], nMaskers;
    const int tid = threadIdx.x;
    const ScoreEval ev = evals[blockIdx.x];
    const double* left = rows + (size_t)ev.row * 2 * kScoreLen;
    const double* right = left + kScoreLen;
    rowSpectrum(left, z, raw, t.tw, true);
    rowSpectrum(right, z, raw, t.tw, false);
    double* segThr = thr + (size_t)ev.thr * kScoreBins;
    if (thresholdsOnly) {                                           // computeMaskingThreshold(0.5 (|L|^2 + |R|^2), k binWidth)
        for (int k = tid; k < kScoreBins; k += kThreads) segThr[k] = fmax(t.athPow[k], fmax(raw[k], kMinPower) * t.thrSpread[k]);
        return;
    }
    // the transform's LDS again: dB of every bin, consumed, valid peaks
    double* pdb = reinterpret_cast<double*>(z);
    unsigned char* consumed = reinterpret_cast<unsigned char*>(pdb + kScoreBins + 1);
    unsigned char* isPeak = consumed + kScoreBins + 7;
    static_assert(sizeof(double) * (kScoreBins + 1) + 2 * (kScoreBins + 7) <= sizeof(double2) * kHalf, "the per-bin arrays fit the transform's LDS");

    double sumSq = 0.0;
    for (int i = tid; i < kScoreLen; i += kThreads) sumSq += 0.5 * (left[i] * left[i] + right[i] * right[i]);
    sumSq = blockSum(sumSq, scratch);
    const double timeRms = sqrt(sumSq / kScoreLen);

    double total = 0.0, flatLog = 0.0, flatPow = 0.0, high = 0.0, ultra = 0.0, peak = 0.0;
    for (int k = tid; k < kScoreBins; k += kThreads) {
        const double avg = fmax(kMinPower, raw[k]);
        const double safe = avg + kMinPower;
        pdb[k] = powerToDb(avg);
        consumed[k] = 0;
        isPeak[k] = 0;
        total += avg;
        if (k >= t.flatStart && k <= t.flatEnd) { flatLog += log(safe); flatPow += safe; }
        if (k >= t.highStart) high += avg;
        if (k >= t.ultraStart) ultra += avg;
        if (k > 0 && k < kScoreBins - 1) {
            const double localAvg = 0.5 * (raw[k - 1] + raw[k + 1]) + kMinPower;
            if (avg > 6.0 * localAvg) peak = fmax(peak, avg);
        }
    }
    total = blockSum(total, scratch);
    flatLog = blockSum(flatLog, scratch);
    flatPow = blockSum(flatPow, scratch);
    high = blockSum(high, scratch);
    ultra = blockSum(ultra, scratch);
    peak = blockMax(peak, scratch);                                 // (the barriers inside also publish pdb, consumed, isPeak)

    // detectTonalMaskersFixed: a peak stands 7 dB above every neighbour within neighborRangeBins
    for (int i = 3 + tid; i < kScoreBins - 3; i += kThreads) {
        const int range = t.range[i];
        const double centerDb = pdb[i];
        bool is = true;
        for (int k = 1; k <= range && is; ++k) {
            if (i - k >= 0 && centerDb - pdb[i - k] < 7.0) is = false;
            else if (i + k < kScoreBins && centerDb - pdb[i + k] < 7.0) is = false;
        }
        if (!is) continue;
        double e, b;
        if (tonalMasker<true>(i, raw, t, consumed, e, b)) isPeak[i] = 1;
    }
    __syncthreads();
    // the maskers in bin order, the first 128: wave 0 counts 33 bins a lane, then every lane writes its own
    constexpr int kPerLane = (kScoreBins + 63) / 64;
    if (tid < 64) {
        int n = 0;
        for (int i = tid * kPerLane; i < min(kScoreBins, (tid + 1) * kPerLane); ++i) n += isPeak[i];
        peakCount[tid] = n;
    }
    __syncthreads();
    if (tid < 64) {
        int at = 0;
        for (int u = 0; u < tid; ++u) at += peakCount[u];
        for (int i = tid * kPerLane; i < min(kScoreBins, (tid + 1) * kPerLane); ++i) {
            if (!isPeak[i]) continue;
            if (at < kMaxMaskers) {
                double e, b;                                        // at most 128 peaks: summed again, not kept per bin
                tonalMasker<false>(i, raw, t, consumed, e, b);
                mLevel[at] = powerToDb(e);
                mBark[at] = b;
                mType[at] = 0;
            }
            ++at;
        }
        if (tid == 63) nMaskers = min(at, kMaxMaskers);
    }
    // buildNoiseMaskersFixed: a wave per Bark band, over the bins no tonal masker absorbed
    for (int band = tid >> 6; band < kScoreBands; band += kThreads / 64) {
        double sumEnergy = 0.0, sumBarkWeighted = 0.0, logSum = 0.0, linearSum = 0.0;
        int count = 0;
        for (int i = t.bandStart[band] + (tid & 63); i < t.bandStart[band + 1]; i += 64) {
            if (consumed[i]) continue;
            const double pw = fmax(kMinPower, raw[i]);
            const double e = pw * t.width[i];
            sumEnergy += e;
            sumBarkWeighted += t.bark[i] * e;
            const double pf = fmax(pw, 1.0e-15);
            logSum += log(pf);
            linearSum += pf;
            ++count;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sumEnergy += __shfl_xor(sumEnergy, o);
            sumBarkWeighted += __shfl_xor(sumBarkWeighted, o);
            logSum += __shfl_xor(logSum, o);
            linearSum += __shfl_xor(linearSum, o);
            count += __shfl_xor(count, o);
        }
        if ((tid & 63) == 0) {
            const bool valid = !(count <= 0 || sumEnergy <= kMinPower);
            bandValid[band] = valid;
            if (valid) {
                const double geometric = exp(logSum / (double)count);
                const double arithmetic = linearSum / (double)count;
                const double sfm = geometric / fmax(arithmetic, 1.0e-15);
                double tonality = -0.299 + (-0.43 * log(fmax(sfm, 1.0e-12)) * 0.43429448190325182765);
                tonality = tonality < 0.0 ? 0.0 : (1.0 < tonality ? 1.0 : tonality);
                bandBark[band] = sumBarkWeighted / sumEnergy;
                bandLevel[band] = powerToDb(sumEnergy) + (-5.0 * (1.0 - tonality));        // the noise masker's correction
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        int at = nMaskers;
        for (int band = 0; band < kScoreBands; ++band) {
            if (!bandValid[band] || at >= kMaxMaskers) continue;    // MaskerBuffer::push drops what does not fit
            mLevel[at] = bandLevel[band];
            mBark[at] = bandBark[band];
            mType[at] = 1;
            ++at;
        }
        nMaskers = at;
    }
    __syncthreads();

    // computeMaskingEnergyStable, the thresholds and the JND-weighted excess, per bin
    const int nm = nMaskers;
    constexpr double kLogScale = 0.2302585093;
    double psycho = 0.0;
    for (int i = tid; i < kScoreBins; i += kThreads) {
        const double barkI = t.bark[i];
        double maxDb = -__builtin_huge_val();
        int n = 0;
        for (int j = 0; j < nm; ++j) {
            const double deltaBark = barkI - mBark[j];
            if (fabs(deltaBark) > 8.0) continue;
            const double totalDb = mLevel[j] + spreadDb(deltaBark, mType[j], t);
            ++n;
            if (totalDb > maxDb) maxDb = totalDb;
        }
        double maskingEnergy = t.athPow[i];
        if (n > 0 && fabs(maxDb) < __builtin_huge_val()) {
            double sum = 0.0;
            for (int j = 0; j < nm; ++j) {
                const double deltaBark = barkI - mBark[j];
                if (fabs(deltaBark) > 8.0) continue;
                const double totalDb = mLevel[j] + spreadDb(deltaBark, mType[j], t);
                sum += exp((totalDb - maxDb) * kLogScale);
            }
            maskingEnergy = fmax(exp(maxDb * kLogScale) * sum, t.athPow[i]);
        }
        double threshold = fmax(powerToDb(maskingEnergy), t.athDb[i]);
        threshold = fmax(threshold, powerToDb(fmax(segThr[i], kMinPower)));
        const double deltaDb = pdb[i] - threshold;
        const double zz = 2.0 * deltaDb;                            // softplus
        const double soft = zz > 50.0 ? deltaDb : zz < -50.0 ? exp(zz) / 2.0 : log1p(exp(zz)) / 2.0;
        const double effectiveDb = 20.0 * tanh(soft / 20.0);        // smoothCap
        const double effectivePower = fmax(0.0, pow(10.0, effectiveDb / 10.0) - 1.0);
        psycho += t.weight[i] * effectivePower;
    }
    psycho = blockSum(psycho, scratch);
    if (tid != 0) return;

    cpq_score_parts r;
    r.noise_power = t.weightSum > kMinPower ? (psycho / t.weightSum) * (double)kScoreLen : 0.0;
    const int flatBins = min(t.flatEnd, kScoreBins - 1) - t.flatStart + 1;
    r.spectral_flatness_penalty = 0.0;
    if (flatBins > 0) {
        const double arithmeticMean = flatPow / (double)flatBins;
        const double geometricMean = exp(flatLog / (double)flatBins);
        const double f = geometricMean / fmax(arithmeticMean, kMinPower);
        r.spectral_flatness_penalty = 1.0 - (f < 0.0 ? 0.0 : (1.0 < f ? 1.0 : f));
    }
    const double observedShare = ultra / fmax(high + kMinPower, kMinPower);
    const double excessShare = fmax(0.0, observedShare - t.ultraShare);
    r.hf_penalty = excessShare / fmax(1.0 - t.ultraShare, kMinPower);
    r.time_domain_rms = timeRms;
    const double tonalRatio = peak / (total + kMinPower);
    const double tonalPenalty = fmax(0.0, tonalRatio - 0.05) * 10.0;
    r.composite_score = r.noise_power * (1.0 + (t.flatWeight * r.spectral_flatness_penalty) + (t.hfWeight * r.hf_penalty) + tonalPenalty);
    parts[ev.slot] = r;
    const double timeScore = timeRms * 1000.0;
    const double freqScore = sqrt(r.composite_score / (double)kScoreLen) * 1000.0;
    blended[ev.slot] = (ev.alpha * freqScore + (1.0 - ev.alpha) * timeScore);
}

// grid: ceil(pairs / 64); a thread is one (learner, candidate)
__global__ void __launch_bounds__(64)
k_score_reduce(const double* __restrict__ blended, const int* __restrict__ counts, const int* __restrict__ state, int nPairs, int nCand,
               double w0, double w1, double w2, double w3, double* __restrict__ scores)
{
    const int pair = blockIdx.x * 64 + threadIdx.x;
    if (pair >= nPairs) return;
    if (state[pair] == 1) { scores[pair] = CPQ_SCORE_UNSTABLE; return; }
    const int* cnt = counts + (size_t)(pair / nCand) * kScoreLevels;
    const double w[kScoreLevels] = { w0, w1, w2, w3 };
    double totalWeightedScore = 0.0, totalWeight = 0.0;
    int s = 0;
#pragma unroll
    for (int i = 0; i < kScoreLevels; ++i) {
        const int count = cnt[i];
        if (count == 0) continue;
        double levelScoreSum = 0.0;
        for (int j = 0; j < count; ++j) levelScoreSum += blended[(size_t)pair * kScoreMaxSegments + s++];
        const double levelAverageScore = levelScoreSum / count;
        totalWeightedScore += levelAverageScore * w[i];
        totalWeight += w[i];
    }
    scores[pair] = totalWeight <= 0.0 ? DBL_MAX : totalWeightedScore / totalWeight;
}

}  // namespace

void launch_score_lattice(hipStream_t stream, const double* seg, double* err, const ScoreChain* chains, int nChains, const double* coef,
                          const unsigned long long* rng, const DitherParams& p)
{
    if (nChains <= 0) return;
    hipLaunchKernelGGL(k_score_lattice, dim3((unsigned)((nChains + 63) / 64)), dim3(64), 0, stream, seg, err, chains, nChains, coef, rng, p);
}

void launch_score_level(hipStream_t stream, const double* recent, int64_t stride, const int* start, const double* gain, double* seg,
                        int nSegments)
{
    if (nSegments <= 0) return;
    hipLaunchKernelGGL(k_score_level, dim3((unsigned)(2 * nSegments)), dim3(256), 0, stream, recent, stride, start, gain, seg);
}

void launch_score_spectrum(hipStream_t stream, const double* rows, double* thr, const ScoreEval* evals, int nEvals,
                           const ScoreDeviceTables& t, cpq_score_parts* parts, double* blended, bool thresholdsOnly)
{
    if (nEvals <= 0) return;
    hipLaunchKernelGGL(k_score_spectrum, dim3((unsigned)nEvals), dim3(kThreads), 0, stream, rows, thr, evals, t, parts, blended,
                       thresholdsOnly ? 1 : 0);
}

void launch_score_reduce(hipStream_t stream, const double* blended, const int* counts, const int* state, int nLearners, int nCand,
                         const double* levelWeights, double* scores)
{
    const int nPairs = nLearners * nCand;
    if (nPairs <= 0) return;
    hipLaunchKernelGGL(k_score_reduce, dim3((unsigned)((nPairs + 63) / 64)), dim3(64), 0, stream, blended, counts, state, nPairs, nCand,
                       levelWeights[0], levelWeights[1], levelWeights[2], levelWeights[3], scores);
}

}  // namespace cpq
