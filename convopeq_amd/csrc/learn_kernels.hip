// learn_kernels.hip -- the two kernels of cpq_learner on gfx950: CmaEsOptimizer::sample with evaluatePopulation's mapping
// (k_learn_ask) and CmaEsOptimizer::update with the generation loop's best tracking (k_learn_tell).  Every operation on a value
// is a function of learn_plan.hpp, the same text the host entries run; this file only deals the elements to lanes.
//
// A learner is a few thousand flops with long dependent chains (81 polar pairs drawn one after the other from one generator,
// a 9 x 9 Cholesky factor, an insertion sort of 18), so a generation is bound by latency and not by throughput: a workgroup is
// one learner, and what is serial runs in one lane while the rest waits.  Everything indexed at run time -- z, the factor, the
// candidates, the sort -- lives in LDS (under 5 KiB), never in private arrays, so nothing goes to scratch.
//   k_learn_ask   two waves: lane 0 of wave 0 draws the 162 variates while lane 0 of wave 1 factors the covariance (two serial
//                 chains side by side on two SIMDs); then thread i < 162 builds candidate entry i, maps it and stores the clamped
//                 coefficient straight into the scorer's coef buffer; thread p < 18 sets the scorer's state flag of candidate p.
//   k_learn_tell  one wave: lane 0 sorts; lanes 0-8 the elite mean; lanes 0-44 one covariance entry each; lane 0 sigma, the best
//                 tracking and the history.  A lane overwrites only the state entries it alone read.
// The file is built with -ffp-contract=off like every other.
#include "kernels.hpp"
#include "learn_plan.hpp"

namespace cpq {
namespace {

constexpr int kAskThreads = 128;

// grid: nLearners workgroups
__global__ void __launch_bounds__(kAskThreads)
k_learn_ask(cpq_learn_state* __restrict__ states, const int* __restrict__ active, double margin, int stabilityCheck,
            double* __restrict__ coef, int* __restrict__ flag, double* __restrict__ zOut, double* __restrict__ candOut,
            double* __restrict__ mappedOut)
{
    __shared__ double z[kLearnVars], map[kLearnVars], lower[kLearnDim * kLearnDim], cov[kLearnCov], mean[kLearnDim];
    const int l = blockIdx.x, tid = threadIdx.x;
    if (!active[l]) return;                                         // the whole workgroup
    cpq_learn_state* st = states + l;
    if (tid < kLearnCov) cov[tid] = st->cov_upper[tid];
    if (tid < kLearnDim) mean[tid] = st->mean[tid];
    if (tid < kLearnDim * kLearnDim) lower[tid] = 0.0;
    const double sigma = st->sigma;
    __syncthreads();
    if (tid == 0) {
        uint64_t rng[4] = { st->rng[0], st->rng[1], st->rng[2], st->rng[3] };
        int rejected = st->rejected_pairs;
        learnNormals(rng, z, &rejected);
        st->rng[0] = rng[0];
        st->rng[1] = rng[1];
        st->rng[2] = rng[2];
        st->rng[3] = rng[3];
        st->rejected_pairs = rejected;
    } else if (tid == 64) {
        learnCholesky(cov, lower);
    }
    __syncthreads();
    const size_t base = (size_t)l * kLearnVars;
    for (int i = tid; i < kLearnVars; i += kAskThreads) {
        const double c = learnCandidate(mean, sigma, lower, z, i / kLearnDim, i % kLearnDim);
        const double m = learnMap(c, margin);
        map[i] = m;
        zOut[base + i] = z[i];
        candOut[base + i] = c;
        mappedOut[base + i] = m;
        coef[base + i] = learnShaperCoeff(m);                       // pair l * 18 + p of a score call of 18 candidates
    }
    __syncthreads();
    if (tid < kLearnPop) {
        bool refused = false;
        for (int d = 0; d < kLearnDim; ++d) refused = refused || learnRefused(map[tid * kLearnDim + d]);
        flag[(size_t)l * kLearnPop + tid] = (stabilityCheck && refused) ? 1 : 0;
    }
}

// grid: nLearners workgroups of one wave.  history: [nLearners][histStride], this generation at column g
__global__ void __launch_bounds__(64)
k_learn_tell(cpq_learn_state* __restrict__ states, const int* __restrict__ active, cpq_learn_params p, const double* __restrict__ cand,
             const double* __restrict__ mapped, const double* __restrict__ scores, int* __restrict__ orderOut,
             double* __restrict__ history, int histStride, int g)
{
    __shared__ double c[kLearnVars], fit[kLearnPop], oldMean[kLearnDim], newMean[kLearnDim];
    __shared__ int order[kLearnPop];
    const int l = blockIdx.x, lane = threadIdx.x;
    if (!active[l]) return;
    cpq_learn_state* st = states + l;
    const size_t base = (size_t)l * kLearnVars;
    for (int i = lane; i < kLearnVars; i += 64) c[i] = cand[base + i];
    if (lane < kLearnPop) fit[lane] = scores[(size_t)l * kLearnPop + lane];
    if (lane < kLearnDim) oldMean[lane] = st->mean[lane];
    const double sigma = st->sigma;
    const double retention = learnRetention(st->cov_retention, p);
    const double oldCov = lane < kLearnCov ? st->cov_upper[lane] : 0.0;
    __syncthreads();
    if (lane == 0) learnOrder(fit, order);
    __syncthreads();
    if (lane < kLearnDim) newMean[lane] = learnNewMean(c, order, lane);
    double covNew = 0.0;
    if (lane < kLearnCov) {
        int row = 0, column = lane;                                 // entry `lane` of the upper triangle by rows
        while (column >= kLearnDim - row) { column -= kLearnDim - row; ++row; }
        column += row;
        covNew = learnCovEntry(c, order, oldMean, sigma, retention, oldCov, row, column);
    }
    __syncthreads();
    if (lane < kLearnCov) st->cov_upper[lane] = covNew;
    if (lane < kLearnDim) st->mean[lane] = learnSanitize(newMean[lane]);
    if (lane < kLearnPop) orderOut[(size_t)l * kLearnPop + lane] = order[lane];
    if (lane != 0) return;
    st->sigma = learnSigma(c, order, newMean, p);
    st->cov_retention = retention;
    double score;
    const int best = learnBestCandidate(fit, &score);
    if (learnReplacesBest(score, st->best_score)) {
        st->best_score = score;
        for (int d = 0; d < kLearnDim; ++d) {
            st->best_raw[d] = c[best * kLearnDim + d];
            st->best_scored[d] = mapped[base + best * kLearnDim + d];
        }
    }
    st->generations += 1;
    history[(size_t)l * histStride + g] = score;
}

}  // namespace

void launch_learn_ask(hipStream_t stream, cpq_learn_state* states, const int* active, int nLearners, double margin, bool stabilityCheck,
                      double* coef, int* flag, double* z, double* candidates, double* mapped)
{
    if (nLearners <= 0) return;
    hipLaunchKernelGGL(k_learn_ask, dim3((unsigned)nLearners), dim3(kAskThreads), 0, stream, states, active, margin, stabilityCheck ? 1 : 0,
                       coef, flag, z, candidates, mapped);
}

void launch_learn_tell(hipStream_t stream, cpq_learn_state* states, const int* active, int nLearners, const cpq_learn_params& p,
                       const double* candidates, const double* mapped, const double* scores, int* order, double* history, int histStride,
                       int g)
{
    if (nLearners <= 0) return;
    hipLaunchKernelGGL(k_learn_tell, dim3((unsigned)nLearners), dim3(64), 0, stream, states, active, p, candidates, mapped, scores, order,
                       history, histStride, g);
}

}  // namespace cpq
