// learn_plan_check.cpp -- csrc/learn_plan.hpp as a program of its own under ASan and UBSan: k_learn_ask and k_learn_tell of
// learn_kernels.hip restated as host loops over workgroups, phases and lanes that call the header's functions, on heap blocks
// of exactly the sizes engine_learn.cpp and engine_score.cpp allocate (a workgroup's LDS arrays are heap blocks of their declared
// sizes).  What is checked: every index the kernels form, that the lane-dealt tell equals the header's own learnTell and the
// lane-dealt ask its learnAsk bit for bit, the order under ties and NaN, and the bounded polar loop.
#include "learn_plan.hpp"

#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

using namespace cpq;

static int failed = 0, checks = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        ++checks;                                                                 \
        if (!(cond)) { ++failed; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

template <typename T> std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n]()); }
static bool sameBits(const double* a, const double* b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

struct Device {
    int L;
    std::unique_ptr<cpq_learn_state[]> states;
    std::unique_ptr<int[]> active, flag, order;
    std::unique_ptr<double[]> coef, z, cand, mapped, scores, history;
    int histStride;
    Device(int l, int g) : L(l), states(block<cpq_learn_state>(l)), active(block<int>(l)), flag(block<int>((size_t)l * kLearnPop)),
                           order(block<int>((size_t)l * kLearnPop)), coef(block<double>((size_t)l * kLearnVars)), z(block<double>((size_t)l * kLearnVars)),
                           cand(block<double>((size_t)l * kLearnVars)), mapped(block<double>((size_t)l * kLearnVars)),
                           scores(block<double>((size_t)l * kLearnPop)), history(block<double>((size_t)l * g)), histStride(g) {}
};

// k_learn_ask, workgroup l of 128 threads: the phases between its barriers, one after the other
static void askKernel(Device& d, int l, double margin, int stabilityCheck)
{
    if (!d.active[l]) return;
    auto z = block<double>(kLearnVars), map = block<double>(kLearnVars), lower = block<double>(kLearnDim * kLearnDim), cov = block<double>(kLearnCov),
         mean = block<double>(kLearnDim);
    cpq_learn_state* st = d.states.get() + l;
    for (int tid = 0; tid < 128; ++tid) {
        if (tid < kLearnCov) cov[tid] = st->cov_upper[tid];
        if (tid < kLearnDim) mean[tid] = st->mean[tid];
        if (tid < kLearnDim * kLearnDim) lower[tid] = 0.0;
    }
    const double sigma = st->sigma;
    {
        uint64_t rng[4] = { st->rng[0], st->rng[1], st->rng[2], st->rng[3] };
        int rejected = st->rejected_pairs;
        learnNormals(rng, z.get(), &rejected);
        for (int i = 0; i < 4; ++i) st->rng[i] = rng[i];
        st->rejected_pairs = rejected;
        learnCholesky(cov.get(), lower.get());
    }
    const size_t base = (size_t)l * kLearnVars;
    for (int tid = 0; tid < 128; ++tid)
        for (int i = tid; i < kLearnVars; i += 128) {
            const double c = learnCandidate(mean.get(), sigma, lower.get(), z.get(), i / kLearnDim, i % kLearnDim);
            const double m = learnMap(c, margin);
            map[i] = m;
            d.z[base + i] = z[i];
            d.cand[base + i] = c;
            d.mapped[base + i] = m;
            d.coef[base + i] = learnShaperCoeff(m);
        }
    for (int tid = 0; tid < kLearnPop; ++tid) {
        bool refused = false;
        for (int k = 0; k < kLearnDim; ++k) refused = refused || learnRefused(map[tid * kLearnDim + k]);
        d.flag[(size_t)l * kLearnPop + tid] = (stabilityCheck && refused) ? 1 : 0;
    }
}

// k_learn_tell, workgroup l of one wave
static void tellKernel(Device& d, int l, const cpq_learn_params& p, int g)
{
    if (!d.active[l]) return;
    auto c = block<double>(kLearnVars), fit = block<double>(kLearnPop), oldMean = block<double>(kLearnDim), newMean = block<double>(kLearnDim);
    auto order = block<int>(kLearnPop);
    cpq_learn_state* st = d.states.get() + l;
    const size_t base = (size_t)l * kLearnVars;
    double oldCov[64] = {}, covNew[64] = {};
    for (int lane = 0; lane < 64; ++lane) {
        for (int i = lane; i < kLearnVars; i += 64) c[i] = d.cand[base + i];
        if (lane < kLearnPop) fit[lane] = d.scores[(size_t)l * kLearnPop + lane];
        if (lane < kLearnDim) oldMean[lane] = st->mean[lane];
        oldCov[lane] = lane < kLearnCov ? st->cov_upper[lane] : 0.0;
    }
    const double sigma = st->sigma;
    const double retention = learnRetention(st->cov_retention, p);
    learnOrder(fit.get(), order.get());
    int seen[kLearnCov] = {};
    for (int lane = 0; lane < 64; ++lane) {
        if (lane < kLearnDim) newMean[lane] = learnNewMean(c.get(), order.get(), lane);
        if (lane < kLearnCov) {
            int row = 0, column = lane;
            while (column >= kLearnDim - row) { column -= kLearnDim - row; ++row; }
            column += row;
            CHECK(row >= 0 && row <= column && column < kLearnDim && learnCovIndex(row, column) == lane, "lane %d -> (%d, %d)", lane, row, column);
            ++seen[learnCovIndex(column, row)];
            covNew[lane] = learnCovEntry(c.get(), order.get(), oldMean.get(), sigma, retention, oldCov[lane], row, column);
        }
    }
    for (int i = 0; i < kLearnCov; ++i) CHECK(seen[i] == 1, "covariance entry %d taken %d times", i, seen[i]);
    for (int lane = 0; lane < 64; ++lane) {
        if (lane < kLearnCov) st->cov_upper[lane] = covNew[lane];
        if (lane < kLearnDim) st->mean[lane] = learnSanitize(newMean[lane]);
        if (lane < kLearnPop) d.order[(size_t)l * kLearnPop + lane] = order[lane];
    }
    st->sigma = learnSigma(c.get(), order.get(), newMean.get(), p);
    st->cov_retention = retention;
    double score;
    const int best = learnBestCandidate(fit.get(), &score);
    CHECK(best >= 0 && best < kLearnPop, "best candidate %d", best);
    if (learnReplacesBest(score, st->best_score)) {
        st->best_score = score;
        for (int k = 0; k < kLearnDim; ++k) {
            st->best_raw[k] = c[best * kLearnDim + k];
            st->best_scored[k] = d.mapped[base + best * kLearnDim + k];
        }
    }
    st->generations += 1;
    d.history[(size_t)l * d.histStride + g] = score;
}

static void fitnessOf(int kind, int l, int g, const double* cand, double* f)
{
    for (int i = 0; i < kLearnPop; ++i) {
        double v = 0.0;
        for (int k = 0; k < kLearnDim; ++k) v += cand[i * kLearnDim + k] * cand[i * kLearnDim + k];
        f[i] = v;
    }
    if (kind == 1) for (int i = 0; i < kLearnPop; ++i) f[i] = (double)((i * 7 + l + g) % 4);         // ties
    if (kind == 2) { f[(l + g) % kLearnPop] = NAN; f[(l + 5) % kLearnPop] = NAN; f[(l + 9) % kLearnPop] = DBL_MAX; }
    if (kind == 3) for (int i = 0; i < kLearnPop; ++i) f[i] = i % 5 == 0 ? (double)i : (i % 2 ? NAN : DBL_MAX);     // four finite values
    if (kind == 4) for (int i = 0; i < kLearnPop; ++i) f[i] = NAN;
}

static void checkOrder(const double* f, const int* order)
{
    bool seen[kLearnPop] = {};
    for (int i = 0; i < kLearnPop; ++i) {
        CHECK(order[i] >= 0 && order[i] < kLearnPop && !seen[order[i]], "order[%d] = %d", i, order[i]);
        if (order[i] >= 0 && order[i] < kLearnPop) seen[order[i]] = true;
    }
    for (int i = 0; i + 1 < kLearnPop; ++i) {
        const double a = f[order[i]], b = f[order[i + 1]];
        const bool ok = (b != b && (a == a || order[i] < order[i + 1])) || (a == a && b == b && (a < b || (a == b && order[i] < order[i + 1])));
        CHECK(ok, "order at %d: %g (%d) before %g (%d)", i, a, order[i], b, order[i + 1]);
    }
}

static void runLearners(int L)
{
    const int G = 3;
    Device d(L, G);
    std::vector<cpq_learn_state> twin((size_t)L);
    const cpq_learn_params p = learnDefaultParams(nullptr);
    for (int l = 0; l < L; ++l) {
        double parcor[kLearnDim];
        for (int k = 0; k < kLearnDim; ++k) parcor[k] = 0.9 * std::sin(1.0 + l + 2.0 * k);
        learnInit(parcor, 1000u + (uint64_t)l, p, d.states[l]);
        if (l % 7 == 3) { d.states[l].cov_upper[learnCovIndex(2, 2)] = 0.0; d.states[l].cov_upper[learnCovIndex(5, 5)] = -1.0; }   // the floors
        if (l % 11 == 5) d.states[l].sigma = 3.0;               // candidates onto the safety margin and the stability flag's way
        d.active[l] = l % 5 != 4;
        twin[(size_t)l] = d.states[l];
    }
    for (int g = 0; g < G; ++g) {
        for (int l = 0; l < L; ++l) askKernel(d, l, l % 2 ? 0.85 : 1.0, 1);
        for (int l = 0; l < L; ++l) {
            cpq_learn_state& t = twin[(size_t)l];
            if (!d.active[l]) { CHECK(std::memcmp(&t, &d.states[l], sizeof(t)) == 0, "inactive learner %d moved", l); continue; }
            double z[kLearnVars], cand[kLearnVars], f[kLearnPop];
            int rejected = t.rejected_pairs, order[kLearnPop];
            learnNormals(t.rng, z, &rejected);
            t.rejected_pairs = rejected;
            learnAsk(t, z, cand);
            const size_t base = (size_t)l * kLearnVars;
            CHECK(sameBits(z, d.z.get() + base, kLearnVars) && sameBits(cand, d.cand.get() + base, kLearnVars), "ask of learner %d, generation %d", l, g);
            for (int i = 0; i < kLearnVars; ++i) {
                const double m = d.mapped[base + i], k = d.coef[base + i];
                CHECK(std::fabs(m) <= (l % 2 ? 0.85 : 1.0) && std::fabs(k) <= 0.85, "mapped %g, coefficient %g", m, k);
            }
            for (int i = 0; i < kLearnPop; ++i) {
                bool any = false;
                for (int k = 0; k < kLearnDim; ++k) any = any || std::fabs(d.mapped[base + i * kLearnDim + k]) >= 1.0 - 1e-12;
                CHECK(d.flag[(size_t)l * kLearnPop + i] == (any ? 1 : 0), "flag of learner %d, candidate %d", l, i);
            }
            fitnessOf((l + g) % 5, l, g, cand, f);
            for (int i = 0; i < kLearnPop; ++i) d.scores[(size_t)l * kLearnPop + i] = f[i];
            const double best = learnTell(t, p, cand, d.mapped.get() + base, f, order);
            tellKernel(d, l, p, g);
            CHECK(std::memcmp(&t, &d.states[l], sizeof(t)) == 0, "tell of learner %d, generation %d", l, g);
            CHECK(std::memcmp(order, d.order.get() + (size_t)l * kLearnPop, sizeof(order)) == 0, "order of learner %d", l);
            CHECK(std::memcmp(&best, &d.history[(size_t)l * G + g], sizeof(best)) == 0, "history of learner %d", l);
            checkOrder(f, order);
        }
    }
}

int main()
{
    for (int L : { 1, 63, 64, 65, 129 }) runLearners(L);

    // the bounded polar loop: a dead generator ends, with zeros and the counter at 81
    uint64_t dead[4] = {};
    double z[kLearnVars];
    for (double& v : z) v = 1.0;
    int rejected = 0;
    const int words = learnNormals(dead, z, &rejected);
    bool zeros = true;
    for (double v : z) zeros = zeros && v == 0.0;
    CHECK(words == kLearnPairs * 2 * kLearnMaxTries && rejected == kLearnPairs && zeros, "dead generator: %d words, %d pairs given up", words, rejected);
    cpq_learn_state st;
    learnInit(z, 1, learnDefaultParams(nullptr), st);
    CHECK(learnStateValid(st), "a fresh state is valid");
    std::memset(st.rng, 0, sizeof(st.rng));
    CHECK(!learnStateValid(st), "four zero words are refused");

    // the sort on its own: all ties, all NaN
    double f[kLearnPop];
    int order[kLearnPop];
    for (double& v : f) v = 2.0;
    learnOrder(f, order);
    for (int i = 0; i < kLearnPop; ++i) CHECK(order[i] == i, "all tied: order[%d] = %d", i, order[i]);
    for (double& v : f) v = NAN;
    learnOrder(f, order);
    for (int i = 0; i < kLearnPop; ++i) CHECK(order[i] == i, "all NaN: order[%d] = %d", i, order[i]);

    std::printf("%d checks\n%d failed checks\n", checks, failed);
    return failed ? 1 : 0;
}
