// engine_learn.cpp -- cpq_learner: the reference's CmaEsOptimizer (src/CmaEsOptimizer.h) and the generation loop of
// NoiseShaperLearner around a cpq_scorer, with the learners' states on the device.  The arithmetic is learn_plan.hpp's, the
// kernels are in learn_kernels.hip.  A run builds the scorer's tables once for 18 candidates of every active learner (every
// candidate runs: a set the stability check refuses is flagged by k_learn_ask and scores CPQ_SCORE_UNSTABLE in the reduction) and
// enqueues ask -> lattice -> spectrum -> reduce -> tell per generation on the scorer's stream, with no host work in between.
//   states  [learner]            cpq_learn_state, as the ABI declares it
//   z, cand, mapped [learner][18][9], order [learner][18]     the last generation, for reading back
//   hist    [learner][G]         the best candidate score of every generation of the last run
// The scorer's coef, state and scores buffers carry a generation from ask through the scorer to tell.
#include "score_internal.hpp"

#include <cfloat>

struct cpq_learner {
    cpq_scorer* sc = nullptr;
    std::string lastError;
    cpq_learn_params params{};
    cpqi::DeviceBuffer<cpq_learn_state> states;
    cpqi::DeviceBuffer<double> z, cand, mapped, hist;
    cpqi::DeviceBuffer<int> order, active;
    std::vector<char> inited;
    std::vector<int> lastActive, generated;     // of the last run; generations made so far, per learner
    cpqi::ScoreCallTables tables;               // behind the last run's uploads
    std::vector<int> activeHost;
    int histStride = 0, lastG = 0;
    bool ran = false;
    cpqi::TimingEvents<4> ev;                   // around ask and tell of a run's last generation; the last member: destroyed before the buffers
};

namespace {

using cpq::kLearnDim;
using cpq::kLearnPop;
using cpq::kLearnVars;

int checkLearner(cpq_learner* l, int learner)
{
    const int L = l->sc->desc.n_learners;
    if (learner < 0 || learner >= L) return failTo(&l->lastError, CPQ_ERR_INVALID_ARG, "learner %d outside 0..%d", learner, L - 1);
    return CPQ_OK;
}

int sync(cpq_learner* l)
{
    CPQ_OBJ_HIP(&l->lastError, hipSetDevice(l->sc->device));
    CPQ_OBJ_HIP(&l->lastError, hipStreamSynchronize(l->sc->stream));
    return CPQ_OK;
}

}  // namespace

extern "C" {

int32_t cpq_learner_create(cpq_scorer* sc, cpq_learner** out)
{
    if (out) *out = nullptr;
    if (!sc || !out) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "null argument");
    if (sc->desc.max_candidates < kLearnPop)
        return failTo(nullptr, CPQ_ERR_INVALID_ARG, "the scorer holds %d candidates per learner; a generation has %d", sc->desc.max_candidates, kLearnPop);
    if (sc->desc.rng_mode != CPQ_SCORE_RNG_FRESH) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "the learner needs a scorer in CPQ_SCORE_RNG_FRESH mode");
    std::unique_ptr<cpq_learner, void (*)(cpq_learner*)> l(new (std::nothrow) cpq_learner(), cpq_learner_destroy);
    if (!l) return failTo(nullptr, CPQ_ERR_OOM, "host allocation failed");
    l->sc = sc;
    l->params = cpq::learnDefaultParams(sc->desc.level_weights);
    const size_t L = (size_t)sc->desc.n_learners;
    l->inited.assign(L, 0);
    l->lastActive.assign(L, 0);
    l->generated.assign(L, 0);
    if (hipSetDevice(sc->device) != hipSuccess) return failTo(nullptr, CPQ_ERR_DEVICE, "hipSetDevice failed");
    if (l->ev.create(nullptr) != CPQ_OK) return failTo(nullptr, CPQ_ERR_DEVICE, "hipEventCreate failed");
    if (!l->states.alloc(L) || !l->z.alloc(L * kLearnVars) || !l->cand.alloc(L * kLearnVars) || !l->mapped.alloc(L * kLearnVars) ||
        !l->order.alloc(L * kLearnPop) || !l->active.alloc(L))
        return failTo(nullptr, CPQ_ERR_OOM, "learner buffers for %d learners could not be allocated", sc->desc.n_learners);
    if (hipMemset(l->states, 0, L * sizeof(cpq_learn_state)) != hipSuccess) return failTo(nullptr, CPQ_ERR_DEVICE, "hipMemset failed");
    *out = l.release();
    return CPQ_OK;
}

void cpq_learner_destroy(cpq_learner* l)
{
    if (!l) return;
    if (l->sc) {
        (void)hipSetDevice(l->sc->device);
        (void)hipStreamSynchronize(l->sc->stream);
    }
    delete l;
}

const char* cpq_learner_last_error(const cpq_learner* l) { return l ? l->lastError.c_str() : cpq_last_error(nullptr); }

int32_t cpq_learner_init(cpq_learner* l, int32_t learner, const double parcor[9], uint64_t seed)
{
    if (!l) return CPQ_ERR_INVALID_ARG;
    if (!parcor) return failTo(&l->lastError, CPQ_ERR_INVALID_ARG, "null coefficient set");
    for (int i = 0; i < kLearnDim; ++i)
        if (!std::isfinite(parcor[i])) return failTo(&l->lastError, CPQ_ERR_INVALID_ARG, "coefficient %d is not finite", i);
    int l0 = 0, l1 = l->sc->desc.n_learners;
    if (learner != CPQ_ALL_STREAMS) {
        CPQ_TRY(checkLearner(l, learner));
        l0 = learner;
        l1 = learner + 1;
    }
    CPQ_TRY(sync(l));
    std::vector<cpq_learn_state> st((size_t)(l1 - l0));
    for (int i = l0; i < l1; ++i) {
        cpq::learnInit(parcor, seed + (uint64_t)i, l->params, st[(size_t)(i - l0)]);
        l->inited[(size_t)i] = 1;
        l->generated[(size_t)i] = 0;
    }
    CPQ_OBJ_HIP(&l->lastError, hipMemcpy(l->states.get() + l0, st.data(), st.size() * sizeof(cpq_learn_state), hipMemcpyHostToDevice));
    return CPQ_OK;
}

int32_t cpq_learner_set_params(cpq_learner* l, const cpq_learn_params* p)
{
    if (!l) return CPQ_ERR_INVALID_ARG;
    if (!p) return failTo(&l->lastError, CPQ_ERR_INVALID_ARG, "null parameters");
    if (!cpq::learnParamsValid(*p)) return failTo(&l->lastError, CPQ_ERR_INVALID_ARG, "parameters out of range");
    l->params = *p;
    return CPQ_OK;
}

int32_t cpq_learner_run(cpq_learner* l, int32_t nGenerations)
{
    if (!l) return CPQ_ERR_INVALID_ARG;
    if (nGenerations < 1 || nGenerations > CPQ_LEARN_MAX_GENERATIONS)
        return failTo(&l->lastError, CPQ_ERR_INVALID_ARG, "%d generations outside 1..%d", nGenerations, CPQ_LEARN_MAX_GENERATIONS);
    cpq_scorer* sc = l->sc;
    const int L = sc->desc.n_learners;
    std::vector<int> active((size_t)L);
    for (int i = 0; i < L; ++i) {
        active[(size_t)i] = sc->nSeg[(size_t)i] >= 2 ? 1 : 0;   // the reference waits for audio below two segments
        if (active[(size_t)i] && !l->inited[(size_t)i]) return failTo(&l->lastError, CPQ_ERR_NOT_READY, "learner %d holds segments and was never initialised", i);
    }
    CPQ_TRY(sync(l));                                           // the last run's tables and history are free
    if (nGenerations > l->histStride) {
        if (!l->hist.alloc((size_t)L * nGenerations)) { l->histStride = 0; return failTo(&l->lastError, CPQ_ERR_OOM, "the history of %d generations could not be allocated", nGenerations); }
        l->histStride = nGenerations;
    }
    l->activeHost = active;
    std::vector<char> runs((size_t)L * kLearnPop);
    for (int i = 0; i < L; ++i)
        for (int c = 0; c < kLearnPop; ++c) runs[(size_t)i * kLearnPop + c] = (char)active[(size_t)i];
    hipStream_t st = sc->stream;
    CPQ_OBJ_HIP(&l->lastError, hipMemcpyAsync(l->active, l->activeHost.data(), (size_t)L * sizeof(int), hipMemcpyHostToDevice, st));
    if (cpqi::scoreBuildTables(sc, kLearnPop, runs.data(), l->tables) != CPQ_OK) return failTo(&l->lastError, CPQ_ERR_DEVICE, "%s", sc->lastError.c_str());
    const bool check = sc->desc.stability_check != 0;
    for (int g = 0; g < nGenerations; ++g) {
        const bool last = g == nGenerations - 1;
        if (last) CPQ_OBJ_HIP(&l->lastError, hipEventRecord(l->ev[0], st));
        cpq::launch_learn_ask(st, l->states, l->active, L, sc->desc.coeff_safety_margin, check, sc->coef, sc->state, l->z, l->cand, l->mapped);
        if (last) CPQ_OBJ_HIP(&l->lastError, hipEventRecord(l->ev[1], st));
        if (cpqi::scoreLaunch(sc, kLearnPop, l->params.level_weights) != CPQ_OK) return failTo(&l->lastError, CPQ_ERR_DEVICE, "%s", sc->lastError.c_str());
        if (last) CPQ_OBJ_HIP(&l->lastError, hipEventRecord(l->ev[2], st));
        cpq::launch_learn_tell(st, l->states, l->active, L, l->params, l->cand, l->mapped, sc->scores, l->order, l->hist, l->histStride, g);
        if (last) CPQ_OBJ_HIP(&l->lastError, hipEventRecord(l->ev[3], st));
    }
    CPQ_OBJ_HIP(&l->lastError, hipGetLastError());
    l->lastActive = active;
    l->lastG = nGenerations;
    for (int i = 0; i < L; ++i)
        if (active[(size_t)i]) l->generated[(size_t)i] += nGenerations;
    l->ran = true;
    return CPQ_OK;
}

int32_t cpq_learner_get_state(cpq_learner* l, int32_t learner, cpq_learn_state* out)
{
    if (!l) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(checkLearner(l, learner));
    if (!out) return failTo(&l->lastError, CPQ_ERR_INVALID_ARG, "null state");
    CPQ_TRY(sync(l));
    CPQ_OBJ_HIP(&l->lastError, hipMemcpy(out, l->states.get() + learner, sizeof(cpq_learn_state), hipMemcpyDeviceToHost));
    return CPQ_OK;
}

int32_t cpq_learner_set_state(cpq_learner* l, int32_t learner, const cpq_learn_state* in)
{
    if (!l) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(checkLearner(l, learner));
    if (!in) return failTo(&l->lastError, CPQ_ERR_INVALID_ARG, "null state");
    if (!cpq::learnStateValid(*in)) return failTo(&l->lastError, CPQ_ERR_INVALID_ARG, "state refused: a value that is not finite, a generator of four zero words or a negative counter");
    CPQ_TRY(sync(l));
    CPQ_OBJ_HIP(&l->lastError, hipMemcpy(l->states.get() + learner, in, sizeof(cpq_learn_state), hipMemcpyHostToDevice));
    l->inited[(size_t)learner] = 1;
    return CPQ_OK;
}

int32_t cpq_learner_read_generation(cpq_learner* l, int32_t learner, double* z, double* candidates, double* mapped, double* scores,
                                    int32_t* order)
{
    if (!l) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(checkLearner(l, learner));
    if (!l->ran || !l->lastActive[(size_t)learner]) return failTo(&l->lastError, CPQ_ERR_NOT_READY, "the last run made no generation for learner %d", learner);
    CPQ_TRY(sync(l));
    const size_t at = (size_t)learner * kLearnVars, bytes = kLearnVars * sizeof(double);
    if (z) CPQ_OBJ_HIP(&l->lastError, hipMemcpy(z, l->z.get() + at, bytes, hipMemcpyDeviceToHost));
    if (candidates) CPQ_OBJ_HIP(&l->lastError, hipMemcpy(candidates, l->cand.get() + at, bytes, hipMemcpyDeviceToHost));
    if (mapped) CPQ_OBJ_HIP(&l->lastError, hipMemcpy(mapped, l->mapped.get() + at, bytes, hipMemcpyDeviceToHost));
    if (scores) CPQ_OBJ_HIP(&l->lastError, hipMemcpy(scores, l->sc->scores.get() + (size_t)learner * kLearnPop, kLearnPop * sizeof(double), hipMemcpyDeviceToHost));
    if (order) CPQ_OBJ_HIP(&l->lastError, hipMemcpy(order, l->order.get() + (size_t)learner * kLearnPop, kLearnPop * sizeof(int32_t), hipMemcpyDeviceToHost));
    return CPQ_OK;
}

int32_t cpq_learner_read_history(cpq_learner* l, int32_t learner, double* best, int32_t* n)
{
    if (!l) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(checkLearner(l, learner));
    const int count = (l->ran && l->lastActive[(size_t)learner]) ? l->lastG : 0;
    if (n) *n = count;
    if (!best || count == 0) return CPQ_OK;
    CPQ_TRY(sync(l));
    CPQ_OBJ_HIP(&l->lastError, hipMemcpy(best, l->hist.get() + (size_t)learner * l->histStride, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    return CPQ_OK;
}

int32_t cpq_learner_published(cpq_learner* l, int32_t learner, double k[9])
{
    if (!l) return CPQ_ERR_INVALID_ARG;
    if (!k) return failTo(&l->lastError, CPQ_ERR_INVALID_ARG, "null buffer");
    cpq_learn_state st;
    CPQ_TRY(cpq_learner_get_state(l, learner, &st));
    cpq::learnPublished(st.best_raw, k);
    return CPQ_OK;
}

/* Diagnostic (tools/learn_bench.py): events around ask and tell of the last run's last generation, in milliseconds */
int32_t cpq_learner_last_timing(cpq_learner* l, double* askMs, double* tellMs)
{
    if (!l) return CPQ_ERR_INVALID_ARG;
    if (!l->ran) return failTo(&l->lastError, CPQ_ERR_NOT_READY, "no run yet");
    CPQ_TRY(sync(l));
    float a = 0.0f, b = 0.0f;
    CPQ_OBJ_HIP(&l->lastError, hipEventElapsedTime(&a, l->ev[0], l->ev[1]));
    CPQ_OBJ_HIP(&l->lastError, hipEventElapsedTime(&b, l->ev[2], l->ev[3]));
    if (askMs) *askMs = a;
    if (tellMs) *tellMs = b;
    return CPQ_OK;
}

// ---- the host side of learn_plan.hpp

int32_t cpq_learn_init_host(const double parcor[9], uint64_t seed, const cpq_learn_params* params, cpq_learn_state* out)
{
    if (!parcor || !out) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_init: null argument");
    for (int i = 0; i < kLearnDim; ++i)
        if (!std::isfinite(parcor[i])) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_init: coefficient %d is not finite", i);
    if (params && !cpq::learnParamsValid(*params)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_init: parameters out of range");
    cpq::learnInit(parcor, seed, params ? *params : cpq::learnDefaultParams(nullptr), *out);
    return CPQ_OK;
}

int32_t cpq_learn_normals_host(cpq_learn_state* state, double z[162], int32_t* words)
{
    if (!state || !z) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_normals: null argument");
    int rejected = state->rejected_pairs;
    const int n = cpq::learnNormals(state->rng, z, &rejected);
    state->rejected_pairs = rejected;
    if (words) *words = n;
    return CPQ_OK;
}

int32_t cpq_learn_ask_host(const cpq_learn_state* state, const double z[162], double candidates[162])
{
    if (!state || !z || !candidates) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_ask: null argument");
    cpq::learnAsk(*state, z, candidates);
    return CPQ_OK;
}

int32_t cpq_learn_tell_host(cpq_learn_state* state, const cpq_learn_params* params, const double candidates[162], const double mapped[162],
                            const double fitness[18], int32_t order[18])
{
    if (!state || !params || !candidates || !fitness) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_tell: null argument");
    if (!cpq::learnParamsValid(*params)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_tell: parameters out of range");
    int own[kLearnPop];
    cpq::learnTell(*state, *params, candidates, mapped, fitness, order ? order : own);
    return CPQ_OK;
}

int32_t cpq_learn_phase(int32_t mode, double seconds)
{
    if (!std::isfinite(seconds)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_phase: seconds not finite");
    const int phase = cpq::learnPhase(mode, seconds);
    if (phase == 0) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_phase: unknown mode %d", mode);
    return phase;
}

int32_t cpq_learn_phase_params(int32_t mode, int32_t phase, cpq_learn_params* out, double* interval)
{
    if (!out) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_phase_params: null argument");
    double iv = 0.0;
    if (!cpq::learnPhaseParams(mode, phase, *out, iv)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "learn_phase_params: mode %d or phase %d unknown", mode, phase);
    if (interval) *interval = iv;
    return CPQ_OK;
}

}  // extern "C"
