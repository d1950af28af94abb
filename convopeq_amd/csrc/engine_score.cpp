// engine_score.cpp -- cpq_scorer: the deterministic part of the adaptive shaper's learner (src/NoiseShaperLearner.cpp:
// configureEvaluationContexts, buildTrainingSegments, evaluateCandidate, evaluateCandidateMapped) as an object of its own beside
// cpq_engine.  The kernels are in score_kernels.hip, the tables, the segment selection and the generator start states in
// score_design.cpp.  The host owns, per learner, the segment table; the device holds the levelled segments, their masking
// thresholds, and the rows of the last score call:
//   seg   [learner][16][2][4096]            levelled segments in evaluation order (level-major, then bucket order)
//   thr   [learner][16][2049]               LeveledSegment::maskingThresholds
//   err   [learner][max_candidates][16][2][4096]   error rows of the last score call (allocated at the first one)
// A score call builds its chain and evaluation tables on the host (unstable candidates and empty learners take no lane), uploads
// them, and runs lattice, spectrum and reduction on the scorer's stream; it carries nothing to the next call.  The two halves
// (scoreBuildTables, scoreLaunch; score_internal.hpp) are also cpq_learner's (engine_learn.cpp), which builds the tables once
// for a run and launches once per generation.
#include "score_internal.hpp"

#include <cfloat>

namespace cpqi {

// LatticeNoiseShaper::prepare
cpq::DitherParams scoreDitherParams(int bits)
{
    cpq::DitherParams p{};
    p.invScale = std::ldexp(1.0, bits - 1);
    p.scale = 1.0 / p.invScale;
    p.maxV = 1.0 - (1.0 / p.invScale);
    p.headroom = cpq::kOutHeadroom;
    return p;
}

int uploadScoreTables(const cpq::ScoreTables& t, ScoreTableBuffers& b, std::string& error)
{
    auto ship = [&error](hipError_t err, const char* what) {
        if (err == hipSuccess) return true;
        error = std::string(what) + " failed: " + hipGetErrorString(err);
        return false;
    };
    std::vector<double2> tw(cpq::kScoreLen / 2);
    const long double step = -2.0L * 3.14159265358979323846264338327950288L / (long double)cpq::kScoreLen;
    for (size_t k = 0; k < tw.size(); ++k) tw[k] = make_double2((double)cosl(step * (long double)k), (double)sinl(step * (long double)k));
    const std::vector<double>* dbl[8] = { &t.weight, &t.bark, &t.athDb, &t.athPow, &t.width, &t.thrSpread, &t.spreadTonal, &t.spreadNoise };
    size_t nD = 0;
    for (auto* v : dbl) nD += v->size() + (v->size() & 1);          // every table starts on 16 bytes
    if (!b.tabD.alloc(nD + 2 * tw.size()) || !b.tabI.alloc(2 * (size_t)cpq::kScoreBins + cpq::kScoreBands + 1)) {
        error = "scorer tables could not be allocated";
        return CPQ_ERR_OOM;
    }
    const double* at[8];
    size_t off = 0;
    for (int i = 0; i < 8; ++i) {
        at[i] = b.tabD.get() + off;
        if (!ship(hipMemcpy(b.tabD.get() + off, dbl[i]->data(), dbl[i]->size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy of a scorer table"))
            return CPQ_ERR_DEVICE;
        off += dbl[i]->size() + (dbl[i]->size() & 1);
    }
    int* ip = b.tabI.get();
    if (!ship(hipMemcpy(b.tabD.get() + off, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice), "hipMemcpy of the scorer twiddles") ||
        !ship(hipMemcpy(ip, t.band.data(), cpq::kScoreBins * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy of a scorer table") ||
        !ship(hipMemcpy(ip + cpq::kScoreBins, t.range.data(), cpq::kScoreBins * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy of a scorer table") ||
        !ship(hipMemcpy(ip + 2 * cpq::kScoreBins, t.bandStart, sizeof(t.bandStart), hipMemcpyHostToDevice), "hipMemcpy of a scorer table"))
        return CPQ_ERR_DEVICE;
    b.dev = cpq::ScoreDeviceTables{ at[0], at[1], at[2], at[3], at[4], at[5], at[6], at[7], ip, ip + cpq::kScoreBins, ip + 2 * cpq::kScoreBins,
                                    reinterpret_cast<const double2*>(b.tabD.get() + off), t.flatStart, t.flatEnd, t.highStart,
                                    t.ultraStart, t.ultraShare, t.flatWeight, t.hfWeight, t.weightSum };
    return CPQ_OK;
}

}  // namespace cpqi

namespace {

using cpq::kScoreBins;
using cpq::kScoreLen;
using cpq::kScoreMaxSegments;
using cpq::kScoreRecent;

// LatticeNoiseShaper::rngState
constexpr unsigned long long kRngDefault[2][4] = {
    { 0x123456789ABCDEF0ULL, 0xFEDCBA9876543210ULL, 0x0123456789ABCDEFULL, 0xEFCDAB8967452301ULL },
    { 0x89ABCDEF01234567ULL, 0x76543210FEDCBA98ULL, 0xABCDEF0123456789ULL, 0x67452301EFCDAB89ULL } };

int uploadRng(cpq_scorer* s)
{
    std::vector<unsigned long long> table;
    cpq::scoreRngTable(s->rngStart, s->desc.max_candidates * kScoreMaxSegments, table);
    CPQ_OBJ_HIP(&s->lastError, hipSetDevice(s->device));
    CPQ_OBJ_HIP(&s->lastError, hipStreamSynchronize(s->stream));
    CPQ_OBJ_HIP(&s->lastError, hipMemcpy(s->rng, table.data(), table.size() * sizeof(table[0]), hipMemcpyHostToDevice));
    return CPQ_OK;
}

int checkLearner(cpq_scorer* s, int learner)
{
    if (learner < 0 || learner >= s->desc.n_learners) return failTo(&s->lastError, CPQ_ERR_INVALID_ARG, "learner %d outside 0..%d", learner, s->desc.n_learners - 1);
    return CPQ_OK;
}

// the most recent samples are on the device in s->recent (rows of kScoreRecent) and on the host in l, r (usable each)
int buildSegments(cpq_scorer* s, int learner, const double* l, const double* r, int usable, int32_t* nSegments)
{
    auto& segs = s->segs[learner];
    const int n = cpq::scoreSelectSegments(l, r, usable, segs.data(), s->counts[learner].data());
    s->nSeg[learner] = n;
    if (nSegments) *nSegments = n;
    if (n == 0) return CPQ_OK;
    int start[kScoreMaxSegments];
    double gain[kScoreMaxSegments];
    cpq::ScoreEval evals[kScoreMaxSegments];
    for (int i = 0; i < n; ++i) {
        start[i] = segs[i].start;
        gain[i] = segs[i].gain;
        evals[i] = cpq::ScoreEval{ learner * kScoreMaxSegments + i, learner * kScoreMaxSegments + i, 0, 0.0 };
    }
    CPQ_OBJ_HIP(&s->lastError, hipMemcpyAsync(s->segStart, start, n * sizeof(int), hipMemcpyHostToDevice, s->stream));
    CPQ_OBJ_HIP(&s->lastError, hipMemcpyAsync(s->segGain, gain, n * sizeof(double), hipMemcpyHostToDevice, s->stream));
    CPQ_OBJ_HIP(&s->lastError, hipMemcpyAsync(s->evals, evals, n * sizeof(cpq::ScoreEval), hipMemcpyHostToDevice, s->stream));
    cpq::launch_score_level(s->stream, s->recent, kScoreRecent, s->segStart, s->segGain,
                            s->seg.get() + (size_t)learner * kScoreMaxSegments * 2 * kScoreLen, n);
    cpq::launch_score_spectrum(s->stream, s->seg, s->thr, s->evals, n, s->tables.dev, nullptr, nullptr, true);
    CPQ_OBJ_HIP(&s->lastError, hipGetLastError());
    CPQ_OBJ_HIP(&s->lastError, hipStreamSynchronize(s->stream));            // the tables above are this frame's
    return CPQ_OK;
}

int setAudio(cpq_scorer* s, int learner, const double* left, const double* right, int n, int32_t* nSegments, bool onDevice)
{
    if (!s) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(checkLearner(s, learner));
    if (n < 0) return failTo(&s->lastError, CPQ_ERR_INVALID_ARG, "%d samples", n);
    if (n > 0 && (!left || !right)) return failTo(&s->lastError, CPQ_ERR_INVALID_ARG, "null buffer");
    const int usable = std::min(n, kScoreRecent);
    if (usable < kScoreLen) {                               // copiedSamples < AudioSegment::kLength: no segments, no error
        s->nSeg[learner] = 0;
        s->counts[learner].fill(0);
        if (nSegments) *nSegments = 0;
        return CPQ_OK;
    }
    CPQ_OBJ_HIP(&s->lastError, hipSetDevice(s->device));
    CPQ_OBJ_HIP(&s->lastError, hipStreamSynchronize(s->stream));
    const double* rows[2] = { left + (n - usable), right + (n - usable) };
    std::vector<double> host[2];
    for (int ch = 0; ch < 2; ++ch) {
        CPQ_OBJ_HIP(&s->lastError, hipMemcpy(s->recent.get() + (size_t)ch * kScoreRecent, rows[ch], usable * sizeof(double),
                              onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        if (onDevice) {                                     // the selection is host work: it reads a copy
            host[ch].resize(usable);
            CPQ_OBJ_HIP(&s->lastError, hipMemcpy(host[ch].data(), s->recent.get() + (size_t)ch * kScoreRecent, usable * sizeof(double), hipMemcpyDeviceToHost));
            rows[ch] = host[ch].data();
        }
    }
    return buildSegments(s, learner, rows[0], rows[1], usable, nSegments);
}

int score(cpq_scorer* s, const double* mapped, int nCand, double* scores, cpq_score_parts* parts)
{
    const int L = s->desc.n_learners;
    CPQ_OBJ_HIP(&s->lastError, hipSetDevice(s->device));
    const int nPairs = L * nCand;
    std::vector<double> coef((size_t)nPairs * cpq::kLatticeOrder);
    std::vector<int> state(nPairs);
    std::vector<char> runs(nPairs);
    for (int pair = 0; pair < nPairs; ++pair) {
        const double* k = mapped + (size_t)pair * cpq::kLatticeOrder;
        const bool refused = s->desc.stability_check && !cpq::scoreStable(k, cpq::kLatticeOrder);
        state[pair] = refused ? 1 : 0;
        runs[pair] = refused ? 0 : 1;               // a refused candidate draws no words: the chained stream passes it by
        cpq::ditherClampAdaptive(k, cpq::kLatticeOrder, &coef[(size_t)pair * cpq::kLatticeOrder]);     // setCoefficients
    }
    hipStream_t st = s->stream;
    cpqi::ScoreCallTables t;
    CPQ_OBJ_HIP(&s->lastError, hipMemcpyAsync(s->coef, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, st));
    CPQ_OBJ_HIP(&s->lastError, hipMemcpyAsync(s->state, state.data(), state.size() * sizeof(int), hipMemcpyHostToDevice, st));
    CPQ_TRY(cpqi::scoreBuildTables(s, nCand, runs.data(), t));
    CPQ_TRY(cpqi::scoreLaunch(s, nCand, s->desc.level_weights));
    CPQ_OBJ_HIP(&s->lastError, hipMemcpyAsync(scores, s->scores, (size_t)nPairs * sizeof(double), hipMemcpyDeviceToHost, st));
    if (parts) CPQ_OBJ_HIP(&s->lastError, hipMemcpyAsync(parts, s->parts, (size_t)nPairs * kScoreMaxSegments * sizeof(cpq_score_parts), hipMemcpyDeviceToHost, st));
    CPQ_OBJ_HIP(&s->lastError, hipStreamSynchronize(st));
    return CPQ_OK;
}

int checkScore(cpq_scorer* s, const double* k, int nCand, const double* scores)
{
    if (!s) return CPQ_ERR_INVALID_ARG;
    if (!k || !scores) return failTo(&s->lastError, CPQ_ERR_INVALID_ARG, "null buffer");
    if (nCand < 1 || nCand > s->desc.max_candidates) return failTo(&s->lastError, CPQ_ERR_INVALID_ARG, "%d candidates outside 1..%d", nCand, s->desc.max_candidates);
    return CPQ_OK;
}

void fillSegments(const cpq::ScoreSegment* in, int n, cpq_score_segment* out)
{
    for (int i = 0; i < n; ++i) out[i] = cpq_score_segment{ in[i].start, in[i].level, in[i].type, 0, in[i].gain };
}

}  // namespace

namespace cpqi {

int scoreBuildTables(cpq_scorer* s, int nCand, const char* runs, ScoreCallTables& t)
{
    const int L = s->desc.n_learners, maxC = s->desc.max_candidates;
    CPQ_OBJ_HIP(&s->lastError, hipSetDevice(s->device));
    if (!s->err && !s->err.alloc((size_t)L * maxC * kScoreMaxSegments * 2 * kScoreLen))
        return failTo(&s->lastError, CPQ_ERR_OOM, "the error rows of %d learners x %d candidates could not be allocated", L, maxC);
    const int nPairs = L * nCand;
    t.counts.assign((size_t)L * cpq::kScoreLevels, 0);
    t.chains.clear();
    t.evals.clear();
    std::fill(s->lastRan.begin(), s->lastRan.end(), 0);
    s->lastNSeg = s->nSeg;
    for (int l = 0; l < L; ++l) {
        for (int i = 0; i < cpq::kScoreLevels; ++i) t.counts[(size_t)l * cpq::kScoreLevels + i] = s->counts[l][i];
        const int nSeg = s->nSeg[l];
        int ranBefore = 0;
        for (int c = 0; c < nCand; ++c) {
            const int pair = l * nCand + c;
            if (!runs[pair] || nSeg == 0) continue;
            s->lastRan[(size_t)l * maxC + c] = 1;
            for (int sg = 0; sg < nSeg; ++sg) {
                const int row = (l * maxC + c) * kScoreMaxSegments + sg, src = l * kScoreMaxSegments + sg;
                const int rng = cpq::scoreRngIndex(s->desc.rng_mode, ranBefore, nSeg, sg);
                t.evals.push_back(cpq::ScoreEval{ row, src, pair * kScoreMaxSegments + sg, cpq::scoreAlpha(s->segs[l][sg].level) });
                for (int ch = 0; ch < 2; ++ch) t.chains.push_back(cpq::ScoreChain{ 2 * src + ch, 2 * row + ch, pair, 2 * rng + ch });
            }
            ++ranBefore;
        }
    }
    hipStream_t st = s->stream;
    CPQ_OBJ_HIP(&s->lastError, hipMemcpyAsync(s->countsDev, t.counts.data(), t.counts.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (!t.chains.empty()) {
        CPQ_OBJ_HIP(&s->lastError, hipMemcpyAsync(s->chains, t.chains.data(), t.chains.size() * sizeof(cpq::ScoreChain), hipMemcpyHostToDevice, st));
        CPQ_OBJ_HIP(&s->lastError, hipMemcpyAsync(s->evals, t.evals.data(), t.evals.size() * sizeof(cpq::ScoreEval), hipMemcpyHostToDevice, st));
    }
    CPQ_OBJ_HIP(&s->lastError, hipMemsetAsync(s->parts, 0, (size_t)nPairs * kScoreMaxSegments * sizeof(cpq_score_parts), st));
    CPQ_OBJ_HIP(&s->lastError, hipMemsetAsync(s->blended, 0, (size_t)nPairs * kScoreMaxSegments * sizeof(double), st));
    s->nChains = (int)t.chains.size();
    s->nEvals = (int)t.evals.size();
    return CPQ_OK;
}

int scoreLaunch(cpq_scorer* s, int nCand, const double* levelWeights)
{
    hipStream_t st = s->stream;
    CPQ_OBJ_HIP(&s->lastError, hipEventRecord(s->ev[0], st));
    cpq::launch_score_lattice(st, s->seg, s->err, s->chains, s->nChains, s->coef, s->rng, s->p);
    CPQ_OBJ_HIP(&s->lastError, hipEventRecord(s->ev[1], st));
    cpq::launch_score_spectrum(st, s->err, s->thr, s->evals, s->nEvals, s->tables.dev, s->parts, s->blended, false);
    CPQ_OBJ_HIP(&s->lastError, hipEventRecord(s->ev[2], st));
    cpq::launch_score_reduce(st, s->blended, s->countsDev, s->state, s->desc.n_learners, nCand, levelWeights, s->scores);
    CPQ_OBJ_HIP(&s->lastError, hipGetLastError());
    s->scored = true;
    return CPQ_OK;
}

}  // namespace cpqi

extern "C" {

int32_t cpq_scorer_create(const cpq_scorer_desc* d, cpq_scorer** out)
{
    if (!d || !out) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (d->n_learners < 1 || d->max_candidates < 1) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "n_learners and max_candidates must be >= 1");
    if (d->max_candidates > CPQ_SCORE_MAX_CANDIDATES)       // the start-state table is stepped word by word on the host
        return failTo(nullptr, CPQ_ERR_INVALID_ARG, "max_candidates %d above %d", d->max_candidates, CPQ_SCORE_MAX_CANDIDATES);
    if ((int64_t)d->n_learners * d->max_candidates > (1 << 20)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "more than 2^20 candidates per call");
    if (!(d->sample_rate_hz > 0.0) || !std::isfinite(d->sample_rate_hz)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "sample rate must be finite and > 0");
    if (d->bit_depth < 1 || d->bit_depth > 32) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "bit depth %d outside 1..32", d->bit_depth);
    for (double w : d->level_weights)
        if (!(w >= 0.0) || !std::isfinite(w)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "level weights must be finite and >= 0");
    if (!(d->coeff_safety_margin > 0.0) || !(d->coeff_safety_margin <= 1.0)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "safety margin outside (0, 1]");
    if (d->rng_mode != CPQ_SCORE_RNG_FRESH && d->rng_mode != CPQ_SCORE_RNG_CHAINED) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "unknown generator mode %d", d->rng_mode);
    if (d->stability_check != 0 && d->stability_check != 1) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "stability_check must be 0 or 1");

    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || nDev <= 0) {
        (void)hipGetLastError();
        return failTo(nullptr, CPQ_ERR_NO_DEVICE, "no HIP device visible: the gfx950 kernels cannot run (no CPU fallback)");
    }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return failTo(nullptr, CPQ_ERR_NO_DEVICE, "hipGetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return failTo(nullptr, CPQ_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return failTo(nullptr, CPQ_ERR_NO_DEVICE, "device %d is %s; this library ships gfx950 code only", device, prop.gcnArchName);

    std::unique_ptr<cpq_scorer, void (*)(cpq_scorer*)> s(new (std::nothrow) cpq_scorer(), cpq_scorer_destroy);
    if (!s) return failTo(nullptr, CPQ_ERR_OOM, "host allocation failed");
    s->desc = *d;
    s->device = device;
    if (!cpq::scoreTables(d->sample_rate_hz, s->tab)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "no Bark band layout at %g Hz", d->sample_rate_hz);
    s->p = cpqi::scoreDitherParams(d->bit_depth);
    std::memcpy(s->rngStart, kRngDefault, sizeof(kRngDefault));
    const size_t L = (size_t)d->n_learners, pairs = L * d->max_candidates;
    s->nSeg.assign(L, 0);
    s->lastNSeg.assign(L, 0);
    s->counts.assign(L, {});
    s->segs.resize(L);
    s->lastRan.assign(pairs, 0);
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) return failTo(nullptr, CPQ_ERR_DEVICE, "hipStreamCreate failed");
    if (s->ev.create(nullptr) != CPQ_OK) return failTo(nullptr, CPQ_ERR_DEVICE, "hipEventCreate failed");
    const bool ok = s->seg.alloc(L * kScoreMaxSegments * 2 * kScoreLen) && s->thr.alloc(L * kScoreMaxSegments * kScoreBins) &&
                    s->recent.alloc(2 * (size_t)kScoreRecent) && s->segGain.alloc(kScoreMaxSegments) && s->segStart.alloc(kScoreMaxSegments) &&
                    s->coef.alloc(pairs * cpq::kLatticeOrder) && s->blended.alloc(pairs * kScoreMaxSegments) && s->scores.alloc(pairs) &&
                    s->chains.alloc(pairs * kScoreMaxSegments * 2) && s->evals.alloc(pairs * kScoreMaxSegments) &&
                    s->parts.alloc(pairs * kScoreMaxSegments) && s->countsDev.alloc(L * cpq::kScoreLevels) && s->state.alloc(pairs) &&
                    s->rng.alloc((size_t)d->max_candidates * kScoreMaxSegments * 8);
    if (!ok) return failTo(nullptr, CPQ_ERR_OOM, "scorer buffers for %d learners x %d candidates could not be allocated", d->n_learners, d->max_candidates);
    int rc = cpqi::uploadScoreTables(s->tab, s->tables, s->lastError);
    if (rc == CPQ_OK) rc = uploadRng(s.get());
    if (rc != CPQ_OK) return failTo(nullptr, rc, "%s", s->lastError.c_str());
    *out = s.release();
    return CPQ_OK;
}

void cpq_scorer_destroy(cpq_scorer* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
    delete s;
}

const char* cpq_scorer_last_error(const cpq_scorer* s) { return s ? s->lastError.c_str() : cpq_last_error(nullptr); }

int32_t cpq_scorer_set_audio(cpq_scorer* s, int32_t learner, const double* left, const double* right, int32_t n, int32_t* nSegments)
{
    return setAudio(s, learner, left, right, n, nSegments, false);
}

int32_t cpq_scorer_set_audio_device(cpq_scorer* s, int32_t learner, const double* dLeft, const double* dRight, int32_t n, int32_t* nSegments)
{
    return setAudio(s, learner, dLeft, dRight, n, nSegments, true);
}

int32_t cpq_scorer_get_segments(const cpq_scorer* s, int32_t learner, cpq_score_segment* segments, int32_t* nSegments, int32_t counts[4])
{
    if (!s || learner < 0 || learner >= s->desc.n_learners) return CPQ_ERR_INVALID_ARG;
    if (segments) fillSegments(s->segs[learner].data(), s->nSeg[learner], segments);
    if (nSegments) *nSegments = s->nSeg[learner];
    if (counts) std::memcpy(counts, s->counts[learner].data(), sizeof(int32_t) * cpq::kScoreLevels);
    return CPQ_OK;
}

int32_t cpq_scorer_read_thresholds(cpq_scorer* s, int32_t learner, int32_t segment, double* thresholds)
{
    if (!s) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(checkLearner(s, learner));
    if (!thresholds) return failTo(&s->lastError, CPQ_ERR_INVALID_ARG, "null buffer");
    if (segment < 0 || segment >= s->nSeg[learner]) return failTo(&s->lastError, CPQ_ERR_INVALID_ARG, "segment %d outside the learner's %d", segment, s->nSeg[learner]);
    CPQ_OBJ_HIP(&s->lastError, hipSetDevice(s->device));
    CPQ_OBJ_HIP(&s->lastError, hipStreamSynchronize(s->stream));
    CPQ_OBJ_HIP(&s->lastError, hipMemcpy(thresholds, s->thr.get() + ((size_t)learner * kScoreMaxSegments + segment) * kScoreBins, kScoreBins * sizeof(double),
                          hipMemcpyDeviceToHost));
    return CPQ_OK;
}

int32_t cpq_scorer_score(cpq_scorer* s, const double* mapped, int32_t nCand, double* scores, cpq_score_parts* parts)
{
    CPQ_TRY(checkScore(s, mapped, nCand, scores));
    return score(s, mapped, nCand, scores, parts);
}

int32_t cpq_scorer_score_raw(cpq_scorer* s, const double* raw, int32_t nCand, double* scores, cpq_score_parts* parts)
{
    CPQ_TRY(checkScore(s, raw, nCand, scores));
    std::vector<double> mapped((size_t)s->desc.n_learners * nCand * cpq::kLatticeOrder);
    for (size_t i = 0; i < mapped.size(); i += cpq::kLatticeOrder) cpq::scoreMapRaw(raw + i, s->desc.coeff_safety_margin, &mapped[i]);
    return score(s, mapped.data(), nCand, scores, parts);
}

int32_t cpq_scorer_set_rng_start(cpq_scorer* s, const uint64_t state[2][4])
{
    if (!s) return CPQ_ERR_INVALID_ARG;
    if (!state) return failTo(&s->lastError, CPQ_ERR_INVALID_ARG, "null state");
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "generator words travel as unsigned long long");
    std::memcpy(s->rngStart, state, sizeof(s->rngStart));
    return uploadRng(s);
}

int32_t cpq_scorer_read_error(cpq_scorer* s, int32_t learner, int32_t candidate, int32_t segment, double* left, double* right)
{
    if (!s) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(checkLearner(s, learner));
    if (candidate < 0 || candidate >= s->desc.max_candidates || segment < 0 || segment >= kScoreMaxSegments)
        return failTo(&s->lastError, CPQ_ERR_INVALID_ARG, "candidate %d or segment %d out of range", candidate, segment);
    if (!s->scored || !s->lastRan[(size_t)learner * s->desc.max_candidates + candidate] || segment >= s->lastNSeg[learner])
        return failTo(&s->lastError, CPQ_ERR_NOT_READY, "the last score call did not run learner %d, candidate %d, segment %d", learner, candidate, segment);
    CPQ_OBJ_HIP(&s->lastError, hipSetDevice(s->device));
    CPQ_OBJ_HIP(&s->lastError, hipStreamSynchronize(s->stream));
    const double* row = s->err.get() + (((size_t)learner * s->desc.max_candidates + candidate) * kScoreMaxSegments + segment) * 2 * kScoreLen;
    if (left) CPQ_OBJ_HIP(&s->lastError, hipMemcpy(left, row, kScoreLen * sizeof(double), hipMemcpyDeviceToHost));
    if (right) CPQ_OBJ_HIP(&s->lastError, hipMemcpy(right, row + kScoreLen, kScoreLen * sizeof(double), hipMemcpyDeviceToHost));
    return CPQ_OK;
}

int32_t cpq_scorer_last_timing(cpq_scorer* s, double* latticeMs, double* spectrumMs)
{
    if (!s) return CPQ_ERR_INVALID_ARG;
    if (!s->scored) return failTo(&s->lastError, CPQ_ERR_NOT_READY, "no score call yet");
    float a = 0.0f, b = 0.0f;
    CPQ_OBJ_HIP(&s->lastError, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
    CPQ_OBJ_HIP(&s->lastError, hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
    if (latticeMs) *latticeMs = a;
    if (spectrumMs) *spectrumMs = b;
    return CPQ_OK;
}

int32_t cpq_score_design(double rate, double* weight, double* bark, double* athDb, double* width, int32_t* band, int32_t* range,
                         int32_t bins[4], double scalars[4])
{
    if (!(rate > 0.0) || !std::isfinite(rate)) return CPQ_ERR_INVALID_ARG;
    cpq::ScoreTables t;
    if (!cpq::scoreTables(rate, t)) return CPQ_ERR_INVALID_ARG;
    const size_t nb = kScoreBins * sizeof(double);
    if (weight) std::memcpy(weight, t.weight.data(), nb);
    if (bark) std::memcpy(bark, t.bark.data(), nb);
    if (athDb) std::memcpy(athDb, t.athDb.data(), nb);
    if (width) std::memcpy(width, t.width.data(), nb);
    if (band) std::memcpy(band, t.band.data(), kScoreBins * sizeof(int32_t));
    if (range) std::memcpy(range, t.range.data(), kScoreBins * sizeof(int32_t));
    if (bins) { bins[0] = t.flatStart; bins[1] = t.flatEnd; bins[2] = t.highStart; bins[3] = t.ultraStart; }
    if (scalars) { scalars[0] = t.ultraShare; scalars[1] = t.flatWeight; scalars[2] = t.hfWeight; scalars[3] = t.weightSum; }
    return CPQ_OK;
}

int32_t cpq_score_select_segments(const double* left, const double* right, int32_t n, cpq_score_segment* segments, int32_t* nSegments,
                                  int32_t counts[4])
{
    if (n < 0 || (n > 0 && (!left || !right))) return CPQ_ERR_INVALID_ARG;
    cpq::ScoreSegment segs[kScoreMaxSegments];
    int cnt[cpq::kScoreLevels];
    const int total = cpq::scoreSelectSegments(left, right, n, segs, cnt);
    if (segments) fillSegments(segs, total, segments);
    if (nSegments) *nSegments = total;
    if (counts) std::memcpy(counts, cnt, sizeof(cnt));
    return CPQ_OK;
}

}  // extern "C"
