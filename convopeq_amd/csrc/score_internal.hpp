// score_internal.hpp -- cpq_scorer as engine_score.cpp defines it and engine_learn.cpp borrows it: the object, and the two halves
// of a score call (the tables of its chains and evaluations, and the three launches), which cpq_scorer_score and cpq_learner_run
// both go through.
#pragma once

#include "engine_internal.hpp"
#include "object_support.hpp"

#include <array>

using cpqi::failTo;

struct cpq_scorer {
    cpq_scorer_desc desc{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string lastError;

    cpq::ScoreTables tab;
    cpqi::ScoreTableBuffers tables;             // tab on the device
    cpq::DitherParams p{};
    unsigned long long rngStart[2][4] = {};
    cpqi::DeviceBuffer<unsigned long long> rng; // [max_candidates * 16][2][4]

    std::vector<int> nSeg;                                                  // per learner
    std::vector<std::array<int, cpq::kScoreLevels>> counts;
    std::vector<std::array<cpq::ScoreSegment, cpq::kScoreMaxSegments>> segs;
    cpqi::DeviceBuffer<double> seg, thr, recent, segGain;
    cpqi::DeviceBuffer<int> segStart;

    cpqi::DeviceBuffer<double> err, coef, blended, scores;
    cpqi::DeviceBuffer<cpq::ScoreChain> chains;
    cpqi::DeviceBuffer<cpq::ScoreEval> evals;
    cpqi::DeviceBuffer<cpq_score_parts> parts;
    cpqi::DeviceBuffer<int> countsDev, state;
    // what the last score call ran: per (learner, max_candidates slot), and the segments each learner held then
    std::vector<char> lastRan;
    std::vector<int> lastNSeg;
    int nChains = 0, nEvals = 0;                // of the tables on the device
    bool scored = false;
    cpqi::TimingEvents<3> ev;                   // around lattice and spectrum; the last member: destroyed before the buffers are freed
};

namespace cpqi {

// The tables of a call of nCand candidates per learner: allocates the error rows at the first call, records which (learner,
// candidate) pairs run (runs[learner * nCand + c] != 0; a learner without segments runs nothing), and enqueues the upload of the
// chains, the evaluations and the per-level counts and the clearing of parts and blended on the scorer's stream.  The vectors
// behind the uploads are the caller's and must live until the stream has passed them.
struct ScoreCallTables {
    std::vector<int> counts;
    std::vector<cpq::ScoreChain> chains;
    std::vector<cpq::ScoreEval> evals;
};
int scoreBuildTables(cpq_scorer* s, int nCand, const char* runs, ScoreCallTables& t);
// lattice, spectrum and reduction over the tables on the device, with the timing events around the first two
int scoreLaunch(cpq_scorer* s, int nCand, const double* levelWeights);

}  // namespace cpqi
