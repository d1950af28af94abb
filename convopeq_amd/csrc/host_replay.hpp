// host_replay.hpp -- the reference's per-stream ramps and fades, replayed on the host once per callback before any kernel
// is launched.  All four are its LinearRamp (src/DspNumericPolicy.h:319-421) with a little policy on top:
//   GainRamp     smoothTotalGain, 50 ms: setTargetValue + skip(B) per callback         (planEqGain)
//   EqBypass     bypassFadeGain, 5 ms: requested / effective / released per callback   (planEqCall)
//   MixRamp      mixSmoother: getNextValue per sample over a prefix of the call        (planProcRest, planProcMix)
//   LatencyFade  crossfadeGain, 20 ms, between the delay in use and the new one        (planProcLatency)
// and, built on the first two, the EQ's plan of a whole call, which engine_eq.cpp only carries out: planEqGain (which streams
// ramp, their segments, whose device gain flips) and planEqCall / needsSilence / assignResets / cutPieces (classes, band resets
// and the pieces of equal class the call is cut into); built on the last two, the processor-level stage's plan of a call, which
// engine_proc.cpp only carries out: planProcRest (whose convolver rests), planProcMix (the smoothed prefixes and their gain
// pairs) and planProcLatency (the ranges between fade starts, their delays and fade values), with the stage's pure arithmetic
// (equalPowerSin, staticMixGains, procDelay).
// Plain integer and double arithmetic, operation for operation the reference's; no HIP, no engine: a stepper returns plain
// data and the caller turns it into uploads and launches.  What has to be known BEFORE state may move (which convolvers rest
// in a call) is asked of a copy of the ramp, once, in planProcRest.
// tests/sanitize/host_replay_check.cpp drives this header alone, on the CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace cpqi {

struct LinearRamp {
    double current = 1.0, target = 1.0, step = 0.0;     // every ramp of the engine is a gain that rests at unity
    int remaining = 0, totalSteps = 1;

    static int stepsFor(double rate, double seconds)
    {
        const int n = (int)(rate * seconds + 0.5);
        return n > 0 ? n : 1;
    }
    bool isSmoothing() const { return remaining > 0; }
    void setCurrentAndTargetValue(double v)
    {
        current = target = v;
        step = 0.0;
        remaining = 0;
    }
    // a retarget while the ramp runs keeps the steps it has left; at rest it takes totalSteps
    void setTargetValue(double v)
    {
        if (v == target) return;
        target = v;
        const int n = isSmoothing() ? remaining : totalSteps;
        step = (target - current) / (double)n;
        remaining = n;
    }
    double getNextValue()
    {
        if (!isSmoothing()) return current;
        current += step;
        if (--remaining <= 0) current = target;     // the last step lands on the target itself
        return current;
    }
    // n samples at once: ONE multiply-add, not n additions
    void skip(int n)
    {
        if (n <= 0 || !isSmoothing()) return;
        if (n >= remaining) { current = target; remaining = 0; return; }
        current += step * (double)n;
        remaining -= n;
    }
};

// total-gain ramp (src/eqprocessor/EQProcessor.Processing.cpp:1262-1274)
struct GainRamp {
    LinearRamp ramp;
    double wanted = 1.0;
    bool devUnity = false;      // the cascade kernel's table holds unity gain: the ramp kernel applies the gain

    bool moving() const { return ramp.isSmoothing() || std::fabs(ramp.target - wanted) > 1e-6 || ramp.current != wanted; }
    void snap() { ramp.setCurrentAndTargetValue(wanted); }
    struct Segment { double start, increment; };        // gain of the callback's first sample, change per sample
    Segment callback(int B, int totalSteps)
    {
        if (std::fabs(ramp.target - wanted) > 1e-6) { ramp.totalSteps = totalSteps; ramp.setTargetValue(wanted); }
        const double start = ramp.current;
        ramp.skip(B);
        return { start, (ramp.current - start) / (double)B };
    }
};

// EQ bypass (EQProcessor::setBypassFromRT + the fade of the basic process(block), Processing.cpp:499-526, 977-1015)
struct EqBypass {
    enum Class : char { kNormal = 0, kFade = 1, kPass = 2 };
    bool requested = false, effective = false;
    LinearRamp fade;
    int mode = 0;       // what the device tables of the stream hold now: 0 parameters as set, 1 band nodes of the basic
                        // path, 2 pass-through

    bool active() const { return requested || effective || fade.isSmoothing() || mode != 0; }
    // prepareToPlay / reset / before the first callback: the fade is synchronised with the request, not run
    void sync()
    {
        effective = requested;
        fade.setCurrentAndTargetValue(requested ? 0.0 : 1.0);
    }
    struct Step { Class cls; bool released; };          // released: the bypass ends here, every band state is to be cleared
    // one callback of B samples; the fade values it draws (fewer than B when the ramp ends inside it) are appended to vals
    Step callback(int B, int totalSteps, std::vector<double>& vals)
    {
        Step st{ kNormal, false };
        const double want = requested ? 0.0 : 1.0;
        if (std::fabs(fade.target - want) > 1.0e-12) {
            if (!requested && effective) { st.released = true; effective = false; }
            fade.totalSteps = totalSteps;
            fade.setTargetValue(want);
        }
        const bool transition = fade.isSmoothing();
        if (requested && !effective && !transition) effective = true;
        if (requested && effective && !transition) { st.cls = kPass; return st; }
        if (!transition) return st;
        st.cls = kFade;
        for (int i = 0; i < B && fade.isSmoothing(); ++i) vals.push_back(fade.getNextValue());
        if (!fade.isSmoothing()) effective = requested;
        return st;
    }
};

// ---- the EQ's plan of one range of cbs callbacks of B samples over S streams (engine_eq.cpp carries it out)

// Total gain (Processing.cpp:1262-1274): evaluated per callback on the host, applied by the ramp kernel only while some stream
// is moving.  A stream's ramp rests in the range while its AGC is on (agcOn[s]) or it is bypassed for the whole range (pass, or
// null: none is).
inline bool gainSkipped(const int* agcOn, const char* pass, int s) { return agcOn[s] || (pass && pass[s]); }
// does planEqGain find a ramp to move?  Nothing moves here: the engine refuses a ragged range on this answer
inline bool anyGainRamp(const GainRamp* ramps, const int* agcOn, const char* pass, int S)
{
    for (int s = 0; s < S; ++s)
        if (!gainSkipped(agcOn, pass, s) && ramps[s].moving()) return true;
    return false;
}
struct EqGainPlan {
    bool anyRamp = false;
    std::vector<int> rampOn;            // [S] the ramp kernel applies this stream's gain; empty while nothing ramps
    std::vector<double> segments;       // [S][cbs][2] start, increment per callback; empty while nothing ramps
    // streams whose gain the ramp kernel applies need unity gain in the cascade kernel's table, and `wanted` back afterwards:
    // the table entries to rewrite.  The caller uploads them and sets GainRamp::devUnity.
    struct Flip { int s; bool unity; double gain; };
    std::vector<Flip> flips;
};
// steps every moving ramp through the range; a range in which nothing moves and nothing flips allocates nothing
inline EqGainPlan planEqGain(GainRamp* ramps, const int* agcOn, const char* pass, int S, int cbs, int B, int totalSteps)
{
    EqGainPlan g;
    for (int s = 0; s < S; ++s) {
        GainRamp& r = ramps[s];
        if (gainSkipped(agcOn, pass, s) || !r.moving()) continue;
        if (!g.anyRamp) { g.rampOn.assign((size_t)S, 0); g.segments.assign((size_t)S * cbs * 2, 0.0); g.anyRamp = true; }
        g.rampOn[(size_t)s] = 1;
        for (int t = 0; t < cbs; ++t) {
            const GainRamp::Segment seg = r.callback(B, totalSteps);
            g.segments[((size_t)s * cbs + t) * 2] = seg.start;
            g.segments[((size_t)s * cbs + t) * 2 + 1] = seg.increment;
        }
    }
    for (int s = 0; s < S; ++s) {
        if (gainSkipped(agcOn, pass, s)) continue;
        const bool needUnity = g.anyRamp && g.rampOn[(size_t)s];
        if (needUnity != ramps[s].devUnity) g.flips.push_back({ s, needUnity, needUnity ? 1.0 : ramps[s].wanted });
    }
    return g;
}

// Bypass (DSPCore's setBypassFromRT + process per callback): class, release and fade values of every (stream, callback), then
// the band resets, then the pieces.  Indexed [s * cbs + t].
struct EqCallPlan {
    int S = 0, cbs = 0, B = 0;
    std::vector<char> cls;                      // EqBypass::Class
    std::vector<char> released;                 // the bypass is released here: every band is to be cleared
    std::vector<uint32_t> reset;                // bands cleared at the start of the callback (assignResets)
    std::vector<std::vector<double>> fade;      // per stream: the fade values of its kFade callbacks, in order
    std::vector<double> fadeRest;               // per stream: where the fade stands behind the range
    size_t at(int s, int t) const { return (size_t)s * cbs + t; }
};
inline EqCallPlan planEqCall(EqBypass* bypass, int S, int cbs, int B, int totalSteps)
{
    EqCallPlan p;
    p.S = S; p.cbs = cbs; p.B = B;
    p.cls.assign((size_t)S * cbs, EqBypass::kNormal);
    p.released.assign((size_t)S * cbs, 0);
    p.reset.assign((size_t)S * cbs, 0u);
    p.fade.resize((size_t)S);
    p.fadeRest.resize((size_t)S);
    for (int s = 0; s < S; ++s) {
        for (int t = 0; t < cbs; ++t) {
            const EqBypass::Step st = bypass[s].callback(B, totalSteps, p.fade[(size_t)s]);
            p.cls[p.at(s, t)] = st.cls;
            p.released[p.at(s, t)] = st.released ? 1 : 0;
        }
        p.fadeRest[(size_t)s] = bypass[s].fade.current;
    }
    return p;
}
// A pending band reset is taken by the first callback that is fading (canSafelyResetState, Processing.cpp:565-568) or whose
// input block is silent; a fully bypassed callback returns before it gets there.  Silence is only known on the device: does some
// stream with a pending reset meet a kNormal callback before a kFade one?
inline bool needsSilence(const EqCallPlan& p, const uint32_t* pending)
{
    for (int s = 0; s < p.S; ++s) {
        if (!pending[s]) continue;
        for (int t = 0; t < p.cbs; ++t) {
            if (p.cls[p.at(s, t)] == EqBypass::kFade) break;
            if (p.cls[p.at(s, t)] == EqBypass::kNormal) return true;
        }
    }
    return false;
}
// silent: [s * cbs + t] != 0 where the stream's input block is silent, or null (nothing was asked: needsSilence was false).
// Fills p.reset, leaves in pending[] what no callback took; true: some stream still has a reset pending
inline bool assignResets(EqCallPlan& p, uint32_t* pending, const int* silent)
{
    bool anyLeft = false;
    for (int s = 0; s < p.S; ++s) {
        uint32_t m = pending[s];
        for (int t = 0; t < p.cbs; ++t) {
            if (p.released[p.at(s, t)]) m = 0xFFFFFFFFu;
            if (!m) continue;
            const char k = p.cls[p.at(s, t)];
            if (k == EqBypass::kFade || (k == EqBypass::kNormal && silent && silent[p.at(s, t)])) {
                p.reset[p.at(s, t)] = m;
                m = 0u;
            }
        }
        pending[s] = m;
        anyLeft = anyLeft || m != 0u;
    }
    return anyLeft;
}
// A piece: a maximal run of callbacks [c0, c1) in which no stream changes class and no callback after the first carries a reset;
// it runs the ordinary kernels with the streams' tables switched to their class.
struct EqPiece {
    int c0 = 0, c1 = 0;
    struct Stream {
        char cls;               // EqBypass::Class throughout the piece
        uint32_t reset;         // bands cleared in front of the piece
        size_t fadeStart;       // kFade: the piece's samples take fade[fadeStart ... fadeStart + fadeLen), then fadeEnd
        int fadeLen;
        double fadeEnd;
    };
    std::vector<Stream> streams;
};
inline std::vector<EqPiece> cutPieces(const EqCallPlan& p)
{
    std::vector<EqPiece> pieces;
    std::vector<size_t> used((size_t)p.S, 0);           // fade values of the stream consumed by earlier pieces
    for (int c0 = 0; c0 < p.cbs;) {
        auto sameClass = [&](int t) {
            for (int s = 0; s < p.S; ++s)
                if (p.cls[p.at(s, t)] != p.cls[p.at(s, c0)] || p.reset[p.at(s, t)]) return false;
            return true;
        };
        int c1 = c0 + 1;
        while (c1 < p.cbs && sameClass(c1)) ++c1;
        EqPiece pc;
        pc.c0 = c0; pc.c1 = c1;
        const size_t n = (size_t)(c1 - c0) * p.B;
        for (int s = 0; s < p.S; ++s) {
            const std::vector<double>& f = p.fade[(size_t)s];
            EqPiece::Stream ps{ p.cls[p.at(s, c0)], p.reset[p.at(s, c0)], used[(size_t)s], 0, 1.0 };
            if (ps.cls == EqBypass::kFade) {
                ps.fadeLen = (int)std::min(f.size() - ps.fadeStart, n);
                // past the end of the ramp getNextValue keeps returning its final value; a ramp that drew nothing rests
                ps.fadeEnd = f.empty() ? p.fadeRest[(size_t)s] : f[std::min(f.size(), ps.fadeStart + n) - 1];
                used[(size_t)s] += (size_t)ps.fadeLen;
            }
            pc.streams.push_back(ps);
        }
        pieces.push_back(std::move(pc));
        c0 = c1;
    }
    return pieces;
}

// processor-level mix smoother (src/ConvolverProcessor.h:945; Runtime.cpp:340-375, 591-607); ramp.totalSteps is the
// smoothing time of the stream's parameters
struct MixRamp {
    LinearRamp ramp{ 1.0, 1.0, 0.0, 0, 4800 };

    // Start of a call of n samples in callbacks of B: the target follows the mix (:366-371); returns how many leading
    // samples are mixed with per-sample gains -- every callback that STARTS while the ramp runs, whole.  0: no smoothing.
    int beginCall(double mix, int n, int B)
    {
        if (std::fabs(ramp.target - mix) > 1.0e-5) ramp.setTargetValue(mix);
        if (!ramp.isSmoothing()) return 0;
        return (int)std::min<int64_t>(n, ((int64_t)ramp.remaining + B - 1) / B * B);
    }
    double next() { return ramp.getNextValue(); }
    // would beginCall smooth?  Answered by running it on a copy: nothing moves.
    bool wouldSmooth(double mix, int n, int B) const
    {
        MixRamp probe = *this;
        return probe.beginCall(mix, n, B) > 0;
    }
};

// latency compensation (Runtime.cpp:263-290, 394-540): latencySmoother is only ever snapped, crossfadeGain runs 20 ms
struct LatencyFade {
    double latCurrent = 0.0, latTarget = 0.0, oldDelay = 0.0;
    LinearRamp fade;
    bool primed = false;        // latCurrent holds the prepareToPlay value (Lifecycle.cpp:377-388)

    // prepareToPlay: latency + irLatency (MAX_IR_LATENCY 2^21, MAX_BLOCK_SIZE 524288), fade gain at 1
    void prime(int P0, int irPeakLatency)
    {
        latCurrent = latTarget = oldDelay = (double)std::min(P0 + std::min(std::max(0, irPeakLatency), 2097152), 2097152 + 524288);
        fade.setCurrentAndTargetValue(1.0);
        primed = true;
    }
    // Start of a callback with `total` samples of latency wanted: a move of >= 2 samples starts, unless one is running, a
    // cross-fade of xTotal steps from the delay in use (applyImmediateValueRT(0), setTargetValue(1)).  true: it started here.
    bool beginCallback(double total, int xTotal)
    {
        if (!(std::fabs(latTarget - total) >= 2.0) || fade.isSmoothing()) return false;
        oldDelay = latCurrent;
        fade.setCurrentAndTargetValue(0.0);
        fade.totalSteps = xTotal;
        fade.setTargetValue(1.0);
        latTarget = total;
        return true;
    }
    bool fading() const { return fade.isSmoothing(); }
    int newDelay() const { return fading() ? (int)latTarget : (int)(latCurrent + 0.5); }    // of the dry read at this point
    // the len samples of a callback: getNextValue until the ramp has ended, the values appended to vals unless it is null
    void advance(int len, std::vector<double>* vals)
    {
        if (!fade.isSmoothing()) return;
        for (int i = 0; i < len && fade.isSmoothing(); ++i) {
            const double v = fade.getNextValue();
            if (vals) vals->push_back(v);
        }
        if (!fade.isSmoothing()) { latCurrent = latTarget; oldDelay = latCurrent; }
    }
};

// ---- the processor-level stage's plan of one call of n samples, callbacks of B (the last one may be shorter), over S streams
// (engine_proc.cpp carries it out).  Per stream: bypass[s], dryOnly[s] (mix <= 0.001), mix[s] and irPeak[s] as last set.

// equalPowerSin, src/convolver/ConvolverProcessor.Runtime.cpp:26-31 (9th-order Taylor of sin(pi x / 2))
inline double equalPowerSin(double x)
{
    const double t = x * (3.141592653589793238462643383279502884 * 0.5);
    const double t2 = t * t;
    return t * (1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 + t2 * (-1.0 / 5040.0 + t2 * (1.0 / 362880.0)))));
}
// the gains of a mix at rest (targetMixValue, the float widened, :366)
struct MixGains { double wet, dry; };
inline MixGains staticMixGains(double mix)
{
    // !needsConvolution (:374, :573-585): the delayed dry signal is copied as it is -- matters when the convolver still runs
    // because a mix ramp is finishing in the same call
    if (!(mix > 0.001)) return { 0.0, 1.0 };
    return { equalPowerSin(mix) * 1.0,                              // * CONVOLUTION_HEADROOM_GAIN
             (mix < 0.999) ? equalPowerSin(1.0 - mix) : 0.0 };      // needsDrySignal, :375, :676
}
// the dry signal's delay: algorithmLatency = conv->latency = the layer-0 partition P0, 0 with the direct head (:266), plus
// irPeakLatency, clamped like :266-277 (MAX_BLOCK_SIZE 524288, MAX_IR_LATENCY 2^21)
inline int procDelay(bool directHead, int P0, int irPeakLatency)
{
    const int alg = directHead ? 0 : std::min(P0, 524288);
    const int peak = std::min(std::max(0, irPeakLatency), 2097152);
    return alg + peak;
}

// Whose convolver rests in this call: needsConvolution = isSmoothing || mix > 0.001 (:374); bypassed: the convolver is not called
// (:123-186).  A dry-only stream keeps convolving while its mix ramp runs, so streams set dry-only together can still differ for
// a call or two when their ramps have different lengths left.  Nothing moves here: the answer is what planProcMix will decide.
struct ProcRest {
    std::vector<char> rest;             // [S]
    bool allRest = true, anyRest = false;
};
inline ProcRest planProcRest(const MixRamp* ramps, const char* bypass, const char* dryOnly, const double* mix, int S, int n, int B)
{
    ProcRest r;
    r.rest.assign((size_t)S, 0);
    for (int s = 0; s < S; ++s) {
        r.rest[(size_t)s] = bypass[s] || (dryOnly[s] && !ramps[s].wouldSmooth(mix[s], n, B));
        r.allRest = r.allRest && r.rest[(size_t)s];
        r.anyRest = r.anyRest || r.rest[(size_t)s];
    }
    return r;
}

// Mix smoothing: per callback the reference moves the ramp's target to the current mix (:366-371) and, while the ramp is running
// at the START of a callback, mixes that whole callback with per-sample gains equalPowerSin(getNextValue()) (:591-607).
// Parameters only change between calls, so the smoothed region is a prefix of the call.
struct ProcMixPlan {
    bool anyRamp = false;
    int rampStride = 0;                 // samples per stream in gains: the longest smoothed prefix
    std::vector<int> len;               // [S] smoothed prefix per stream; empty while nothing ramps
    std::vector<double> gains;          // [S][rampStride][2] wet, dry per sample; zero behind a stream's prefix
};
// steps the ramps of the streams that are not bypassed (the bypass path does not touch the smoother, :123-186); a call in which
// nothing ramps allocates nothing
inline ProcMixPlan planProcMix(MixRamp* ramps, const char* bypass, const double* mix, int S, int n, int B)
{
    ProcMixPlan p;
    for (int s = 0; s < S; ++s) {
        if (bypass[s]) continue;
        const int len = ramps[s].beginCall(mix[s], n, B);
        if (len <= 0) continue;
        if (!p.anyRamp) { p.len.assign((size_t)S, 0); p.anyRamp = true; }
        p.len[(size_t)s] = len;
        p.rampStride = std::max(p.rampStride, len);
    }
    if (p.anyRamp) p.gains.assign((size_t)S * p.rampStride * 2, 0.0);
    for (int s = 0; s < S && p.anyRamp; ++s)
        for (int i = 0; i < p.len[(size_t)s]; ++i) {
            const double m = ramps[s].next();
            p.gains[((size_t)s * p.rampStride + i) * 2] = equalPowerSin(m) * 1.0;
            p.gains[((size_t)s * p.rampStride + i) * 2 + 1] = equalPowerSin(1.0 - m);
        }
    return p;
}

// Latency compensation per callback and stream (:263-290): a total latency that moved by >= 2 samples starts, unless one is
// running, a 20 ms cross-fade of the dry read from the delay in use to the new one; the callbacks that start while it runs blend
// sample by sample until the ramp ends (:394-540).  The bypass reads at the present latency (:141-145) and leaves the fade alone.
// The call is cut into ranges of callbacks [c0, c1) at the callbacks t > 0 where some stream starts a fade: one launch each.
struct ProcLatRange {
    int c0 = 0, c1 = 0;
    std::vector<int> dNew, dOld, xLen;  // [S] delay read, delay faded out, leading samples of the range with a gain of their own
    std::vector<double> gains;          // [S][xStride], zero behind xLen[s]; empty while no stream fades in the range
    bool fade() const { return !gains.empty(); }
};
struct ProcLatPlan {
    int xStride = 0;                    // xTotal + B: no range draws more (a fade ends inside a callback at the latest)
    std::vector<ProcLatRange> ranges;
    bool anyFade = false;               // a fade of ONE value (a one-sample call) counts
};
// steps the fades of the streams that are not bypassed, each (stream, callback) once: what the callback's start showed and how
// many values it drew are kept per stream, and the ranges are cut from that record.  reprime: the first call since prepare
// primes every fade anew.
inline ProcLatPlan planProcLatency(LatencyFade* fades, const char* bypass, const int* irPeak, int S, bool directHead, int P0,
                                   bool reprime, int n, int B, int xTotal)
{
    const int cbs = (n + B - 1) / B;
    struct Seen { int dNew, dOld; size_t drawn; };      // at the callback's start; values of the stream drawn in front of it
    std::vector<Seen> seen((size_t)S * cbs);
    std::vector<std::vector<double>> vals((size_t)S);
    std::vector<char> starts((size_t)cbs, 0);
    for (int s = 0; s < S; ++s) {
        const int total = procDelay(directHead, P0, irPeak[s]);
        if (bypass[s]) {
            for (int t = 0; t < cbs; ++t) seen[(size_t)s * cbs + t] = { total, total, 0 };
            continue;
        }
        LatencyFade& f = fades[s];
        if (!f.primed || reprime) f.prime(P0, irPeak[s]);
        for (int t = 0; t < cbs; ++t) {
            if (f.beginCallback((double)total, xTotal) && t > 0) starts[(size_t)t] = 1;
            seen[(size_t)s * cbs + t] = { f.newDelay(), (int)f.oldDelay, vals[(size_t)s].size() };
            f.advance(std::min(B, n - t * B), &vals[(size_t)s]);
        }
    }
    ProcLatPlan p;
    p.xStride = xTotal + B;
    for (int c0 = 0, t = 1; t <= cbs; ++t) {
        if (t != cbs && !starts[(size_t)t]) continue;
        ProcLatRange r;
        r.c0 = c0; r.c1 = t;
        r.dNew.resize((size_t)S); r.dOld.resize((size_t)S); r.xLen.resize((size_t)S);
        for (int s = 0; s < S; ++s) {
            const Seen& at = seen[(size_t)s * cbs + c0];
            const size_t end = t < cbs ? seen[(size_t)s * cbs + t].drawn : vals[(size_t)s].size();
            r.dNew[(size_t)s] = at.dNew;
            r.dOld[(size_t)s] = at.dOld;
            r.xLen[(size_t)s] = (int)(end - at.drawn);
            if (end == at.drawn) continue;
            if (r.gains.empty()) r.gains.assign((size_t)S * p.xStride, 0.0);
            std::copy(vals[(size_t)s].begin() + (std::ptrdiff_t)at.drawn, vals[(size_t)s].begin() + (std::ptrdiff_t)end,
                      r.gains.begin() + (std::ptrdiff_t)((size_t)s * p.xStride));
        }
        p.anyFade = p.anyFade || r.fade();
        p.ranges.push_back(std::move(r));
        c0 = t;
    }
    return p;
}

}  // namespace cpqi
