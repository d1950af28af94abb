// host_replay.hpp -- the reference's per-stream ramps and fades, replayed on the host once per callback before any kernel
// is launched.  All four are its LinearRamp (src/DspNumericPolicy.h:319-421) with a little policy on top:
//   GainRamp     smoothTotalGain, 50 ms: setTargetValue + skip(B) per callback         (engine_eq.cpp::enqueueEqCore)
//   EqBypass     bypassFadeGain, 5 ms: requested / effective / released per callback   (engine_eq.cpp::enqueueEqRange)
//   MixRamp      mixSmoother: getNextValue per sample over a prefix of the call        (engine_proc.cpp::enqueueConvProc)
//   LatencyFade  crossfadeGain, 20 ms, between the delay in use and the new one        (engine_proc.cpp::enqueueConvProc)
// Plain integer and double arithmetic, operation for operation the reference's; no HIP, no engine: a stepper returns plain
// data and the caller turns it into uploads and launches.  Whatever has to be known BEFORE state may move (which convolvers
// rest in a call, where latency fades start) is found by running the same steppers on a copy.
// tests/sanitize/host_replay_check.cpp drives this header alone, on the CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
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

}  // namespace cpqi
