// Host-only driver for convopeq_amd/csrc/host_replay.hpp (tests/test_host_replay_cpu.py): the ramps and fades the engine replays
// per callback, with no HIP and no engine.  Every check is exact (== on doubles): the properties hold bit for bit by construction.
//   1. LinearRamp semantics
//   2. call-split invariance: N callbacks as one call, as every split into two calls and as N calls give the same outputs and
//      leave the same state (the reference only ever sees callbacks, so it has this by construction)
//   3. what is predicted before state may move (which convolver rests) is what the plan then decides, and the prediction moved
//      nothing
//   4. the EQ's plan of a call (planEqGain, planEqCall, needsSilence, assignResets, cutPieces -- the planners engine_eq.cpp
//      itself calls): invariant under the cut into calls for several streams at once, its pieces tile the call, and the fade end
//      value of a piece in hand-written cases
//   5. the processor-level stage's plan of a call (planProcRest, planProcMix, planProcLatency -- the planners engine_proc.cpp
//      itself calls) and its arithmetic (equalPowerSin, staticMixGains, procDelay): the same properties, the shape of the gain
//      tables and of the latency ranges in hand-written cases
#include "host_replay.hpp"

#include <cstdio>

using namespace cpqi;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

struct Rng {        // seeded, the same everywhere
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    double unit() { return (double)next() / 2147483648.0; }
};

static bool same(const LinearRamp& a, const LinearRamp& b)
{
    return a.current == b.current && a.target == b.target && a.step == b.step && a.remaining == b.remaining && a.totalSteps == b.totalSteps;
}
static bool same(const GainRamp& a, const GainRamp& b) { return same(a.ramp, b.ramp) && a.wanted == b.wanted && a.devUnity == b.devUnity; }
static bool same(const EqBypass& a, const EqBypass& b)
{
    return same(a.fade, b.fade) && a.requested == b.requested && a.effective == b.effective && a.mode == b.mode;
}
static bool same(const MixRamp& a, const MixRamp& b) { return same(a.ramp, b.ramp); }
static bool same(const LatencyFade& a, const LatencyFade& b)
{
    return same(a.fade, b.fade) && a.latCurrent == b.latCurrent && a.latTarget == b.latTarget && a.oldDelay == b.oldDelay && a.primed == b.primed;
}

// ---------------------------------------------------------------------------------------------------- per-call drivers
struct Shape { int B; double rate; };

struct GainOut { double start, increment; bool operator==(const GainOut&) const = default; };
// planEqGain: a stream that is not moving at the start of the call draws nothing (the cascade kernel applies `wanted`)
static void gainCall(GainRamp& r, const Shape& sh, int cbs, std::vector<GainOut>& out)
{
    const int agcOff = 0;
    const GainRamp before = r;
    const bool predicted = anyGainRamp(&r, &agcOff, nullptr, 1);
    CHECK(same(before, r));                                     // the prediction moved nothing
    const EqGainPlan g = planEqGain(&r, &agcOff, nullptr, 1, cbs, sh.B, LinearRamp::stepsFor(sh.rate, 0.05));
    CHECK(predicted == g.anyRamp);
    // the device gain flips exactly when it has to (devUnity is the engine's to set: it stays false here)
    CHECK(g.flips.size() == (g.anyRamp ? 1u : 0u));
    if (g.anyRamp) CHECK(g.flips[0].s == 0 && g.flips[0].unity && g.flips[0].gain == 1.0 && g.rampOn[0] == 1);
    if (!g.anyRamp) { CHECK(g.segments.empty() && g.rampOn.empty()); out.insert(out.end(), (size_t)cbs, GainOut{ r.wanted, 0.0 }); return; }
    CHECK(g.segments.size() == (size_t)cbs * 2);
    for (int t = 0; t < cbs; ++t) out.push_back({ g.segments[(size_t)t * 2], g.segments[(size_t)t * 2 + 1] });
}

struct BypassOut {
    std::vector<char> cls, released;
    std::vector<double> vals;
    bool operator==(const BypassOut&) const = default;
};
static void bypassCall(EqBypass& b, const Shape& sh, int cbs, BypassOut& out)
{
    const EqCallPlan p = planEqCall(&b, 1, cbs, sh.B, LinearRamp::stepsFor(sh.rate, 0.005));
    out.cls.insert(out.cls.end(), p.cls.begin(), p.cls.end());
    out.released.insert(out.released.end(), p.released.begin(), p.released.end());
    out.vals.insert(out.vals.end(), p.fade[0].begin(), p.fade[0].end());
    CHECK(p.fadeRest[0] == b.fade.current);
}

// The whole EQ plan of a call over several streams, as enqueueEqRange runs the planners.  silent: the script's flag per
// (stream, callback of the stretch), the same however the stretch is cut; pos: callbacks of the stretch already played.
struct EqState { std::vector<EqBypass> byp; std::vector<uint32_t> pending; int pos; };
static bool same(const EqState& a, const EqState& b)
{
    if (a.byp.size() != b.byp.size() || a.pending != b.pending || a.pos != b.pos) return false;
    for (size_t s = 0; s < a.byp.size(); ++s)
        if (!same(a.byp[s], b.byp[s])) return false;
    return true;
}
struct EqOut {
    std::vector<char> cls;              // per (callback, stream)
    std::vector<uint32_t> reset;        // per (callback, stream)
    std::vector<double> gain;           // per (callback, stream, sample): the cross-fade gain, 1 = EQ alone, kPass: 0
    std::vector<uint32_t> left;         // masks still pending behind the last call
    bool operator==(const EqOut&) const = default;
};
struct EqSaw {
    bool resetByFade = false, resetBySilence = false, pendingLeft = false, releaseClears = false, noSilenceAsked = false,
         cutByResetAlone = false, cutByOneStream = false;
};
static void checkPieces(const EqCallPlan& p, const std::vector<EqPiece>& pieces, EqSaw& saw)
{
    int at = 0;
    for (const EqPiece& pc : pieces) {
        CHECK(pc.c0 == at && pc.c1 > pc.c0 && pc.c1 <= p.cbs && (int)pc.streams.size() == p.S);     // contiguous, not empty
        for (int s = 0; s < p.S; ++s) {
            const EqPiece::Stream& ps = pc.streams[(size_t)s];
            CHECK(ps.reset == p.reset[p.at(s, pc.c0)]);
            for (int t = pc.c0; t < pc.c1; ++t) {
                CHECK(p.cls[p.at(s, t)] == ps.cls);                         // one class per stream
                CHECK(t == pc.c0 || p.reset[p.at(s, t)] == 0u);             // a reset only in front
            }
            CHECK(ps.fadeLen >= 0 && ps.fadeLen <= (pc.c1 - pc.c0) * p.B && ps.fadeStart + (size_t)ps.fadeLen <= p.fade[(size_t)s].size());
            CHECK(ps.cls == EqBypass::kFade || (ps.fadeLen == 0 && ps.fadeEnd == 1.0));
        }
        if (pc.c1 < p.cbs) {            // maximal: the cut has a reason, in some stream
            int byClass = 0, byReset = 0, streams = 0;
            for (int s = 0; s < p.S; ++s) {
                const bool c = p.cls[p.at(s, pc.c1)] != p.cls[p.at(s, pc.c0)], r = p.reset[p.at(s, pc.c1)] != 0u;
                byClass += c; byReset += r; streams += c || r;
            }
            CHECK(streams > 0);
            saw.cutByResetAlone = saw.cutByResetAlone || (byClass == 0 && byReset > 0);
            saw.cutByOneStream = saw.cutByOneStream || (streams == 1 && p.S > 1);
        }
        at = pc.c1;
    }
    CHECK(at == p.cbs);                 // ... and they cover the call
}
static void eqCall(EqState& st, const Shape& sh, int cbs, const std::vector<std::vector<int>>& silent, EqOut& out, EqSaw& saw)
{
    const int S = (int)st.byp.size();
    const std::vector<uint32_t> before = st.pending;
    EqCallPlan p = planEqCall(st.byp.data(), S, cbs, sh.B, LinearRamp::stepsFor(sh.rate, 0.005));
    const bool ask = needsSilence(p, st.pending.data());
    std::vector<int> flags((size_t)S * cbs);
    for (int s = 0; s < S; ++s)
        for (int t = 0; t < cbs; ++t) flags[p.at(s, t)] = silent[(size_t)s][(size_t)(st.pos + t)];
    const bool left = assignResets(p, st.pending.data(), ask ? flags.data() : nullptr);     // no flags unless asked for, as in the engine
    bool anyLeft = false;
    for (uint32_t m : st.pending) anyLeft = anyLeft || m != 0u;
    CHECK(left == anyLeft);
    saw.pendingLeft = saw.pendingLeft || left;
    const std::vector<EqPiece> pieces = cutPieces(p);
    checkPieces(p, pieces, saw);
    std::vector<double> gain((size_t)S * cbs * sh.B, 0.0);
    for (const EqPiece& pc : pieces)
        for (int s = 0; s < S; ++s) {
            const EqPiece::Stream& ps = pc.streams[(size_t)s];
            for (int i = 0; i < (pc.c1 - pc.c0) * sh.B; ++i) {
                double g = ps.cls == EqBypass::kNormal ? 1.0 : 0.0;
                if (ps.cls == EqBypass::kFade) g = i < ps.fadeLen ? p.fade[(size_t)s][ps.fadeStart + (size_t)i] : ps.fadeEnd;
                gain[((size_t)s * cbs + pc.c0) * sh.B + (size_t)i] = g;
            }
        }
    for (int s = 0; s < S; ++s) {
        bool fadeFirst = false;
        for (int t = 0; t < cbs && !fadeFirst && p.cls[p.at(s, t)] != EqBypass::kNormal; ++t) fadeFirst = p.cls[p.at(s, t)] == EqBypass::kFade;
        saw.noSilenceAsked = saw.noSilenceAsked || (!ask && before[(size_t)s] != 0u && fadeFirst);
        for (int t = 0; t < cbs; ++t) {
            const uint32_t m = p.reset[p.at(s, t)];
            const char k = p.cls[p.at(s, t)];
            CHECK(m == 0u || k != EqBypass::kPass);
            saw.resetByFade = saw.resetByFade || (m != 0u && k == EqBypass::kFade && !p.released[p.at(s, t)]);
            saw.resetBySilence = saw.resetBySilence || (m != 0u && k == EqBypass::kNormal);
            if (p.released[p.at(s, t)]) { CHECK(m == 0xFFFFFFFFu && k == EqBypass::kFade); saw.releaseClears = true; }
        }
    }
    for (int t = 0; t < cbs; ++t)
        for (int s = 0; s < S; ++s) {
            out.cls.push_back(p.cls[p.at(s, t)]);
            out.reset.push_back(p.reset[p.at(s, t)]);
            out.gain.insert(out.gain.end(), gain.begin() + (long)(p.at(s, t) * sh.B), gain.begin() + (long)((p.at(s, t) + 1) * sh.B));
        }
    out.left = st.pending;
    st.pos += cbs;
}

// planProcRest + planProcMix of one stream: the gain pair of every sample -- the plan's over the smoothed prefix, behind it the
// pair of the value the ramp rests at
struct MixState { MixRamp r; double mix; };
static bool same(const MixState& a, const MixState& b) { return same(a.r, b.r) && a.mix == b.mix; }
static void mixCall(MixState& m, const Shape& sh, int n, std::vector<double>& out)
{
    const char bypass = 0, dryOnly = !(m.mix > 0.001);
    const MixRamp before = m.r;
    const ProcRest rest = planProcRest(&m.r, &bypass, &dryOnly, &m.mix, 1, n, sh.B);
    CHECK(same(before, m.r));                                   // the prediction moved nothing
    const ProcMixPlan p = planProcMix(&m.r, &bypass, &m.mix, 1, n, sh.B);
    CHECK((rest.rest[0] != 0) == (dryOnly && !p.anyRamp));      // ... and is what the ramps decide once they have moved
    CHECK(rest.allRest == (rest.rest[0] != 0) && rest.anyRest == rest.allRest);
    const int len = p.anyRamp ? p.len[0] : 0;
    CHECK(p.anyRamp == (len > 0) && p.rampStride == len && p.gains.size() == (size_t)len * 2 && (p.anyRamp || p.len.empty()));
    CHECK(len <= n && (len == n || len % sh.B == 0));
    out.insert(out.end(), p.gains.begin(), p.gains.end());
    if (len < n) CHECK(!m.r.ramp.isSmoothing());                // the prefix covers the whole ramp or the whole call
    for (int i = len; i < n; ++i) { out.push_back(equalPowerSin(m.r.ramp.current) * 1.0); out.push_back(equalPowerSin(1.0 - m.r.ramp.current)); }
}

// planProcLatency of one stream: per sample the delay read, the delay faded out (-1: none) and the fade gain
struct LatState { LatencyFade f; bool processed; int irPeak; };
static bool same(const LatState& a, const LatState& b) { return same(a.f, b.f) && a.processed == b.processed && a.irPeak == b.irPeak; }
struct LatSample { int dNew, dOld; double g; bool operator==(const LatSample&) const = default; };
constexpr int kP0 = 64;
// what every plan shows: the ranges tile the call, a range behind the first begins where some stream starts a fade (its first
// value is one step of xTotal) and no fade starts inside a range (the values of a row only rise)
static void checkRanges(const ProcLatPlan& p, int S, int n, int B, int xTotal)
{
    const int cbs = (n + B - 1) / B;
    int at = 0;
    bool any = false;
    CHECK(p.xStride == xTotal + B && !p.ranges.empty());
    for (size_t r = 0; r < p.ranges.size(); ++r) {
        const ProcLatRange& g = p.ranges[r];
        const int len = std::min(g.c1 * B, n) - g.c0 * B;
        CHECK(g.c0 == at && g.c1 > g.c0 && g.c1 <= cbs && (int)g.dNew.size() == S && (int)g.dOld.size() == S && (int)g.xLen.size() == S);
        CHECK(g.gains.empty() || g.gains.size() == (size_t)S * p.xStride);
        bool starts = false, draws = false;
        for (int s = 0; s < S; ++s) {
            const int x = g.xLen[(size_t)s];
            CHECK(x >= 0 && x <= len && x <= xTotal);
            CHECK(x == 0 || g.fade());
            draws = draws || x > 0;
            if (!g.fade()) continue;
            const double* row = &g.gains[(size_t)s * p.xStride];
            starts = starts || (x > 0 && row[0] == 1.0 / (double)xTotal);
            for (int i = 1; i < x; ++i) CHECK(row[i] > row[i - 1]);
            for (int i = x; i < p.xStride; ++i) CHECK(row[i] == 0.0);
        }
        CHECK(draws == g.fade());
        CHECK(r == 0 || starts);
        any = any || g.fade();
        at = g.c1;
    }
    CHECK(at == cbs && any == p.anyFade);
}
static void latCall(LatState& st, const Shape& sh, int n, std::vector<LatSample>& out)
{
    const int xTotal = LinearRamp::stepsFor(sh.rate, 0.02);
    const bool firstCall = !st.processed;
    st.processed = true;
    const char bypass = 0;
    const ProcLatPlan p = planProcLatency(&st.f, &bypass, &st.irPeak, 1, false, kP0, firstCall, n, sh.B, xTotal);
    checkRanges(p, 1, n, sh.B, xTotal);
    for (const ProcLatRange& r : p.ranges) {
        const int len = std::min(r.c1 * sh.B, n) - r.c0 * sh.B;
        for (int i = 0; i < len; ++i)
            out.push_back(i < r.xLen[0] ? LatSample{ r.dNew[0], r.dOld[0], r.gains[(size_t)i] } : LatSample{ r.dNew[0], -1, 1.0 });
    }
}

// One stretch of callbacks (lens: B, ..., B and possibly a shorter last one) from state s0: as one call, as every split into two
// calls, as one call per callback.  Returns the state behind it.
template <class State, class Out, class Call>
static State splitInvariant(const State& s0, const std::vector<int>& lens, bool bySamples, Call call, Out& whole)
{
    const int N = (int)lens.size();
    auto size = [&](int a, int b) { int n = 0; for (int t = a; t < b; ++t) n += bySamples ? lens[(size_t)t] : 1; return n; };
    State end = s0;
    call(end, size(0, N), whole);
    for (int k = 1; k < N; ++k) {
        State s = s0;
        Out o;
        call(s, size(0, k), o);
        call(s, size(k, N), o);
        CHECK(o == whole);
        CHECK(same(s, end));
    }
    State s = s0;
    Out o;
    for (int t = 0; t < N; ++t) call(s, size(t, t + 1), o);
    CHECK(o == whole);
    CHECK(same(s, end));
    return end;
}

static void rampSemantics()
{
    for (double rate : { 44100.0, 48000.0, 384000.0 })
        for (double t : { 0.005, 0.02, 0.05, 0.1 }) {
            const int n = LinearRamp::stepsFor(rate, t);
            CHECK(n >= 1 && n == (int)(rate * t + 0.5));
        }
    CHECK(LinearRamp::stepsFor(44100.0, 0.005) == 221 && LinearRamp::stepsFor(44100.0, 0.02) == 882 && LinearRamp::stepsFor(44100.0, 0.05) == 2205);
    CHECK(LinearRamp::stepsFor(48000.0, 0.005) == 240 && LinearRamp::stepsFor(48000.0, 0.1) == 4800 && LinearRamp::stepsFor(384000.0, 0.05) == 19200);
    CHECK(LinearRamp::stepsFor(48000.0, 0.0) == 1 && LinearRamp::stepsFor(1.0, 0.005) == 1 && LinearRamp::stepsFor(48000.0, -1.0) == 1);

    LinearRamp r;
    CHECK(r.current == 1.0 && r.target == 1.0 && !r.isSmoothing());
    r.totalSteps = 10;
    r.setTargetValue(1.0);                                      // the target it has: nothing happens
    CHECK(!r.isSmoothing() && r.step == 0.0 && r.getNextValue() == 1.0);
    r.setTargetValue(0.3);
    CHECK(r.isSmoothing() && r.remaining == 10 && r.step == (0.3 - 1.0) / 10.0);
    { const LinearRamp was = r; r.setTargetValue(0.3); CHECK(same(was, r)); }
    double c = 1.0;
    for (int i = 0; i < 4; ++i) { c += r.step; CHECK(r.getNextValue() == c); }
    r.setTargetValue(0.9);                                      // in mid-ramp: the 6 steps left, not 10
    CHECK(r.remaining == 6 && r.step == (0.9 - c) / 6.0);
    for (int i = 0; i < 5; ++i) { c += r.step; CHECK(r.getNextValue() == c); }
    CHECK(r.remaining == 1 && r.current != 0.9);                // accumulated rounding: not there yet ...
    CHECK(r.getNextValue() == 0.9 && !r.isSmoothing());         // ... the last step lands on the target itself
    CHECK(r.getNextValue() == 0.9 && r.current == 0.9);         // at rest it keeps returning it

    r.setCurrentAndTargetValue(0.1);
    r.totalSteps = 7;
    r.setTargetValue(0.7);
    {   // skip(n), n < remaining: one multiply-add -- and that is NOT n additions (0.1 -> 0.7 in 7 steps tells them apart)
        LinearRamp a = r, b = r;
        a.skip(5);
        CHECK(a.current == 0.1 + a.step * 5.0 && a.remaining == 2 && a.isSmoothing());
        for (int i = 0; i < 5; ++i) b.getNextValue();
        CHECK(b.remaining == 2 && b.current != a.current);
        a.skip(0); a.skip(-3);
        CHECK(a.current == 0.1 + a.step * 5.0 && a.remaining == 2);
        a.skip(2);                                              // n == remaining: snaps
        CHECK(a.current == 0.7 && !a.isSmoothing());
        LinearRamp d = r;
        d.skip(1000);
        CHECK(d.current == 0.7 && d.remaining == 0);
        d.skip(3);
        CHECK(d.current == 0.7);
    }
    r.setCurrentAndTargetValue(0.25);
    CHECK(r.current == 0.25 && r.target == 0.25 && r.step == 0.0 && r.remaining == 0 && r.totalSteps == 7);
}

static std::vector<int> callbacks(Rng& rng, int B, bool ragged)
{
    std::vector<int> lens((size_t)(1 + rng.below(6)), B);
    if (ragged && rng.below(2)) lens.push_back(1 + rng.below(B - 1));
    return lens;
}

static void splitScripts()
{
    const Shape shapes[3] = { { 64, 48000.0 }, { 441, 44100.0 }, { 512, 48000.0 } };
    const double gainsOf[6] = { 1.0, 0.5, 2.0, 0.5 + 1.0e-7, 0.25, 1.0 + 5.0e-7 };
    const int peaks[5] = { 0, 150, 151, 900, 3000 };
    for (const Shape& sh : shapes)
        for (uint64_t seed = 1; seed <= 6; ++seed) {
            Rng rng{ seed * 7919u + (uint64_t)sh.B };
            GainRamp gain;
            EqBypass byp;
            MixState mix{ MixRamp{}, 1.0 };
            mix.r.ramp.totalSteps = LinearRamp::stepsFor(sh.rate, seed % 2 ? 0.1 : 0.01);
            LatState lat{ LatencyFade{}, false, 0 };
            bool sawFade = false, sawPass = false, sawRelease = false, sawLatFade = false, sawMixRamp = false, sawGainRamp = false;
            for (int seg = 0; seg < 60; ++seg) {
                // parameters change between calls only
                if (rng.below(3) == 0) gain.wanted = rng.below(4) ? gainsOf[rng.below(6)] : 0.1 + rng.unit();
                if (rng.below(4) == 0) byp.requested = !byp.requested;
                if (rng.below(3) == 0) mix.mix = rng.below(3) ? (double)(float)rng.unit() : (rng.below(2) ? 0.0 : mix.mix + 5.0e-6);
                if (rng.below(3) == 0) lat.irPeak = peaks[rng.below(5)];
                const std::vector<int> whole = callbacks(rng, sh.B, false), ragged = callbacks(rng, sh.B, true);

                std::vector<GainOut> go;
                gain = splitInvariant(gain, whole, false, [&](GainRamp& r, int cbs, std::vector<GainOut>& o) { gainCall(r, sh, cbs, o); }, go);
                for (const auto& g : go) sawGainRamp = sawGainRamp || g.increment != 0.0;
                BypassOut bo;
                byp = splitInvariant(byp, whole, false, [&](EqBypass& b, int cbs, BypassOut& o) { bypassCall(b, sh, cbs, o); }, bo);
                sawFade = sawFade || !bo.vals.empty();
                for (size_t t = 0; t < bo.cls.size(); ++t) { sawPass = sawPass || bo.cls[t] == EqBypass::kPass; sawRelease = sawRelease || bo.released[t]; }
                CHECK(byp.active() == (byp.requested || byp.effective || byp.fade.isSmoothing()));
                std::vector<double> mo;
                mix = splitInvariant(mix, ragged, true, [&](MixState& m, int n, std::vector<double>& o) { mixCall(m, sh, n, o); }, mo);
                for (size_t i = 0; i < mo.size(); i += 2) sawMixRamp = sawMixRamp || mo[i] != mo[mo.size() - 2];
                std::vector<LatSample> lo;
                lat = splitInvariant(lat, ragged, true, [&](LatState& l, int n, std::vector<LatSample>& o) { latCall(l, sh, n, o); }, lo);
                for (const auto& v : lo) sawLatFade = sawLatFade || v.dOld >= 0;
            }
            CHECK(sawFade && sawPass && sawRelease && sawLatFade && sawMixRamp && sawGainRamp);   // the scripts reach every machine
        }
}

// 2 or 3 streams whose bypass requests and band resets change between stretches, each stream on its own; the silence flags are
// scripted per (stream, callback) of the stretch
static void eqPlanScripts()
{
    const Shape shapes[3] = { { 64, 48000.0 }, { 441, 44100.0 }, { 512, 48000.0 } };
    for (const Shape& sh : shapes) {
        EqSaw saw;
        for (uint64_t seed = 1; seed <= 6; ++seed) {
            Rng rng{ seed * 104729u + (uint64_t)sh.B };
            const int S = 2 + (int)(seed % 2);
            EqState st{ std::vector<EqBypass>((size_t)S), std::vector<uint32_t>((size_t)S, 0u), 0 };
            for (int seg = 0; seg < 120; ++seg) {
                for (int s = 0; s < S; ++s) {
                    if (rng.below(5) == 0) st.byp[(size_t)s].requested = !st.byp[(size_t)s].requested;
                    if (rng.below(4) == 0) st.pending[(size_t)s] |= rng.below(8) ? (1u << rng.below(20)) | (1u << rng.below(20)) : 0xFFFFFFFFu;
                }
                const std::vector<int> lens = callbacks(rng, sh.B, false);
                std::vector<std::vector<int>> silent((size_t)S, std::vector<int>(lens.size(), 0));
                for (auto& row : silent)
                    for (int& f : row) f = rng.below(4) == 0;
                st.pos = 0;
                EqOut eo;
                st = splitInvariant(st, lens, false, [&](EqState& q, int cbs, EqOut& o) { eqCall(q, sh, cbs, silent, o, saw); }, eo);
                CHECK(eo.cls.size() == lens.size() * (size_t)S && eo.gain.size() == eo.cls.size() * (size_t)sh.B && st.pos == (int)lens.size());
            }
        }
        CHECK(saw.resetByFade && saw.resetBySilence && saw.pendingLeft && saw.releaseClears && saw.noSilenceAsked);
        CHECK(saw.cutByResetAlone && saw.cutByOneStream);           // the scripts reach every way a reset is taken and a call is cut
    }
}

// the fade end value of a piece, by hand
static void fadeEndValues()
{
    {   // 48 kHz, B = 64: the fade-out of 240 steps ends inside its piece of 4 callbacks; the pass-through piece follows
        EqBypass b;
        b.requested = true;
        const EqCallPlan p = planEqCall(&b, 1, 6, 64, LinearRamp::stepsFor(48000.0, 0.005));
        const std::vector<EqPiece> pieces = cutPieces(p);
        CHECK(pieces.size() == 2 && pieces[0].c0 == 0 && pieces[0].c1 == 4 && pieces[1].c1 == 6 && p.fade[0].size() == 240);
        const EqPiece::Stream& f = pieces[0].streams[0];
        CHECK(f.cls == EqBypass::kFade && f.fadeStart == 0 && f.fadeLen == 240 && f.fadeEnd == 0.0 && f.fadeEnd == p.fade[0][239]);
        CHECK(pieces[1].streams[0].cls == EqBypass::kPass && pieces[1].streams[0].fadeLen == 0 && pieces[1].streams[0].fadeEnd == 1.0);
    }
    {   // 51.2 kHz: 256 steps end exactly with the piece's fourth callback
        EqBypass b;
        b.requested = true;
        CHECK(LinearRamp::stepsFor(51200.0, 0.005) == 256);
        const EqCallPlan p = planEqCall(&b, 1, 5, 64, 256);
        const std::vector<EqPiece> pieces = cutPieces(p);
        CHECK(pieces.size() == 2 && pieces[0].c1 == 4 && p.fade[0].size() == 256);
        const EqPiece::Stream& f = pieces[0].streams[0];
        CHECK(f.fadeLen == 256 && f.fadeEnd == 0.0 && p.fade[0][254] != 0.0 && p.fade[0][255] == 0.0);
    }
    {   // a second stream cuts the fade in two pieces: the first ends at the value of its last sample, the second starts behind it
        EqBypass b[2];
        b[0].requested = true;
        b[1].requested = true; b[1].sync();                     // stream 1 passes through; its class is changed by hand
        EqCallPlan p = planEqCall(b, 2, 2, 64, 240);
        p.cls[p.at(1, 1)] = EqBypass::kNormal;
        const std::vector<EqPiece> pieces = cutPieces(p);
        CHECK(pieces.size() == 2 && pieces[0].c1 == 1 && p.fade[0].size() == 128);
        CHECK(pieces[0].streams[0].fadeLen == 64 && pieces[0].streams[0].fadeEnd == p.fade[0][63]);
        CHECK(pieces[1].streams[0].fadeStart == 64 && pieces[1].streams[0].fadeLen == 64 && pieces[1].streams[0].fadeEnd == p.fade[0][127]);
        CHECK(p.fade[0][127] != 0.0 && p.fadeRest[0] == p.fade[0][127]);
    }
    {   // a kFade piece whose ramp drew nothing ends where the fade rests
        EqCallPlan p;
        p.S = 1; p.cbs = 2; p.B = 64;
        p.cls.assign(2, EqBypass::kFade);
        p.released.assign(2, 0);
        p.reset.assign(2, 0u);
        p.fade.resize(1);
        p.fadeRest.assign(1, 0.25);
        const std::vector<EqPiece> pieces = cutPieces(p);
        CHECK(pieces.size() == 1 && pieces[0].c0 == 0 && pieces[0].c1 == 2);
        CHECK(pieces[0].streams[0].fadeLen == 0 && pieces[0].streams[0].fadeStart == 0 && pieces[0].streams[0].fadeEnd == 0.25);
    }
}

// test_latency_cross_fade_starting_in_a_one_sample_call: quantum 96, the latency moves just before a call of ONE sample
static void oneSampleFadeStart()
{
    const Shape sh{ 96, 48000.0 };
    LatState st{ LatencyFade{}, false, 700 };
    std::vector<LatSample> o;
    latCall(st, sh, 96 * 2, o);
    CHECK(o.size() == 192 && o[0] == (LatSample{ kP0 + 700, -1, 1.0 }) && !st.f.fading());
    st.irPeak = 150;
    o.clear();
    latCall(st, sh, 1, o);
    CHECK(o.size() == 1 && o[0] == (LatSample{ kP0 + 150, kP0 + 700, 1.0 / 960.0 }) && st.f.fade.remaining == 959);
    // ... and the same stretch in any cut: 1 + 288 + 2 samples as three calls or as callbacks of the quantum
    LatState a{ LatencyFade{}, false, 700 }, b = a;
    std::vector<LatSample> oa, ob;
    latCall(a, sh, 192, oa); latCall(b, sh, 192, ob);
    a.irPeak = b.irPeak = 150;
    for (int n : { 1, 288, 2 }) latCall(a, sh, n, oa);
    for (int n : { 96, 96, 96, 3 }) latCall(b, sh, n, ob);
    CHECK(oa == ob && same(a, b));
    {   // B = 64: the plan of such a call is one range of one faded sample, and the gain buffer is wanted for it
        LatencyFade f;
        const char bypass = 0;
        int peak = 700;
        planProcLatency(&f, &bypass, &peak, 1, false, kP0, true, 128, 64, 960);
        peak = 150;
        const ProcLatPlan p = planProcLatency(&f, &bypass, &peak, 1, false, kP0, false, 1, 64, 960);
        CHECK(p.ranges.size() == 1 && p.ranges[0].c0 == 0 && p.ranges[0].c1 == 1 && p.ranges[0].xLen[0] == 1 && p.anyFade);
        CHECK(p.ranges[0].fade() && p.ranges[0].gains[0] == 1.0 / 960.0 && p.ranges[0].dNew[0] == kP0 + 150 && p.ranges[0].dOld[0] == kP0 + 700);
    }
}

// the shape of a latency plan, by hand: 48 kHz, B = 64, the fade of 960 samples is 15 callbacks
static void latencyRanges()
{
    const int B = 64, xTotal = 960, S = 2;
    LatencyFade f[2];
    char bypass[2] = { 0, 0 };
    int peak[2] = { 0, 300 };
    ProcLatPlan p = planProcLatency(f, bypass, peak, S, false, kP0, true, 4 * B, B, xTotal);       // the first call primes: nothing fades
    CHECK(p.ranges.size() == 1 && !p.anyFade && !p.ranges[0].fade() && p.ranges[0].dNew == p.ranges[0].dOld);
    CHECK(p.ranges[0].dNew[0] == kP0 && p.ranges[0].dNew[1] == kP0 + 300 && f[0].primed && f[1].primed);
    peak[0] = 700;
    p = planProcLatency(f, bypass, peak, S, false, kP0, false, 4 * B, B, xTotal);                  // a fade starts at callback 0: one range
    checkRanges(p, S, 4 * B, B, xTotal);
    CHECK(p.ranges.size() == 1 && p.ranges[0].xLen[0] == 4 * B && p.ranges[0].xLen[1] == 0 && f[0].fade.remaining == xTotal - 4 * B);
    CHECK(p.ranges[0].dNew[0] == kP0 + 700 && p.ranges[0].dOld[0] == kP0);
    // the latency moves again while the fade runs, and stream 1 is bypassed with a move of its own waiting: the running fade
    // ends with callback 11 of the next call and the new one starts there, in mid-call -- two ranges, the second fading out the
    // delay the first faded in; the bypassed stream reads at its present latency in both and its fade is not touched
    peak[0] = 150; peak[1] = 20; bypass[1] = 1;
    const LatencyFade was = f[1];
    p = planProcLatency(f, bypass, peak, S, false, kP0, false, 32 * B, B, xTotal);
    checkRanges(p, S, 32 * B, B, xTotal);
    CHECK(p.ranges.size() == 2 && p.ranges[0].c1 == 11 && p.ranges[1].c0 == 11 && p.ranges[1].c1 == 32);
    CHECK(p.ranges[0].xLen[0] == 11 * B && p.ranges[1].xLen[0] == xTotal);
    CHECK(p.ranges[0].dNew[0] == kP0 + 700 && p.ranges[0].dOld[0] == kP0);
    CHECK(p.ranges[1].dNew[0] == kP0 + 150 && p.ranges[1].dOld[0] == p.ranges[0].dNew[0]);
    for (const ProcLatRange& r : p.ranges) CHECK(r.dNew[1] == kP0 + 20 && r.dOld[1] == r.dNew[1] && r.xLen[1] == 0);
    CHECK(same(was, f[1]) && !f[0].fading() && f[0].latCurrent == (double)(kP0 + 150));
    // with the direct head the algorithm's share of the delay is 0 while the priming still starts from P0 + irPeakLatency: the
    // first call fades from there
    LatencyFade d;
    const char on = 0;
    const int pk = 77;
    p = planProcLatency(&d, &on, &pk, 1, true, kP0, true, 2 * B, B, xTotal);
    CHECK(p.ranges.size() == 1 && p.ranges[0].dNew[0] == 77 && p.ranges[0].dOld[0] == kP0 + 77 && p.ranges[0].xLen[0] == 2 * B);
}

// the shape of a mix plan, by hand: B = 64, four streams -- a long ramp, a short one, one at rest, one bypassed with a new mix
static void mixPlanShape()
{
    const int B = 64, n = 10 * B, S = 4;
    MixRamp r[4];
    r[0].ramp.totalSteps = 480; r[1].ramp.totalSteps = 100; r[2].ramp.totalSteps = 480; r[3].ramp.totalSteps = 480;
    const char bypass[4] = { 0, 0, 0, 1 }, dryOnly[4] = { 0, 1, 0, 0 };
    const double mix[4] = { 0.25, 0.0, 1.0, 0.5 };
    const MixRamp was[4] = { r[0], r[1], r[2], r[3] };
    const ProcRest rest = planProcRest(r, bypass, dryOnly, mix, S, n, B);
    for (int s = 0; s < S; ++s) CHECK(same(was[s], r[s]));
    CHECK(!rest.rest[0] && !rest.rest[1] && !rest.rest[2] && rest.rest[3] && rest.anyRest && !rest.allRest);     // 1 is dry-only but ramps
    const ProcMixPlan p = planProcMix(r, bypass, mix, S, n, B);
    CHECK(p.anyRamp && p.len.size() == 4 && p.len[0] == 512 && p.len[1] == 128 && p.len[2] == 0 && p.len[3] == 0);
    CHECK(p.rampStride == 512 && p.gains.size() == (size_t)S * 512 * 2);       // the longest prefix
    for (int s = 0; s < S; ++s)
        for (int i = 0; i < p.rampStride; ++i) {
            const double wet = p.gains[((size_t)s * p.rampStride + i) * 2], dry = p.gains[((size_t)s * p.rampStride + i) * 2 + 1];
            if (i >= p.len[(size_t)s]) CHECK(wet == 0.0 && dry == 0.0);        // rows of streams that do not ramp, and behind a prefix
            else CHECK(wet > 0.0 || dry > 0.0);
        }
    CHECK(p.gains[(size_t)(479 * 2)] == equalPowerSin(0.25) * 1.0 && p.gains[(size_t)(479 * 2 + 1)] == equalPowerSin(1.0 - 0.25));
    CHECK(p.gains[(size_t)(480 * 2)] == p.gains[(size_t)(479 * 2)]);           // behind the ramp's end the prefix holds the target
    CHECK(same(was[2], r[2]) && same(was[3], r[3]) && !r[0].ramp.isSmoothing() && !r[1].ramp.isSmoothing());
    const ProcMixPlan none = planProcMix(r, bypass, mix, S, n, B);              // nothing ramps: nothing allocated
    CHECK(!none.anyRamp && none.rampStride == 0 && none.len.empty() && none.gains.empty());
}

// the stage's arithmetic against the expressions of the engine in front of the move, written out
static void procArithmetic()
{
    const double pi = 3.141592653589793238462643383279502884;
    for (double x : { 0.0, 0.25, 0.5, 1.0 }) {
        const double t = x * (pi * 0.5), t2 = t * t;
        CHECK(equalPowerSin(x) == t * (1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 + t2 * (-1.0 / 5040.0 + t2 * (1.0 / 362880.0))))));
    }
    CHECK(equalPowerSin(0.0) == 0.0 && equalPowerSin(1.0) > 1.0000035 && equalPowerSin(1.0) < 1.0000036);
    for (double value : { 0.0, 0.001, 0.0011, 0.5, 0.999, 1.0 })
        for (double mix : { value, (double)(float)value }) {        // the engine hands over the float it was given, widened
            double g0 = equalPowerSin(mix) * 1.0;
            double g1 = (mix < 0.999) ? equalPowerSin(1.0 - mix) : 0.0;
            if (!(mix > 0.001)) { g0 = 0.0; g1 = 1.0; }
            const MixGains g = staticMixGains(mix);
            CHECK(g.wet == g0 && g.dry == g1);
        }
    CHECK(staticMixGains(0.001).wet == 0.0 && staticMixGains(0.001).dry == 1.0 && staticMixGains(0.0011).wet > 0.0);
    CHECK(staticMixGains(0.999).dry == 0.0 && staticMixGains(1.0).dry == 0.0 && staticMixGains(0.5).dry == staticMixGains(0.5).wet);
    CHECK(procDelay(false, 64, 40) == 104 && procDelay(true, 64, 40) == 40 && procDelay(false, 64, -5) == 64);
    CHECK(procDelay(false, 1 << 20, 0) == 524288 && procDelay(false, 64, 1 << 30) == 64 + 2097152 && procDelay(true, 1 << 20, 1 << 30) == 2097152);
}

// test_processor_level_dry_only_with_unequal_ramps_fails_before_any_state_moves: B = 512, calls of 4 callbacks; stream 0 is in
// mid-ramp when both streams are set dry-only, so its ramp ends a call before stream 1's: in that call stream 0 would rest and
// stream 1 not, which has to be known -- twice, the call is refused and made again -- before either ramp moves
static void unequalRamps()
{
    const Shape sh{ 512, 48000.0 };
    const int n = 4 * 512;
    MixState m[2] = { { MixRamp{}, 1.0 }, { MixRamp{}, 1.0 } };
    for (auto& s : m) s.r.ramp.totalSteps = LinearRamp::stepsFor(sh.rate, 0.1);
    std::vector<double> o;
    for (auto& s : m) mixCall(s, sh, n, o);
    m[0].mix = (double)0.5f;
    for (auto& s : m) mixCall(s, sh, n, o);
    CHECK(m[0].r.ramp.remaining == 2752 && !m[1].r.ramp.isSmoothing());
    m[0].mix = m[1].mix = 0.0;
    for (auto& s : m) mixCall(s, sh, n, o);
    CHECK(m[0].r.ramp.remaining == 704 && m[1].r.ramp.remaining == 2752);
    for (auto& s : m) mixCall(s, sh, n, o);
    CHECK(!m[0].r.ramp.isSmoothing() && m[1].r.ramp.remaining == 704);
    MixRamp r[2] = { m[0].r, m[1].r };
    const double mix[2] = { m[0].mix, m[1].mix };
    const char bypass[2] = { 0, 0 }, dryOnly[2] = { 1, 1 };
    for (int attempt = 0; attempt < 2; ++attempt) {
        const ProcRest rest = planProcRest(r, bypass, dryOnly, mix, 2, n, sh.B);
        CHECK(rest.rest[0] && !rest.rest[1] && rest.anyRest && !rest.allRest);                      // dry-only: 0 rests, 1 does not
        CHECK(same(m[0].r, r[0]) && same(m[1].r, r[1]));
    }
    const ProcMixPlan p = planProcMix(r, bypass, mix, 2, n, sh.B);
    CHECK(p.anyRamp && p.len[0] == 0 && p.len[1] == 1024 && p.rampStride == 1024 && p.gains.size() == (size_t)2 * 1024 * 2);
    for (size_t i = 0; i < (size_t)1024 * 2; ++i) CHECK(p.gains[i] == 0.0);                         // the row of the stream at rest
}

static void policies()
{
    GainRamp g;
    CHECK(!g.moving());
    g.wanted = 1.0 + 5.0e-7;                                    // below the retarget threshold: no ramp, yet not at rest either
    CHECK(g.moving());
    const GainRamp::Segment s = g.callback(64, 2400);
    CHECK(s.start == 1.0 && s.increment == 0.0 && !g.ramp.isSmoothing() && g.moving());
    g.snap();
    CHECK(!g.moving() && g.ramp.current == g.wanted && g.ramp.target == g.wanted);

    EqBypass b;
    CHECK(!b.active());
    b.requested = true;
    CHECK(b.active());
    b.sync();
    CHECK(b.effective && b.fade.current == 0.0 && b.fade.target == 0.0 && !b.fade.isSmoothing() && b.active());
    std::vector<double> vals;
    EqBypass::Step st = b.callback(64, 240, vals);
    CHECK(st.cls == EqBypass::kPass && !st.released && vals.empty());
    b.requested = false;
    st = b.callback(64, 240, vals);
    CHECK(st.cls == EqBypass::kFade && st.released && vals.size() == 64 && !b.effective && b.active());
    b.mode = 1;
    for (int t = 0; t < 3; ++t) st = b.callback(64, 240, vals);
    CHECK(st.cls == EqBypass::kFade && !st.released && vals.size() == 240 && vals.back() == 1.0 && b.active());     // mode != 0 alone
    st = b.callback(64, 240, vals);
    CHECK(st.cls == EqBypass::kNormal && vals.size() == 240);
    b.mode = 0;
    CHECK(!b.active());

    LatencyFade f;
    f.prime(64, -5);
    CHECK(f.latCurrent == 64.0 && f.primed && f.fade.current == 1.0);
    f.prime(64, 1 << 30);
    CHECK(f.latCurrent == 64.0 + 2097152.0);
    f.prime(1 << 22, 1 << 30);
    CHECK(f.latCurrent == 2097152.0 + 524288.0 && f.latTarget == f.latCurrent && f.oldDelay == f.latCurrent);
    f.prime(64, 100);
    CHECK(!f.beginCallback(165.0, 960) && f.newDelay() == 164);          // a move of less than 2 samples starts nothing
    CHECK(f.beginCallback(166.0, 960) && f.fade.current == 0.0 && f.fade.remaining == 960 && f.oldDelay == 164.0 && f.newDelay() == 166);
    CHECK(!f.beginCallback(300.0, 960));                                 // not while one is running
    f.advance(959, nullptr);
    CHECK(f.fading() && f.latCurrent == 164.0);
    std::vector<double> one;
    f.advance(64, &one);
    CHECK(one.size() == 1 && one[0] == 1.0 && !f.fading() && f.latCurrent == 166.0 && f.oldDelay == 166.0);
    f.advance(64, &one);
    CHECK(one.size() == 1);
}

int main()
{
    rampSemantics();
    policies();
    procArithmetic();
    oneSampleFadeStart();
    latencyRanges();
    unequalRamps();
    mixPlanShape();
    splitScripts();
    eqPlanScripts();
    fadeEndValues();
    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
