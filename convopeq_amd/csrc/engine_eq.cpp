// engine_eq.cpp -- EQ and output filter: design, device tables, bypass / band-reset state machine, cpq_eq_* / cpq_outfilter_* (see engine_internal.hpp, include/convopeq_mi355x.h).
#include "engine_internal.hpp"

using namespace cpqi;

namespace cpqi {

// The gain is kept as it is (rtAgcCurrentGainShadow), not as gain - 1: (gain - 1) + 1 is not the gain again below 0.5, and a
// gain carried across a call boundary would then differ from the reference's in its last bit.  1.0 = 0x3FF00000'00000000.
int agcStateReset(cpq_engine* e, int s0, int n)
{
    CPQ_HIP(e, hipMemsetAsync(e->agcState + (size_t)s0 * 3, 0, (size_t)n * 3 * sizeof(double), e->stream));
    for (int s = s0; s < s0 + n; ++s)
        CPQ_HIP(e, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(reinterpret_cast<char*>(e->agcState + (size_t)s * 3 + 2) + 4), 0x3FF00000, 1, e->stream));
    return CPQ_OK;
}

// one cascade launch: the time-parallel kernels over every even number of samples, the lane-skewed one over a last odd sample (or everything)
int enqueueCascade(cpq_engine* e, const double* dIn, double* dOut, int64_t stride, int n, bool tp, int idTp, int idSeq,
                   const cpq::CascadeTables& t, bool streamPairs = false)
{
    const int nTp = tp ? n : 0;                   // the time-parallel kernels take any number of samples
    if (nTp > 0) {
        ProfScope p(e, idTp);
        cpq::launch_svf_cascade_tp(e->stream, dIn, dOut, stride, e->nCh, nTp, t, e->svfChain, e->svfChainSpans, e->svfChainGrid);
    }
    if (n > nTp) {
        ProfScope p(e, idSeq);
        cpq::launch_svf_cascade(e->stream, dIn + nTp, dOut + nTp, stride, e->nCh, n - nTp, t, streamPairs);
    }
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}



// prepareToPlay / reset: bypassFadeGain.setCurrentAndTargetValue(requested ? 0 : 1), the effective flag follows the
// request (src/eqprocessor/EQProcessor.Core.cpp:596, 656, 802)
void syncEqBypass(cpq_engine* e)
{
    e->anyEqBypass = false;
    std::fill(e->eqResetPending.begin(), e->eqResetPending.end(), 0u);      // the caller zeroes every state anyway
    std::fill(e->agcResetPending.begin(), e->agcResetPending.end(), 0);
    e->anyEqReset = false;
    for (auto& b : e->eqBypass) {
        b.sync();
        e->anyEqBypass = e->anyEqBypass || b.active();
    }
}

// Host image of one stream's cascade tables (cpq::CascadeTables), filled by one of the three functions below and written to the
// device by uploadCascade alone.
struct CascadeImage {
    enum : unsigned { kCoef = 1, kFlags = 2, kSatGain = 4, kTp = 8, kAll = 15 };
    double coef[2][kBands][6];
    int flags[2][kBands];
    std::vector<double> tp;
    double satGain[2];          // saturation, total gain: the same in both channels
    bool tpSafe = true, midSide = false;
    unsigned parts = kAll;      // the tables uploadCascade writes
};

// Device tables of one stream's EQ as the reference would run it: createCoeffCache (bandActive = enabled && sr > 0,
// src/eqprocessor/EQProcessor.ProcessingCache.cpp:71-90) or, for basicPath, the band nodes of the basic process(block)
// (inactive for non-LP/HP bands within 0.01 dB of flat: createBandNode, Coefficients.cpp:48-53).  An active Mid/Side
// band sends the whole call through the basic path (Processing.cpp:1036-1044).
void designEqStream(const cpq_engine* e, const cpq_eq_params& p, bool basicPath, CascadeImage& d)
{
    d.tp.assign((size_t)kBands * cpq::kSvfTpTableDoubles, 0.0);
    d.tpSafe = true;
    d.midSide = false;
    for (int b = 0; b < kBands; ++b)
        d.midSide = d.midSide || (p.bands[b].enabled && e->sampleRate > 0.0 && p.bands[b].channel_mode >= 3);
    const bool nodes = basicPath || d.midSide;
    for (int b = 0; b < kBands; ++b) {
        const cpq_eq_band& bp = p.bands[b];
        bool active = bp.enabled && e->sampleRate > 0.0;
        if (nodes && bp.type != 3 && bp.type != 4 && std::fabs(bp.gain) < 0.01f) active = false;
        cpq_svf_coeffs c{ 0, 0, 0, 0, 0, 1, 0, 0 };
        if (active) {
            cpq::designSvf(bp.type, bp.frequency, bp.gain, bp.q, e->sampleRate, &c);
            d.tpSafe = cpq::buildSvfTpTables(c, &d.tp[(size_t)b * cpq::kSvfTpTableDoubles]) && d.tpSafe;
        }
        for (int ch = 0; ch < 2; ++ch) {
            const double v[6] = { c.a1, c.a2, c.a3, c.m0, c.m1, c.m2 };
            std::memcpy(d.coef[ch][b], v, sizeof(v));
            // Stereo -> both channels through the packed SSE2+FMA kernel; Left/Right -> one channel, scalar kernel
            // Mid/Side -> both channel lanes run the scalar kernel on the encoded component (flag bit 4 / 5)
            const bool on = active && (bp.channel_mode == 0 || bp.channel_mode == 1 + ch || bp.channel_mode >= 3);
            d.flags[ch][b] = (on ? 1 : 0) | ((bp.channel_mode != 0) ? 2 : 0) | (p.filter_structure == 1 ? 8 : 0) |
                             (bp.channel_mode == 3 ? 16 : 0) | (bp.channel_mode == 4 ? 32 : 0);
        }
    }
    // with AGC the total-gain ramp is replaced by processAGC (Processing.cpp:1256-1259): unity gain in the cascade kernel
    d.satGain[0] = (double)p.nonlinear_saturation;
    d.satGain[1] = p.agc_enabled ? 1.0 : cpq::totalGainLinear(p.total_gain_db);
    if (p.filter_structure == 1 || d.midSide) d.tpSafe = false;   // parallel structure and Mid/Side bands: lane-skewed kernel
}

// the output filter's three DF-II-T sections in band slots 0 .. 2 (an identity section is run like the reference runs it)
void outFilterFlags(CascadeImage& d)
{
    for (int ch = 0; ch < 2; ++ch)
        for (int b = 0; b < kBands; ++b) d.flags[ch][b] = b < 3 ? (1 | 4) : 0;      // active, DF-II-T section
}
void outFilterImage(const cpq_biquad_coeffs q[3], CascadeImage& d)
{
    std::memset(d.coef, 0, sizeof(d.coef));
    d.tp.assign((size_t)kBands * cpq::kSvfTpTableDoubles, 0.0);
    d.tpSafe = true;
    for (int b = 0; b < 3; ++b) {
        const double v[6] = { q[b].b0, q[b].b1, q[b].b2, q[b].a1, q[b].a2, 0.0 };
        for (int ch = 0; ch < 2; ++ch) std::memcpy(d.coef[ch][b], v, sizeof(v));
        d.tpSafe = cpq::buildBiquadTpTables(q[b], &d.tp[(size_t)b * cpq::kSvfTpTableDoubles]) && d.tpSafe;
    }
    outFilterFlags(d);
    d.satGain[0] = 0.0;
    d.satGain[1] = 1.0;
}

// pass-through: no band active, no saturation, unity gain.  Only the flags and the saturation / gain pair are written: what
// the stream's coefficient and time-parallel tables hold stays
void passThroughImage(CascadeImage& d)
{
    std::memset(d.flags, 0, sizeof(d.flags));
    d.satGain[0] = 0.0;
    d.satGain[1] = 1.0;
    d.tpSafe = true;
    d.midSide = false;
    d.parts = CascadeImage::kFlags | CascadeImage::kSatGain;
}

// The one place that writes cascade tables: the image to every stream of [s0, s1), table by table in the order coef, flags,
// satGain, tp.  Blocking: plain hipMemcpy, for the setters, which have synchronised the engine's stream.  Staged: in order on the
// engine's stream with the kernels around it.
enum class Upload { kBlocking, kStaged };
int uploadCascade(cpq_engine* e, const cpq::CascadeTables& t, const CascadeImage& d, int s0, int s1, Upload how)
{
    auto put = [e, how](void* dst, const void* src, size_t bytes) -> int {
        if (how == Upload::kStaged) return stageUpload(e, dst, src, bytes);
        CPQ_HIP(e, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return CPQ_OK;
    };
    const double sg[4] = { d.satGain[0], d.satGain[1], d.satGain[0], d.satGain[1] };
    for (int s = s0; s < s1; ++s) {
        const size_t c = (size_t)2 * s;
        if (d.parts & CascadeImage::kCoef) CPQ_TRY(put(t.coef + c * kBands * 6, d.coef, sizeof(d.coef)));
        if (d.parts & CascadeImage::kFlags) CPQ_TRY(put(t.flags + c * kBands, d.flags, sizeof(d.flags)));
        if (d.parts & CascadeImage::kSatGain) CPQ_TRY(put(t.satGain + c * 2, sg, sizeof(sg)));
        if (d.parts & CascadeImage::kTp) CPQ_TRY(put(t.tp + (size_t)s * d.tp.size(), d.tp.data(), d.tp.size() * sizeof(double)));
    }
    return CPQ_OK;
}

// Switches what the device tables of one stream hold (on the engine's stream, in order with the kernels around it):
// 0 = the parameters as set, 1 = the basic path's band nodes, 2 = pass-through (EQ bypass in effect: nothing runs,
// not even the total gain, the AGC or the gain ramp).
int setEqStreamMode(cpq_engine* e, int s, int mode)
{
    auto& bp = e->eqBypass[s];
    if (bp.mode == mode) return CPQ_OK;
    if (mode != 2 && !e->eqParamsSet[s]) { bp.mode = mode; return CPQ_OK; }      // no parameters: every band inactive anyway
    CascadeImage d;
    if (mode == 2) passThroughImage(d);
    else designEqStream(e, e->eqParamsHost[s], mode == 1, d);
    CPQ_TRY(uploadCascade(e, e->eqTab, d, s, s + 1, Upload::kStaged));
    e->eqTpSafe[s] = d.tpSafe ? 1 : 0;
    e->eqMidSide[s] = d.midSide ? 1 : 0;
    e->gainRamp[s].devUnity = mode == 2;        // otherwise the constant gain (or 1.0 with AGC) is on the device again
    if (e->agcOn) {
        const int on = (mode != 2 && e->agcOnHost[s]) ? 1 : 0;
        CPQ_TRY(stageUpload(e, e->agcOn + s, &on, sizeof(int)));
    }
    bp.mode = mode;
    return CPQ_OK;
}

int setOutFilterPass(cpq_engine* e, int s, bool pass)
{
    CascadeImage d;
    if (pass) passThroughImage(d);
    else outFilterFlags(d);
    d.parts = CascadeImage::kFlags;             // the filter's saturation / gain pair is 0, 1 in either state
    CPQ_TRY(uploadCascade(e, e->ofTab, d, s, s + 1, Upload::kStaged));
    e->ofPass[s] = pass ? 1 : 0;
    return CPQ_OK;
}

// The total gain of a range of n samples in callbacks of B (Processing.cpp:1262-1274), planned on the host (planEqGain) and put on
// the device: the table entries that flip to unity or back, and -- only while some stream is moving -- the ramp kernel's segments.
// pass: streams (or nullptr) that are bypassed for the whole range; their ramp must not move either.
static int prepareGain(cpq_engine* e, int n, int B, const char* pass, EqGainPlan& g)
{
    const int S = e->desc.n_streams, cbs = n / B;
    // CPQ_CALLS_ANY: the last callback of the call is shorter than the quantum.  Refused before any ramp has moved
    if (n % B != 0 && anyGainRamp(e->gainRamp.data(), e->agcOnHost.data(), pass, S))
        return fail(e, CPQ_ERR_UNSUPPORTED, "a total-gain ramp is running: the call must be whole callbacks of %d samples until it ends", B);
    g = planEqGain(e->gainRamp.data(), e->agcOnHost.data(), pass, S, cbs, B, LinearRamp::stepsFor(e->sampleRate, 0.05));
    for (const EqGainPlan::Flip& f : g.flips) {
        for (int ch = 0; ch < 2; ++ch)
            CPQ_TRY(stageUpload(e, e->eqTab.satGain + (size_t)(2 * f.s + ch) * 2 + 1, &f.gain, sizeof(double)));
        e->gainRamp[f.s].devUnity = f.unity;
    }
    if (!g.anyRamp) return CPQ_OK;
    const size_t cbMax = (size_t)e->tMax * e->P / B;
    if (!e->rampOn)
        CPQ_TRY(allocAll(e, { { e->rampOn, (size_t)S }, { e->rampGains, 2 * S * cbMax } }, "gain ramp buffers could not be allocated"));
    CPQ_TRY(stageUpload(e, e->rampOn, g.rampOn.data(), sizeof(int) * S));
    return stageUpload(e, e->rampGains, g.segments.data(), sizeof(double) * g.segments.size());
}

// EQ over n samples of rows `stride` apart, in callbacks of B samples (AGC and gain ramp are block-rate), with the total gain as
// prepareGain left it on the device.
static int enqueueEqCore(cpq_engine* e, const double* dIn, double* dOut, int64_t stride, int n, int B, const EqGainPlan& g)
{
    bool tp = (e->eqMode == CPQ_EQ_MODE_AUTO);
    for (char s : e->eqTpSafe) tp = tp && s;
    const int cbs = n / B;
    e->eqProcessed = true;
    if (e->anyAgc && n % B != 0) return fail(e, CPQ_ERR_UNSUPPORTED, "the block-rate AGC needs calls of whole callbacks of %d samples", B);
    if (e->anyAgc) {
        ProfScope p(e, CPQ_K_MIX);
        cpq::launch_agc_block_rms(e->stream, dIn, stride, e->nCh, B, cbs, e->agcRmsIn);     // cachedInputRMS (:1116-1127)
    }
    bool midSide = false;
    for (char m : e->eqMidSide) midSide = midSide || m;
    CPQ_TRY(enqueueCascade(e, dIn, dOut, stride, n, tp, CPQ_K_SVF_TP, CPQ_K_SVF, e->eqTab, midSide));
    if (g.anyRamp) {
        ProfScope p(e, CPQ_K_MIX);
        cpq::launch_gain_ramp(e->stream, dOut, stride, e->desc.n_streams, B, cbs, e->rampGains, e->rampOn);
        CPQ_HIP(e, hipGetLastError());
    }
    if (!e->anyAgc) return CPQ_OK;
    {
        ProfScope p(e, CPQ_K_MIX);
        // block coefficients of the tables prepareToPlay builds (src/eqprocessor/EQProcessor.Core.cpp:776-784)
        const double nn = (double)B, sr = e->sampleRate;
        const double bAtt = 1.0 - std::exp(-nn / (sr * 0.2)), bRel = 1.0 - std::exp(-nn / (sr * 2.0)),
                     bSm = 1.0 - std::exp(-nn / (sr * 0.2));
        cpq::launch_agc_block_rms(e->stream, dOut, stride, e->nCh, B, cbs, e->agcRmsOut);
        cpq::launch_agc_apply(e->stream, dOut, stride, e->desc.n_streams, B, cbs, e->agcRmsIn, e->agcRmsOut,
                              e->agcState, e->agcOn, e->agcGains, bAtt, bRel, bSm);
    }
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

// rtAgcCurrentGainShadow = 1, envelopes = 0 (Processing.cpp:586-593, 1070-1077)
static int agcReset(cpq_engine* e, int s)
{
    if (e->agcState) CPQ_TRY(agcStateReset(e, s, 1));
    e->agcResetPending[s] = 0;
    return CPQ_OK;
}

// Silence is only known on the device: one small kernel, one read-back and ONE stream synchronisation per call while a band
// reset waits on a stream that is playing.  Leaves silent[stream][callback] in e->silentHost
static int readSilence(cpq_engine* e, const double* dIn, int64_t stride, int B, int cbs)
{
    const int S = e->desc.n_streams;
    const size_t cbMax = (size_t)e->tMax * e->P / B;
    if (!e->silentDev)
        CPQ_TRY(allocAll(e, { { e->silentDev, S * cbMax }, { e->silentHost, S * cbMax } }, "silence flags could not be allocated"));
    cpq::launch_block_silence(e->stream, dIn, stride, B, cbs, S, e->silentDev);
    CPQ_HIP(e, hipMemcpyAsync(e->silentHost, e->silentDev, sizeof(int) * (size_t)S * cbs, hipMemcpyDeviceToHost, e->stream));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

// one stream in front of a piece: the band states its reset mask names cleared, its tables switched to its class, a pending AGC
// reset carried out (a bypassed block returns before it)
static int applyPiece(cpq_engine* e, int s, const EqPiece::Stream& ps, int& rc)
{
    using T = cpq::CascadeTables;
    if (ps.reset == 0xFFFFFFFFu) {             // every band of the stream, Mid / Side states included
        CPQ_HIP(e, hipMemsetAsync(e->eqTab.state + T::stateAt(s, 0, 0), 0, sizeof(double) * T::stateDoubles(2), e->stream));
    } else if (ps.reset) {
        for (int b = 0; b < kBands; ++b)
            if (ps.reset & (1u << b))
                for (int ch = 0; ch < 2; ++ch)
                    CPQ_HIP(e, hipMemsetAsync(e->eqTab.state + T::stateAt(s, ch, b), 0, sizeof(double) * 2, e->stream));
    }
    rc = setEqStreamMode(e, s, ps.cls == EqBypass::kPass ? 2 : ps.cls == EqBypass::kFade ? 1 : 0);
    if (rc == CPQ_OK && e->agcResetPending[s] && ps.cls != EqBypass::kPass) rc = agcReset(e, s);
    return CPQ_OK;
}

// the cross-fade tables of a piece in which some stream fades: per stream on / length / end value and its fade values
static int uploadBlend(cpq_engine* e, const EqCallPlan& plan, const EqPiece& pc)
{
    const int S = e->desc.n_streams;
    std::vector<int> on(S), len(S);
    std::vector<double> end(S);
    int cap = 1;
    for (int s = 0; s < S; ++s) {
        on[s] = pc.streams[s].cls == EqBypass::kFade;
        len[s] = pc.streams[s].fadeLen;
        end[s] = pc.streams[s].fadeEnd;
        cap = std::max(cap, len[s]);
    }
    if (!e->eqDry)
        CPQ_TRY(allocAll(e, { { e->eqDry, (size_t)e->nCh * e->tMax * e->P }, { e->blendOn, (size_t)S }, { e->blendLen, (size_t)S },
                              { e->blendEnd, (size_t)S } }, "EQ bypass cross-fade buffers could not be allocated"));
    CPQ_TRY(grow(e, e->blendGains, e->blendCap, cap, (size_t)S, "EQ bypass cross-fade buffers could not be allocated"));
    std::vector<double> gains((size_t)S * e->blendCap, 0.0);
    for (int s = 0; s < S; ++s)
        if (len[s] > 0) std::memcpy(&gains[(size_t)s * e->blendCap], plan.fade[s].data() + pc.streams[s].fadeStart, sizeof(double) * (size_t)len[s]);
    CPQ_TRY(stageUpload(e, e->blendOn, on.data(), sizeof(int) * S));
    CPQ_TRY(stageUpload(e, e->blendLen, len.data(), sizeof(int) * S));
    CPQ_TRY(stageUpload(e, e->blendEnd, end.data(), sizeof(double) * S));
    return stageUpload(e, e->blendGains, gains.data(), sizeof(double) * gains.size());
}

// One piece of a call: the streams' states and tables, then the ordinary kernels, cross-faded with the dry block where a stream
// fades.  A status of the table switch, the AGC reset or the kernels comes back in rc and ends the call in order (the caller
// still settles anyEqBypass); every other failure returns at once, as a device error does anywhere.
static int runPiece(cpq_engine* e, const double* dIn, double* dOut, int64_t stride, int B, const EqCallPlan& plan, const EqPiece& pc,
                    int& rc)
{
    const int S = e->desc.n_streams;
    const int64_t off = (int64_t)pc.c0 * B;
    const int nSeg = (pc.c1 - pc.c0) * B;
    std::vector<char> pass(S);
    bool anyFade = false;
    for (int s = 0; s < S && rc == CPQ_OK; ++s) {
        CPQ_TRY(applyPiece(e, s, pc.streams[s], rc));
        pass[s] = pc.streams[s].cls == EqBypass::kPass;
        anyFade = anyFade || pc.streams[s].cls == EqBypass::kFade;
    }
    if (rc != CPQ_OK) return CPQ_OK;
    if (anyFade) {
        CPQ_TRY(uploadBlend(e, plan, pc));
        ProfScope p(e, CPQ_K_MIX);
        cpq::launch_rows_copy(e->stream, dIn, stride, off, e->eqDry, (int64_t)nSeg, 0, nSeg, e->nCh);
    }
    EqGainPlan g;
    rc = prepareGain(e, nSeg, B, pass.data(), g);
    if (rc == CPQ_OK) rc = enqueueEqCore(e, dIn + off, dOut + off, stride, nSeg, B, g);
    if (rc == CPQ_OK && anyFade) {
        ProfScope p(e, CPQ_K_MIX);
        cpq::launch_bypass_blend(e->stream, dOut + off, stride, e->eqDry, (int64_t)nSeg, nSeg, e->nCh, e->blendOn,
                                 e->blendLen, e->blendEnd, e->blendGains, e->blendCap);
        CPQ_HIP(e, hipGetLastError());
    }
    return CPQ_OK;
}

// EQProcessor as DSPCore drives it with a per-stream bypass request (setBypassFromRT + process,
// src/audioengine/AudioEngine.Processing.DSPCoreDouble.cpp:384-413).  Per callback and stream the host replays the
// bypass state machine of the basic process(block) (Processing.cpp:499-526, 565-624, 977-1015): a change of the request
// starts the 5 ms LinearRamp bypassFadeGain; callbacks that start while it runs are processed through the basic path
// (band nodes) and cross-faded with the dry block sample by sample; once the fade-out is complete the EQ returns early
// (states, gain ramp and AGC frozen); releasing the bypass clears every filter state and fades back in.  The call is cut
// where some stream changes class, each piece runs the ordinary kernels with the streams' tables switched accordingly.
// The plan is host_replay.hpp's (planEqCall, needsSilence, assignResets, cutPieces); here it is carried out.
// n samples of rows `stride` apart: whole callbacks of B samples, or (no per-callback state in play) any n
static int enqueueEqRange(cpq_engine* e, const double* dIn, double* dOut, int64_t stride, int n, int B)
{
    if (!e->eqSet) return fail(e, CPQ_ERR_NOT_READY, "cpq_eq_set_params has not been called");
    const int S = e->desc.n_streams;
    if (!e->anyEqBypass && !e->anyEqReset) {
        for (int s = 0; s < S; ++s)
            if (e->agcResetPending[s]) CPQ_TRY(agcReset(e, s));
        e->eqProcessed = true;
        EqGainPlan g;
        CPQ_TRY(prepareGain(e, n, B, nullptr, g));
        return enqueueEqCore(e, dIn, dOut, stride, n, B, g);
    }
    if (n % B != 0)
        return fail(e, CPQ_ERR_UNSUPPORTED, "an EQ bypass transition or band reset is pending: the call must be whole callbacks of %d samples", B);
    const int cbs = n / B;
    EqCallPlan plan = planEqCall(e->eqBypass.data(), S, cbs, B, LinearRamp::stepsFor(e->sampleRate, 0.005));    // BYPASS_FADE_TIME_SEC (EQProcessor.h:564)
    const bool silence = needsSilence(plan, e->eqResetPending.data());
    if (silence) CPQ_TRY(readSilence(e, dIn, stride, B, cbs));
    e->anyEqReset = assignResets(plan, e->eqResetPending.data(), silence ? e->silentHost.get() : nullptr);
    e->eqProcessed = true;
    int rc = CPQ_OK;
    for (const EqPiece& pc : cutPieces(plan)) {
        CPQ_TRY(runPiece(e, dIn, dOut, stride, B, plan, pc, rc));
        if (rc != CPQ_OK) break;
    }
    // after the pieces ran: a stream whose tables were left on the basic path's band nodes (its fade ended inside this call)
    // still needs the next call to come through here, which puts the parameter tables back
    bool stillActive = false;
    for (const auto& b : e->eqBypass) stillActive = stillActive || b.active();
    e->anyEqBypass = stillActive;
    return rc;
}

// A call whose last callback is shorter than the quantum (CPQ_CALLS_ANY: n = k B + r) runs as the whole callbacks followed
// by ONE callback of r samples, as the reference's process(block) sees them (src/convolver/ConvolverProcessor.Runtime.cpp:
// 659-682 cuts the host block the same way): the total-gain ramp skips r samples, the AGC takes its RMS and its block
// coefficients (table[numSamples], src/eqprocessor/EQProcessor.Processing.cpp:383-400) over r samples, the bypass fade
// draws r values.  Without per-callback state in play the cascade simply runs over all n samples.
int enqueueEq(cpq_engine* e, const double* dIn, double* dOut, int n)
{
    const int r = n % e->B;
    bool perCallback = e->anyAgc || e->anyEqBypass || e->anyEqReset;
    for (size_t s = 0; s < e->gainRamp.size() && !perCallback; ++s) perCallback = !e->agcOnHost[s] && e->gainRamp[s].moving();
    if (r == 0 || !perCallback) return enqueueEqRange(e, dIn, dOut, (int64_t)n, n, e->B);
    if (n - r > 0) CPQ_TRY(enqueueEqRange(e, dIn, dOut, (int64_t)n, n - r, e->B));
    return enqueueEqRange(e, dIn + (n - r), dOut + (n - r), (int64_t)n, r, r);     // the short callback: a callback of r samples
}

int enqueueOutFilter(cpq_engine* e, const double* dIn, double* dOut, int n)
{
    if (!e->ofSet) return fail(e, CPQ_ERR_NOT_READY, "cpq_outfilter_set_params has not been called");
    const bool tp = (e->eqMode == CPQ_EQ_MODE_AUTO) && e->ofTpSafe;
    return enqueueCascade(e, dIn, dOut, (int64_t)n, n, tp, CPQ_K_OUTFILT, CPQ_K_OUTFILT, e->ofTab);
}


}  // namespace cpqi

extern "C" {

// ---------------------------------------------------------------------------------- EQ
int32_t cpq_eq_set_params(cpq_engine* e, int32_t stream, const cpq_eq_params* p)
{
    if (!e || !p) return CPQ_ERR_INVALID_ARG;
    int s0 = 0, s1 = 0;
    CPQ_TRY(streamRange(e, stream, s0, s1));
    if (p->filter_structure != 0 && p->filter_structure != 1) return fail(e, CPQ_ERR_INVALID_ARG, "filter_structure must be 0 (serial) or 1 (parallel)");
    for (int b = 0; b < kBands; ++b)
        if (p->bands[b].enabled && (p->bands[b].channel_mode < 0 || p->bands[b].channel_mode > 4))
            return fail(e, CPQ_ERR_INVALID_ARG, "band %d: channel_mode must be 0..4 (Stereo, Left, Right, Mid, Side)", b);

    CascadeImage d;
    designEqStream(e, *p, false, d);
    CPQ_HIP(e, hipSetDevice(e->device));
    for (int s = s0; s < s1; ++s) { e->eqTpSafe[s] = d.tpSafe ? 1 : 0; e->eqMidSide[s] = d.midSide ? 1 : 0; }
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    CPQ_TRY(uploadCascade(e, e->eqTab, d, s0, s1, Upload::kBlocking));
    e->eqSet = true;   // streams never given parameters keep all bands inactive (pass-through)
    for (int s = s0; s < s1; ++s) { e->eqParamsHost[s] = *p; e->eqParamsSet[s] = 1; e->eqBypass[s].mode = 0; }
    for (int s = s0; s < s1; ++s) {
        auto& r = e->gainRamp[s];
        r.wanted = cpq::totalGainLinear(p->total_gain_db);
        r.devUnity = false;               // the upload above put the constant gain (or 1.0 with AGC) on the device
        if (!e->eqProcessed || p->agc_enabled) r.snap();
    }
    for (int s = s0; s < s1; ++s) e->agcOnHost[s] = p->agc_enabled ? 1 : 0;
    e->anyAgc = false;              // the AGC kernels run only once their buffers exist
    bool anyAgc = false;
    for (int v : e->agcOnHost) anyAgc = anyAgc || v;
    if (anyAgc) {
        const int S = e->desc.n_streams;
        const size_t cbMax = (size_t)e->tMax * e->P / e->B;
        if (!e->agcOn) {
            CPQ_TRY(allocAll(e, { { e->agcOn, (size_t)S }, { e->agcState, (size_t)3 * S, true }, { e->agcRmsIn, e->nCh * cbMax },
                                  { e->agcRmsOut, e->nCh * cbMax }, { e->agcGains, 2 * S * cbMax } }, "AGC buffers could not be allocated"));
            const int rs = agcStateReset(e, 0, S);
            if (rs != CPQ_OK) return rs;
            CPQ_HIP(e, hipStreamSynchronize(e->stream));
        }
        e->anyAgc = true;
        CPQ_HIP(e, hipMemcpy(e->agcOn, e->agcOnHost.data(), sizeof(int) * S, hipMemcpyHostToDevice));
    } else if (e->agcOn) {
        CPQ_HIP(e, hipMemcpy(e->agcOn, e->agcOnHost.data(), sizeof(int) * e->desc.n_streams, hipMemcpyHostToDevice));
    }
    return CPQ_OK;
}

int32_t cpq_eq_set_bypass(cpq_engine* e, int32_t stream, int32_t bypassed)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    int s0 = 0, s1 = 0;
    CPQ_TRY(streamRange(e, stream, s0, s1));
    for (int s = s0; s < s1; ++s) {
        auto& b = e->eqBypass[s];
        b.requested = bypassed != 0;
        if (!e->eqProcessed) b.sync();    // before the first callback the fade is synchronised, not run (Core.cpp:288, 802)
    }
    e->anyEqBypass = false;
    for (const auto& b : e->eqBypass) e->anyEqBypass = e->anyEqBypass || b.active();
    return CPQ_OK;
}

int32_t cpq_eq_request_band_reset(cpq_engine* e, int32_t stream, uint32_t bandMask)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    int s0 = 0, s1 = 0;
    CPQ_TRY(streamRange(e, stream, s0, s1));
    // requestBandReset(-1) asks for every band (mask 0xFFFFFFFF); single bands keep only the 20 real bits
    const uint32_t m = bandMask == 0xFFFFFFFFu ? bandMask : (bandMask & ((1u << kBands) - 1u));
    for (int s = s0; s < s1; ++s) {
        e->eqResetPending[s] |= m;
        e->anyEqReset = e->anyEqReset || e->eqResetPending[s] != 0u;
    }
    return CPQ_OK;
}

int32_t cpq_eq_request_agc_reset(cpq_engine* e, int32_t stream)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    int s0 = 0, s1 = 0;
    CPQ_TRY(streamRange(e, stream, s0, s1));
    for (int s = s0; s < s1; ++s) e->agcResetPending[s] = 1;
    return CPQ_OK;
}

int32_t cpq_eq_set_mode(cpq_engine* e, int32_t mode)
{
    if (!e || (mode != CPQ_EQ_MODE_AUTO && mode != CPQ_EQ_MODE_SEQUENTIAL)) return CPQ_ERR_INVALID_ARG;
    e->eqMode = mode;
    return CPQ_OK;
}

int32_t cpq_eq_reset(cpq_engine* e)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    syncEqBypass(e);
    return zeroRuntimeState(e, false, true);
}

int32_t cpq_eq_process_device(cpq_engine* e, const double* dIn, double* dOut, int32_t nSamples)
{
    CPQ_TRY(checkCall(e, dIn, dOut, nSamples));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueEq(e, dIn, dOut, nSamples);
}

int32_t cpq_eq_process(cpq_engine* e, const double* in, double* out, int32_t nSamples)
{
    return viaStaging(e, in, out, nSamples, [e](const double* a, double* b, int n) { return enqueueEq(e, a, b, n); });
}

// ------------------------------------------------------------------- output filter (N2)
int32_t cpq_outfilter_design(int32_t convIsLast, int32_t hcMode, int32_t lcMode, int32_t lpMode, double sampleRate,
                             cpq_biquad_coeffs out[3])
{
    if (!out || hcMode < 0 || hcMode > 2 || lcMode < 0 || lcMode > 1 || lpMode < 0 || lpMode > 2) return CPQ_ERR_INVALID_ARG;
    cpq::designOutputFilter(convIsLast, hcMode, lcMode, lpMode, sampleRate, out);
    return CPQ_OK;
}

int32_t cpq_outfilter_set_params(cpq_engine* e, int32_t stream, int32_t convIsLast, int32_t hcMode, int32_t lcMode,
                                 int32_t lpMode)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    int s0 = 0, s1 = 0;
    CPQ_TRY(streamRange(e, stream, s0, s1));
    cpq_biquad_coeffs q[3];
    const int rc = cpq_outfilter_design(convIsLast, hcMode, lcMode, lpMode, e->sampleRate, q);
    if (rc != CPQ_OK) return fail(e, rc, "bad output filter mode");
    CascadeImage d;
    outFilterImage(q, d);
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    for (int s = s0; s < s1; ++s) { e->ofModesHost[s] = cpq_engine::OfModes{ convIsLast, hcMode, lcMode, lpMode }; e->ofModesSet[s] = 1; }
    CPQ_TRY(uploadCascade(e, e->ofTab, d, s0, s1, Upload::kBlocking));      // active flags, whatever ofPass says of the stream
    e->ofTpSafe = e->ofTpSafe && d.tpSafe;      // one flag for every stream: once false it stays false
    e->ofSet = true;
    return CPQ_OK;
}

int32_t cpq_engine_enable_output_filter(cpq_engine* e, int32_t on)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    e->ofInPath = on != 0;
    return CPQ_OK;
}

int32_t cpq_outfilter_reset(cpq_engine* e)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipMemsetAsync(e->ofTab.state, 0, e->ofTab.stateDoubles(e->nCh) * sizeof(double), e->stream));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

int32_t cpq_outfilter_process_device(cpq_engine* e, const double* dIn, double* dOut, int32_t nSamples)
{
    CPQ_TRY(checkCall(e, dIn, dOut, nSamples));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueOutFilter(e, dIn, dOut, nSamples);
}

int32_t cpq_outfilter_process(cpq_engine* e, const double* in, double* out, int32_t nSamples)
{
    return viaStaging(e, in, out, nSamples, [e](const double* a, double* b, int n) { return enqueueOutFilter(e, a, b, n); });
}

}  // extern "C"
