// engine_conv.cpp -- kernel-level convolver: FilterSpec tail layers, the per-call kernel sequence, cpq_conv_* (see engine_internal.hpp, include/convopeq_mi355x.h).
#include "engine_internal.hpp"

using namespace cpqi;

namespace cpqi {

// --- enqueue helpers (device pointers, no sync) -----------------------------------------------------
// n samples per channel; the main (uniform) path needs n to be a whole number of partitions, plan groups take any n
int enqueueConv(cpq_engine* e, const double* dIn, double* dOut, int n)
{
    if (!cpq_conv_is_ready(e)) return fail(e, CPQ_ERR_NOT_READY, "set_impulse has not covered every stream");
    const int64_t stride = n;
    const int T = n / e->P;
    e->lastCallSamples = n;
    if (e->mainActive && (int64_t)T * e->P != n)
        return fail(e, CPQ_ERR_INVALID_ARG, "n_samples=%d is not a multiple of the partition size %d (streams on the uniform path)", n, e->P);
    // before anything writes dOut, which may alias dIn: the call's input joins the plan groups' accumulators and the direct head runs
    if (!e->groups.empty()) CPQ_TRY(groupsAppend(e, dIn, n));
    if (e->anyDirect) {
        ProfScope p(e, CPQ_K_MIX);
        // a stream whose convolver rests (per-stream bypass / dry-only at the processor level) keeps its head history: the
        // reference's processDirectBlock sits inside Add(), which ConvolverProcessor does not call then
        cpq::launch_direct_head(e->stream, dIn, stride, (int)stride, e->directIr, e->directTaps, e->irSlot,
                                e->directHist[e->directSel], e->directHist[e->directSel ^ 1], e->directOut, e->nCh,
                                e->honourFrozen ? e->procWetOn : nullptr);
        e->directSel ^= 1;
    }
    auto addDirect = [&]() {
        if (!e->anyDirect) return;
        ProfScope p(e, CPQ_K_MIX);
        cpq::launch_rows_add(e->stream, dOut, stride, e->directOut, (int)stride, e->nCh);
    };
    if (e->layered) {
        const cpq_nuc_plan& pl = e->layerPlan;
        const int nTail = pl.num_layers - 1;
        {
            ProfScope p(e, CPQ_K_RFFT_FWD);
            cpq::launch_rfft_fwd_ols(e->stream, dIn, stride, e->hist[e->histSel], e->hist[e->histSel ^ 1], e->X, e->XDN,
                                     tables(e), e->P, e->nCh, T, e->head, e->ringSlots);
        }
        // the tail layers first (natural time, into layerOut), then the reader's schedule for the call's callbacks, then layer
        // 0, whose inverse transform adds what the reader reads as it stores the output (no separate pass over the output)
        for (int l = pl.num_layers - 1; l >= 0; --l) {
            {
                ProfScope p(e, CPQ_K_FDL_MAC);
                cpq::launch_fdl_mac(e->stream, e->macTile, e->X, e->H + (int64_t)e->layerRow[l] * e->P, e->irSlot, e->Y,
                                    e->P, e->nCh, e->layerK[l], e->ringSlots, e->head, T, (int64_t)e->hRows * e->P, e->irPrivate);
            }
            if (cpq::fdl_mac_needs_dcnyq(e->macTile, T)) {
                ProfScope p(e, CPQ_K_DCNYQ);
                cpq::launch_fdl_mac_dcnyq(e->stream, e->XDN, e->HDN + e->layerRow[l], e->irSlot, e->Y, e->P, e->nCh,
                                          e->layerK[l], e->ringSlots, e->head, T, e->hRows);
            }
            if (l > 0) {
                ProfScope p(e, CPQ_K_RFFT_INV);
                cpq::launch_rfft_inv_ols(e->stream, e->Y, e->layerOut + (int64_t)(l - 1) * e->nCh * stride, stride, tables(e), e->P, e->nCh, T);
                continue;
            }
            {
                ProfScope p(e, CPQ_K_MIX);
                const int ppc1 = pl.parts_per_callback[1], ppc2 = nTail > 1 ? pl.parts_per_callback[2] : 1;
                const int d1 = (pl.num_parts_ir[1] + ppc1 - 1) / ppc1 - 1;
                const int d2 = nTail > 1 ? (pl.num_parts_ir[2] + ppc2 - 1) / ppc2 - 1 : 0;
                cpq::launch_tail_schedule(e->stream, e->tailState, e->tailSched, n / e->B, e->B, nTail, pl.part_size[1], pl.output_delay[1], d1,
                                          nTail > 1 ? pl.part_size[2] : e->B, nTail > 1 ? pl.output_delay[2] : 0, d2);
            }
            {
                ProfScope p(e, CPQ_K_RFFT_INV);
                cpq::launch_rfft_inv_ols_tail(e->stream, e->Y, dOut, stride, tables(e), e->P, e->nCh, T, nullptr, e->layerOut, e->tailRing,
                                              e->tailRingSlots, e->tailState, e->tailSched, n / e->B, e->B, nTail, pl.gain[1],
                                              nTail > 1 ? pl.gain[2] : 0.0);
            }
            {
                ProfScope p(e, CPQ_K_MIX);
                cpq::launch_tail_append(e->stream, e->tailState, e->layerOut, e->tailRing, e->nCh, (int)stride, e->tailRingSlots, nTail);
            }
        }
        addDirect();
        CPQ_HIP(e, hipGetLastError());
        e->head = (e->head + T) & (e->ringSlots - 1);
        e->histSel ^= 1;
        return CPQ_OK;
    }
    if (e->mainActive) {
        // the channels [c0, c0 + cnt): every buffer of the path is [channel][...]
        auto window = [&](int c0, int cnt) {
            const int64_t ring = (int64_t)c0 * e->ringSlots;
            {
                ProfScope p(e, CPQ_K_RFFT_FWD);
                cpq::launch_rfft_fwd_ols(e->stream, dIn + c0 * stride, stride, e->hist[e->histSel] + (int64_t)c0 * e->P,
                                         e->hist[e->histSel ^ 1] + (int64_t)c0 * e->P, e->X + ring * e->P, e->XDN + ring,
                                         tables(e), e->P, cnt, T, e->head, e->ringSlots);
            }
            double2* y = e->Y + (int64_t)c0 * T * e->P;
            {
                ProfScope p(e, CPQ_K_FDL_MAC);
                cpq::launch_fdl_mac(e->stream, e->macTile, e->X + ring * e->P, e->H, e->irSlot + c0, y, e->P, cnt,
                                    e->kMaxReal, e->ringSlots, e->head, T, (int64_t)e->hRows * e->P, e->irPrivate);
            }
            if (cpq::fdl_mac_needs_dcnyq(e->macTile, T)) {      // the cooperative kernel produces the packed (DC, Nyquist) bin itself
                ProfScope p(e, CPQ_K_DCNYQ);
                cpq::launch_fdl_mac_dcnyq(e->stream, e->XDN + ring, e->HDN, e->irSlot + c0, y, e->P, cnt, e->kMaxReal, e->ringSlots,
                                          e->head, T, e->hRows);
            }
            {
                ProfScope p(e, CPQ_K_RFFT_INV);
                cpq::launch_rfft_inv_ols(e->stream, y, dOut + c0 * stride, stride, tables(e), e->P, cnt, T);
            }
        };
        window(0, e->nCh);
        CPQ_HIP(e, hipGetLastError());
        e->head = (e->head + T) & (e->ringSlots - 1);
        e->histSel ^= 1;
    }
    // Get(): ring output of layer 0, then the direct output, then the tail layers (src/MKLNonUniformConvolver.cpp:1606-1633)
    if (!e->groups.empty()) CPQ_TRY(groupsRunLayer0(e, dOut, n));
    addDirect();
    if (!e->groups.empty()) return groupsRunTails(e, dOut, n);
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

}  // namespace cpqi

// ------------------------------------------------------------------------------------------ IR loading
namespace cpqi {

void zeroHead(std::vector<double>& seg, int headTaps)
{
    for (int i = 0; i < headTaps && i < (int)seg.size(); ++i) seg[(size_t)i] = 0.0;
}

void prepareSegment(const double* taps, int len, double scale, int headTaps, bool zeroThenScale, std::vector<double>& seg)
{
    seg.assign(taps, taps + len);
    if (zeroThenScale) zeroHead(seg, headTaps);
    if (std::abs(scale - 1.0) > 1e-12) for (double& v : seg) v *= scale;
    if (!zeroThenScale) zeroHead(seg, headTaps);
}

int loadSpectra(cpq_engine* e, int layer, const std::vector<double>& seg, const SpectraRows& r, int clearRows,
                const std::vector<double>* gainsA, const std::vector<double>* gainsB)
{
    if ((int64_t)seg.size() > e->heffCap)
        return fail(e, CPQ_ERR_INVALID_ARG, "layer %d has %zu taps, staging capacity %lld", layer, seg.size(), (long long)e->heffCap);
    if (clearRows > 0) {
        CPQ_HIP(e, hipMemsetAsync(r.H, 0, (size_t)clearRows * r.P * sizeof(double2), e->stream));
        CPQ_HIP(e, hipMemsetAsync(r.HDN, 0, (size_t)clearRows * sizeof(double2), e->stream));
    }
    CPQ_HIP(e, hipMemcpyAsync(e->heffDev, seg.data(), seg.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    cpq::launch_ir_spectra(e->stream, e->heffDev, (int)seg.size(), r.H, r.HDN, r.tw, r.P, r.nParts, r.scratch);
    bool gainDevBusy = false;
    for (const std::vector<double>* g : { gainsA, gainsB }) {
        if (!g || g->empty()) continue;
        if (gainDevBusy) CPQ_HIP(e, hipStreamSynchronize(e->stream));       // the first table's multiply still reads gainDev
        CPQ_HIP(e, hipMemcpyAsync(r.gainDev, g->data(), g->size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
        cpq::launch_spectrum_gain(e->stream, r.H, r.HDN, r.gainDev, r.P, r.nParts);
        gainDevBusy = true;
    }
    CPQ_HIP(e, hipGetLastError());
    CPQ_HIP(e, hipStreamSynchronize(e->stream));        // heffDev, gainDev and the caller's vectors are free again
    return CPQ_OK;
}

namespace {

// one cpq_conv_set_impulse call, as its steps below pass it on
struct ImpulseLoad {
    int stream, sFirst, sEnd;
    int slotBase;                   // IR slots: stream s owns slots 2s, 2s+1; CPQ_ALL_STREAMS shares slots 0 and 1 between all streams
    const double* ir[2];
    int irLen;
    double scale;
    bool direct;
    int headTaps;                   // taps that leave the FFT path for the direct head (0: none)
    const cpq_filter_spec* spec;
    bool native = false;            // a plan group takes the IR (engine_native.cpp)
    bool layered = false;           // the engine's layered (time-varying) mode takes it
    cpq_nuc_plan plan{};            // the plan the engine reports afterwards: native -- chooseNative's; main path -- the channel loads'
    std::vector<double> gains;      // FilterSpec gains at the engine's own partition (a spec without tail layers on the uniform path)
};

// Which path runs this IR?  A plan group (engine_native.cpp: every layer at the reference's own partition size, the Add / Get
// bookkeeping replayed per chunk) takes it when the engine accepts any call quantum (CPQ_CALLS_ANY), when it runs the reference's
// schedule natively (CPQ_SCHED_REFERENCE_NUC), or when a FilterSpec plan has tail layers -- the HC/LC gains (and the air-absorption
// damping) multiply every partition spectrum at that LAYER's FFT size (:336-443, :1060-1097).  Everything else runs on the main
// path: one uniform partition over h_eff.  Host work only.
int chooseNative(cpq_engine* e, ImpulseLoad& a)
{
    a.native = e->anyCalls || e->desc.schedule == CPQ_SCHED_REFERENCE_NUC;
    if (!a.spec && !a.native) return CPQ_OK;
    if (cpq::computeNucPlan(a.irLen, e->desc.block_size, a.direct, a.spec, &a.plan) != CPQ_OK)
        return fail(e, CPQ_ERR_INVALID_ARG, "layer plan failed");
    if (e->desc.semantics != CPQ_SEM_REFERENCE) return fail(e, CPQ_ERR_INVALID_ARG, "FilterSpec and the native schedule require reference semantics");
    if (a.spec && a.plan.num_layers > 1) a.native = true;
    if (!a.native && e->P != a.plan.part_size[0])
        return fail(e, CPQ_ERR_UNSUPPORTED, "FilterSpec needs partition_size == the reference layer-0 partition (%d)", a.plan.part_size[0]);
    if (a.native && e->layered) return fail(e, CPQ_ERR_UNSUPPORTED, "engine is in time-varying (layered) mode");
    if (a.spec && !a.native) cpq::spectrumFilterGains(*a.spec, 2 * e->P, a.gains);
    return CPQ_OK;
}

int ensureDirectHead(cpq_engine* e)
{
    if (e->directIr) return CPQ_OK;
    const size_t callSamples = (size_t)e->tMax * e->P;
    const size_t taps = (size_t)32 * e->nCh;
    CPQ_TRY(allocAll(e, { { e->directIr, taps, true }, { e->directTaps, (size_t)e->nCh, true }, { e->directHist[0], taps, true },
                          { e->directHist[1], taps, true }, { e->directOut, e->nCh * callSamples } },
                     "direct-head buffers could not be allocated"));
    e->directTapsHost.assign(e->nCh, 0);
    return CPQ_OK;
}

// the engine's first layered IR: the rows of each layer inside a channel's slot; then the per-layer buffers; the engine's state last
int enterLayered(cpq_engine* e, const cpq_nuc_plan& probe)
{
    const int nTail = probe.num_layers - 1;
    int row = 0, layerRow[3] = { 0, 0, 0 }, layerK[3] = { 0, 0, 0 };
    for (int l = 0; l < probe.num_layers; ++l) {
        layerRow[l] = row;
        layerK[l] = (probe.len[l] + e->P - 1) / e->P;
        row += (int)alignUp(layerK[l], cpq::kMacMaxTile) + cpq::kMacMaxTile;
    }
    if (row > e->hRows) return fail(e, CPQ_ERR_INVALID_ARG, "layered IR needs %d rows, capacity %d", row, e->hRows);
    int span = 0;
    for (int l = 1; l < probe.num_layers; ++l) span = std::max(span, probe.output_delay[l] + 2 * probe.part_size[l]);
    const int tailRingSlots = nextPow2(span + 2 * e->B + e->tMax * e->P);
    const size_t callSamples = (size_t)e->tMax * e->P;
    CPQ_TRY(allocAll(e, { { e->layerOut, nTail * e->nCh * callSamples }, { e->tailRing, (size_t)nTail * e->nCh * tailRingSlots, true },
                          { e->tailState, 4, true }, { e->tailSched, 2 * ((size_t)e->tMax * e->P / e->B) } },      // per tail layer and callback
                     "layered-mode buffers could not be allocated"));
    e->tailRingSlots = tailRingSlots;
    e->layerPlan = probe;
    std::copy(layerRow, layerRow + 3, e->layerRow);
    std::copy(layerK, layerK + 3, e->layerK);
    e->layered = true;
    return CPQ_OK;
}

// Does the reference stay LTI for this IR length / block size?  If not (tail partition longer than the IR that precedes it), the
// engine runs in layered mode: each layer is ONE linear convolution of the call with its segment of the IR, whatever the FFT
// partition; the reader that makes the plan time-varying is replayed per callback of block_size on the layer outputs.
int chooseLayered(cpq_engine* e, ImpulseLoad& a)
{
    if (e->desc.semantics != CPQ_SEM_REFERENCE || a.spec || a.native) return CPQ_OK;
    cpq_nuc_plan probe;
    if (cpq::computeNucPlan(a.irLen, e->desc.block_size, false, nullptr, &probe) != CPQ_OK)
        return fail(e, CPQ_ERR_INVALID_ARG, "layer plan failed");
    a.layered = !probe.lti_valid && probe.num_layers > 1;
    if (!a.layered) {
        if (e->layered) return fail(e, CPQ_ERR_UNSUPPORTED, "engine is in time-varying (layered) mode: every IR must share that plan");
        return CPQ_OK;
    }
    bool anyLoaded = false;
    for (char l : e->irLoaded) anyLoaded = anyLoaded || l;
    if (anyLoaded && (!e->layered || std::memcmp(&probe, &e->layerPlan, sizeof(probe)) != 0))
        return fail(e, CPQ_ERR_UNSUPPORTED, "time-varying reference semantics need the same IR length on every stream");
    return e->layered ? CPQ_OK : enterLayered(e, probe);
}

// SetImpulse leaves a convolver that has seen no input (every buffer is allocated anew and zeroed,
// src/MKLNonUniformConvolver.cpp:697-714, :880-935): the stream's input history goes -- the direct head's last samples, and on
// the main path its rows of the frequency-domain delay line and the overlap block; the other streams play on
int clearHistory(cpq_engine* e, const ImpulseLoad& a)
{
    for (int s = a.sFirst; s < a.sEnd; ++s) {
        for (const auto& h : e->directHist)
            if (h) CPQ_HIP(e, hipMemsetAsync(h + (size_t)2 * s * 32, 0, sizeof(double) * 2 * 32, e->stream));
        if (a.native || !e->X) continue;
        CPQ_HIP(e, hipMemsetAsync(e->X + (int64_t)2 * s * e->ringSlots * e->P, 0, (size_t)2 * e->ringSlots * e->P * sizeof(double2), e->stream));
        CPQ_HIP(e, hipMemsetAsync(e->XDN + (int64_t)2 * s * e->ringSlots, 0, (size_t)2 * e->ringSlots * sizeof(double2), e->stream));
        for (double* p : { e->hist[0], e->hist[1] })
            if (p) CPQ_HIP(e, hipMemsetAsync(p + (int64_t)2 * s * e->P, 0, (size_t)2 * e->P * sizeof(double), e->stream));
        if (e->tailRing)            // layered mode: the stream's delay lines (the reader's phase is the engine's and runs on)
            for (int l = 0; l + 1 < e->layerPlan.num_layers; ++l)
                CPQ_HIP(e, hipMemsetAsync(e->tailRing + ((size_t)l * e->nCh + 2 * s) * e->tailRingSlots, 0,
                                          sizeof(double) * 2 * e->tailRingSlots, e->stream));
    }
    return CPQ_OK;
}

// m_directIRRev (:716-718): the slot's head taps, reversed and scaled, for the time-domain FIR; nothing without direct-head buffers
int setDirectTaps(cpq_engine* e, const ImpulseLoad& a, int ch)
{
    if (!e->directIr) return CPQ_OK;
    const int slot = a.slotBase + ch;
    double rev[32] = { 0 };
    for (int i = 0; i < a.headTaps; ++i) rev[i] = a.ir[ch][a.headTaps - 1 - i] * a.scale;
    CPQ_HIP(e, hipMemcpyAsync(e->directIr + slot * 32, rev, sizeof(rev), hipMemcpyHostToDevice, e->stream));
    CPQ_HIP(e, hipMemcpyAsync(e->directTaps + slot, &a.headTaps, sizeof(int), hipMemcpyHostToDevice, e->stream));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));                     // rev is stack storage
    e->directTapsHost[slot] = a.headTaps;
    return CPQ_OK;
}

int loadNative(cpq_engine* e, const ImpulseLoad& a)
{
    // the stream(s) leave the main path: their rows there become zero (the main path then contributes silence)
    for (int ch = 0; ch < 2; ++ch) {
        const int slot = a.slotBase + ch;
        if (e->irParts[slot] > 0) {
            CPQ_HIP(e, hipMemsetAsync(e->H + (int64_t)slot * e->hRows * e->P, 0, (size_t)e->irParts[slot] * e->P * sizeof(double2), e->stream));
            CPQ_HIP(e, hipMemsetAsync(e->HDN + (int64_t)slot * e->hRows, 0, (size_t)e->irParts[slot] * sizeof(double2), e->stream));
            e->irParts[slot] = 0;
        }
        CPQ_TRY(setDirectTaps(e, a, ch));
    }
    return nativeSetImpulse(e, a.stream, a.ir[0], a.ir[1], a.irLen, a.scale, a.headTaps, a.spec, a.plan);
}

// rows [row0, row0 + nParts) of an IR slot of the main path
SpectraRows mainRows(const cpq_engine* e, int slot, int row0, int nParts)
{
    return SpectraRows{ e->H + ((int64_t)slot * e->hRows + row0) * e->P, e->HDN + (int64_t)slot * e->hRows + row0, tables(e), e->P, nParts,
                        nullptr, e->gainDev };
}

// layered mode: every layer's segment into its own rows of the slot, which is cleared whole first
int loadLayeredSlot(cpq_engine* e, ImpulseLoad& a, int ch)
{
    const int slot = a.slotBase + ch;
    const cpq_nuc_plan& pl = e->layerPlan;
    const SpectraRows whole = mainRows(e, slot, 0, 0);
    CPQ_HIP(e, hipMemsetAsync(whole.H, 0, (size_t)e->hRows * e->P * sizeof(double2), e->stream));
    CPQ_HIP(e, hipMemsetAsync(whole.HDN, 0, (size_t)e->hRows * sizeof(double2), e->stream));
    CPQ_TRY(setDirectTaps(e, a, ch));
    std::vector<double> seg;
    for (int l = 0; l < pl.num_layers; ++l) {
        // scaled, then the head zeroed (+0.0 whatever the scale's sign), as on the uniform path
        prepareSegment(a.ir[ch] + pl.offset[l], pl.len[l], a.scale, (l == 0 && e->directIr) ? a.headTaps : 0, false, seg);
        CPQ_TRY(loadSpectra(e, l, seg, mainRows(e, slot, e->layerRow[l], e->layerK[l]), 0, nullptr, nullptr));
    }
    e->irParts[slot] = e->hRows;
    a.plan = pl;
    return CPQ_OK;
}

// uniform path: one partition size over h_eff (reference semantics: buildHeff, which scales) or over the scaled IR (exact semantics)
int loadUniformSlot(cpq_engine* e, ImpulseLoad& a, int ch)
{
    const int slot = a.slotBase + ch;
    std::vector<double> heff;
    if (e->desc.semantics == CPQ_SEM_REFERENCE) {
        const int rc = cpq::buildHeff(a.ir[ch], a.irLen, e->desc.block_size, a.scale, a.spec, heff, &a.plan);
        if (rc != CPQ_OK) return fail(e, rc, "layer plan failed");
        if (!a.plan.lti_valid)
            return fail(e, CPQ_ERR_UNSUPPORTED, "the reference drops tail blocks for this IR length / block size (time-varying output)");
    } else {
        const int rc = cpq::computeNucPlan(a.irLen, e->desc.block_size, false, nullptr, &a.plan);
        if (rc != CPQ_OK) return fail(e, rc, "layer plan failed");
        prepareSegment(a.ir[ch], a.irLen, a.scale, 0, false, heff);
    }
    if (e->directIr) zeroHead(heff, a.headTaps);       // behind the scale (buildHeff applies it): +0.0 whatever the scale's sign
    CPQ_TRY(setDirectTaps(e, a, ch));
    const int parts = ((int)heff.size() + e->P - 1) / e->P;
    if (parts > e->kCap) return fail(e, CPQ_ERR_INVALID_ARG, "h_eff needs %d partitions, capacity %d", parts, e->kCap);
    // stale partitions of a longer previous IR in this slot become zero rows
    if (e->irParts[slot] > parts) {
        const SpectraRows stale = mainRows(e, slot, parts, 0);
        CPQ_HIP(e, hipMemsetAsync(stale.H, 0, (size_t)(e->irParts[slot] - parts) * e->P * sizeof(double2), e->stream));
        CPQ_HIP(e, hipMemsetAsync(stale.HDN, 0, (size_t)(e->irParts[slot] - parts) * sizeof(double2), e->stream));
    }
    CPQ_TRY(loadSpectra(e, 0, heff, mainRows(e, slot, 0, parts), 0, &a.gains, nullptr));
    e->irParts[slot] = parts;
    return CPQ_OK;
}

int loadMain(cpq_engine* e, ImpulseLoad& a)
{
    for (int s = a.sFirst; s < a.sEnd; ++s)
        if (e->groupOf[(size_t)s] >= 0) CPQ_TRY(leaveNativeGroup(e, s));        // back from a plan group to the main path
    for (int ch = 0; ch < 2; ++ch) CPQ_TRY(a.layered ? loadLayeredSlot(e, a, ch) : loadUniformSlot(e, a, ch));
    a.plan.direct_taps = a.direct ? std::min(a.irLen, std::min(a.plan.part_size[0], 32)) : 0;
    return CPQ_OK;
}

// the load succeeded: what the engine reports and what the per-call sequence reads
int finishImpulse(cpq_engine* e, const ImpulseLoad& a)
{
    e->plan = a.plan;
    e->planValid = true;
    e->directHead = a.direct;
    if (a.stream == CPQ_ALL_STREAMS) {
        for (int c = 0; c < e->nCh; ++c) { e->irSlotHost[c] = c & 1; e->irLoaded[c] = 1; }
    } else {
        for (int ch = 0; ch < 2; ++ch) { e->irSlotHost[2 * a.stream + ch] = 2 * a.stream + ch; e->irLoaded[2 * a.stream + ch] = 1; }
    }
    CPQ_HIP(e, hipMemcpy(e->irSlot, e->irSlotHost.data(), sizeof(int) * e->nCh, hipMemcpyHostToDevice));
    e->irPrivate = true;
    for (int c = 0; c < e->nCh; ++c) e->irPrivate = e->irPrivate && e->irSlotHost[c] == c;
    e->anyDirect = false;
    if (e->directIr)
        for (int c = 0; c < e->nCh; ++c) if (e->irLoaded[c] && e->directTapsHost[e->irSlotHost[c]] > 0) e->anyDirect = true;
    int kMax = 0;
    for (int c = 0; c < e->nCh; ++c) if (e->irLoaded[c]) kMax = std::max(kMax, e->irParts[e->irSlotHost[c]]);
    e->kMaxReal = kMax;
    e->kActive = (int)alignUp(kMax, cpq::kMacMaxTile);
    e->mainActive = false;
    for (int s = 0; s < e->desc.n_streams; ++s) e->mainActive = e->mainActive || (e->irLoaded[2 * s] && e->groupOf[(size_t)s] < 0);
    return CPQ_OK;
}

}  // namespace
}  // namespace cpqi

extern "C" {

// --------------------------------------------------------------------------- convolver
// The steps run in this order and each tests its own conditions in the order it always did.  Nothing is rolled back: a step that
// fails leaves what the steps before it (and itself, up to the failure) wrote -- buffers allocated, layered mode entered, history
// cleared, slot rows and irParts of the channels already loaded, plan-group membership -- while the bookkeeping of finishImpulse
// (the reported plan, readiness, the slot map, the active partition count) changes only when every step has succeeded.
int32_t cpq_conv_set_impulse(cpq_engine* e, int32_t stream, const double* irL, const double* irR, int32_t irLen,
                             double scale, int32_t direct, const cpq_filter_spec* spec)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!irL || !irR || irLen <= 0) return fail(e, CPQ_ERR_INVALID_ARG, "null impulse or non-positive length");
    ImpulseLoad a{};
    a.stream = stream;
    CPQ_TRY(streamRange(e, stream, a.sFirst, a.sEnd));
    if (irLen > e->desc.max_ir_len) return fail(e, CPQ_ERR_INVALID_ARG, "ir_len %d > max_ir_len %d", irLen, e->desc.max_ir_len);
    a.slotBase = (stream == CPQ_ALL_STREAMS) ? 0 : 2 * stream;
    a.ir[0] = irL; a.ir[1] = irR; a.irLen = irLen; a.scale = scale; a.direct = direct != 0; a.spec = spec;
    // Direct head (src/MKLNonUniformConvolver.cpp:689-731): the first min(irLen, partSize0, 32) taps leave the FFT path
    // (zeroed there, :730-731, before the spectra and any FilterSpec gains are formed) and run as a time-domain FIR.
    a.headTaps = direct ? std::min(irLen, std::min(nextPow2(std::max(e->desc.block_size, 64)), 32)) : 0;
    CPQ_TRY(chooseNative(e, a));
    CPQ_HIP(e, hipSetDevice(e->device));
    if (a.direct) CPQ_TRY(ensureDirectHead(e));
    CPQ_TRY(chooseLayered(e, a));
    CPQ_TRY(clearHistory(e, a));
    CPQ_TRY(a.native ? loadNative(e, a) : loadMain(e, a));
    return finishImpulse(e, a);
}

int32_t cpq_conv_is_ready(const cpq_engine* e)
{
    if (!e) return 0;
    for (char l : e->irLoaded) if (!l) return 0;
    return 1;
}

int32_t cpq_conv_latency(const cpq_engine* e) { return (e && e->planValid) ? e->plan.latency : 0; }

int32_t cpq_conv_get_plan(const cpq_engine* e, cpq_nuc_plan* plan)
{
    if (!e || !plan || !e->planValid) return CPQ_ERR_NOT_READY;
    *plan = e->plan;
    return CPQ_OK;
}

int32_t cpq_conv_last_got(const cpq_engine* e, int32_t stream)
{
    if (!e || stream < 0 || stream >= e->desc.n_streams) return CPQ_ERR_INVALID_ARG;
    const int gi = e->groupOf[(size_t)stream];
    return gi < 0 ? e->lastCallSamples : e->groups[(size_t)gi]->lastGot;
}

int32_t cpq_conv_reset(cpq_engine* e) { return e ? zeroRuntimeState(e, true, false) : CPQ_ERR_INVALID_ARG; }

int32_t cpq_conv_process_device(cpq_engine* e, const double* dIn, double* dOut, int32_t nSamples)
{
    CPQ_TRY(checkCall(e, dIn, dOut, nSamples));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueConv(e, dIn, dOut, nSamples);
}

int32_t cpq_conv_process(cpq_engine* e, const double* in, double* out, int32_t nSamples)
{
    return viaStaging(e, in, out, nSamples, [e](const double* a, double* b, int n) { return enqueueConv(e, a, b, n); });
}

}  // extern "C"
