// engine_native.cpp -- plan groups: streams whose convolver runs on the reference's OWN layer plan (every layer at its own
// partition size, src/MKLNonUniformConvolver.cpp:738-758) with the reference's Add / Get bookkeeping replayed per chunk.
//
// Used for (engine_conv.cpp decides per set_impulse): CPQ_CALLS_ANY engines (any call quantum, ragged calls:
// inputPos accumulation :1431-1446, output ring with zero-fill :1376-1402), CPQ_SCHED_REFERENCE_NUC, and FilterSpec plans with
// tail layers (the spectral gains are partition-size dependent, :336-443).  A group = the streams that share one layer
// plan AND one phase (they were loaded while the group was fresh): the integer state of the reference's Add / Get --
// input fill of every layer, the distributed tail MAC's progress (:1497-1545), delay-line cursors (:1653-1688), ring
// read / write counts -- is then the same for all of them and is replayed ONCE on the host per call; the GPU moves the
// data (per layer: input accumulator -> FFT -> FDL MAC -> IFFT -> output ring / delay line -> chunk-wise read).  Streams
// with different IR lengths, FilterSpecs or load times live in different groups, as one StereoConvolver per stream does
// in the reference (src/ConvolverProcessor.h:741-814).
#include "engine_internal.hpp"

#include <type_traits>

using namespace cpqi;

namespace cpqi {

namespace {

struct BufItem { void* ptr; int64_t rowBytes; bool perSlot; };    // perSlot: [hSlots] rows instead of [capCh]

// the row buffers of one layer: f(pointer member, bytes per channel row, perSlot), on a const layer or one being laid out
template <typename Layer, typename F>
void forEachRowBuffer(Layer& t, F&& f)
{
    f(t.X, (int64_t)t.ringSlots * t.P * (int64_t)sizeof(double2), false);
    f(t.XDN, (int64_t)t.ringSlots * (int64_t)sizeof(double2), false);
    f(t.H, (int64_t)t.hRows * t.P * (int64_t)sizeof(double2), true);
    f(t.HDN, (int64_t)t.hRows * (int64_t)sizeof(double2), true);
    f(t.Y, (int64_t)t.nbMax * t.P * (int64_t)sizeof(double2), false);
    f(t.hist[0], (int64_t)t.P * (int64_t)sizeof(double), false);
    f(t.hist[1], (int64_t)t.P * (int64_t)sizeof(double), false);
    f(t.acc[0], (int64_t)t.accCap * (int64_t)sizeof(double), false);
    f(t.acc[1], (int64_t)t.accCap * (int64_t)sizeof(double), false);
    f(t.ring, (int64_t)t.outRing * (int64_t)sizeof(double), false);
}

// the same as (pointer, bytes per channel row) so that growing a group copies row prefixes
std::vector<BufItem> layerItems(const NativeLayer& t)
{
    std::vector<BufItem> items;
    forEachRowBuffer(t, [&](auto* p, int64_t rowBytes, bool perSlot) { items.push_back(BufItem{ p, rowBytes, perSlot }); });
    return items;
}

// lays the layer out in one allocation that it owns: on failure the layer is dropped with whatever it holds
int allocLayer(cpq_engine* e, NativeLayer& t, int capCh, int hSlots)
{
    int64_t total = 0;
    forEachRowBuffer(t, [&](auto*, int64_t rowBytes, bool perSlot) { total += alignUp(rowBytes * (perSlot ? hSlots : capCh), 256); });
    const int64_t twBytes = alignUp(t.P * (int64_t)sizeof(double2), 256);
    const int64_t gainBytes = alignUp((t.P + 1) * (int64_t)sizeof(double), 256);
    const int64_t scratchBytes = t.P > 4096 ? alignUp(std::max<int64_t>((int64_t)capCh * t.nbMax, t.K) * t.P * (int64_t)sizeof(double2), 256) : 256;
    const bool big = t.P > 4096;          // four-step transforms: + the two reordered tables (kernels.hpp: FftTables)
    total += (big ? 4 : 2) * twBytes + gainBytes + scratchBytes;
    {
        CPQ_TRY(allocAll(e, { { t.mem, (size_t)total } }, "plan group layer (partition %d, %d channels): %lld bytes could not be allocated",
                         t.P, capCh, (long long)total));
    }
    char* const mem = t.mem;
    CPQ_HIP(e, hipMemsetAsync(mem, 0, (size_t)total, e->stream));
    int64_t off = 0;
    forEachRowBuffer(t, [&](auto*& p, int64_t rowBytes, bool perSlot) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(mem + off);
        off += alignUp(rowBytes * (perSlot ? hSlots : capCh), 256);
    });
    t.tw = (double2*)(mem + off); off += twBytes;
    t.tw2 = (double2*)(mem + off); off += twBytes;
    t.twCol = t.twSplit = nullptr;
    if (big) { t.twCol = (double2*)(mem + off); off += twBytes; t.twSplit = (double2*)(mem + off); off += twBytes; }
    t.gainDev = (double*)(mem + off); off += gainBytes;
    t.scratch = (double2*)(mem + off);
    std::vector<double2> w, w2;
    hostTwiddles(t.P, w, w2);
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    CPQ_HIP(e, hipMemcpy(t.tw, w.data(), t.P * sizeof(double2), hipMemcpyHostToDevice));
    CPQ_HIP(e, hipMemcpy(t.tw2, w2.data(), t.P * sizeof(double2), hipMemcpyHostToDevice));
    if (big) {
        std::vector<double2> wc(t.P), ws(t.P);
        cpq::fill_big_twiddles(w.data(), w2.data(), t.P, wc.data(), ws.data());
        CPQ_HIP(e, hipMemcpy(t.twCol, wc.data(), t.P * sizeof(double2), hipMemcpyHostToDevice));
        CPQ_HIP(e, hipMemcpy(t.twSplit, ws.data(), t.P * sizeof(double2), hipMemcpyHostToDevice));
    }
    return CPQ_OK;
}

void layerGeometry(const cpq_engine* e, const cpq_nuc_plan& pl, int l, NativeLayer& t)
{
    const int nMax = e->maxCall;
    t.P = pl.part_size[l];
    t.K = pl.num_parts_ir[l];
    t.kPad = (int)alignUp(t.K, cpq::kMacMaxTile);                  // a multiple of every tile the MAC launcher may pick
    t.hRows = t.kPad + 16;                                         // zero rows for the kernels' 4-row read-ahead
    t.nbMax = (t.P - 1 + nMax) / t.P;
    t.ringSlots = nextPow2(t.kPad + cpq::kMacMaxTile + t.nbMax);
    t.accCap = t.P + nMax;
    t.gain = pl.gain[l];
    t.ppc = std::max(1, (int)pl.parts_per_callback[l]);
    t.outputDelay = pl.output_delay[l];
    // layer 0: the output ring holds what Get() has not read yet (< P0 + one chunk) plus one call of new blocks;
    // tail layers: the reader is at most outputDelay behind the writer, blocks are stored when their partition fills
    t.outRing = (l == 0) ? nextPow2(2 * t.P + nMax + t.P) : nextPow2(pl.output_delay[l] + 3 * t.P + nMax + e->B);
}

void resetGroupHost(PlanGroup& g)
{
    for (NativeLayer& t : g.layers) static_cast<LayerState&>(t) = LayerState{};
    g.samplesSinceReset = 0;
}

int uploadGroupMaps(cpq_engine* e, PlanGroup& g)
{
    std::vector<int> chMap((size_t)g.capCh, -1), irSlot((size_t)g.capCh, 0);
    g.usedCh = 0;
    for (int p = 0; p < g.capCh / 2; ++p) {
        const int s = g.streamOfPair[p];
        for (int ch = 0; ch < 2; ++ch) {
            chMap[2 * p + ch] = s >= 0 ? 2 * s + ch : -1;
            irSlot[2 * p + ch] = g.shared ? ch : 2 * p + ch;
        }
        if (s >= 0) g.usedCh = 2 * p + 2;
    }
    g.identityMap = true;                      // local channel i = row i of the call's buffers, no free slot in between
    for (int i = 0; i < g.usedCh; ++i) g.identityMap = g.identityMap && chMap[(size_t)i] == i;
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    CPQ_HIP(e, hipMemcpy(g.chMapDev, chMap.data(), sizeof(int) * chMap.size(), hipMemcpyHostToDevice));
    CPQ_HIP(e, hipMemcpy(g.irSlotDev, irSlot.data(), sizeof(int) * irSlot.size(), hipMemcpyHostToDevice));
    return CPQ_OK;
}

// a group with room for capPairs streams: allocates every layer (the old buffers' row prefixes are kept when growing).
// The new layers are built aside and swapped in on success: on any failure the group is as it was.
int sizeGroup(cpq_engine* e, PlanGroup& g, int capPairs)
{
    const int newCapCh = 2 * capPairs;
    const int hSlots = g.shared ? 2 : newCapCh;
    const std::vector<NativeLayer>& old = g.layers;
    const int oldCapCh = g.capCh, oldHSlots = g.shared ? 2 : oldCapCh;
    std::vector<NativeLayer> fresh;           // owners: whatever has been built is freed on every way out but the swap
    DeviceBuffer<int> chMapNew, irSlotNew;
    DeviceBuffer<long long> tabNew;
    fresh.reserve((size_t)g.plan.num_layers);
    auto undo = [&](int rc) {
        (void)hipStreamSynchronize(e->stream);      // row copies into the fresh buffers may still be in flight before they are freed
        (void)hipGetLastError();
        return rc;
    };
    for (int l = 0; l < g.plan.num_layers; ++l) {
        fresh.emplace_back();
        NativeLayer& t = fresh.back();
        if (!old.empty()) static_cast<LayerState&>(t) = old[(size_t)l];
        layerGeometry(e, g.plan, l, t);
        const int rc = allocLayer(e, t, newCapCh, hSlots);
        if (rc != CPQ_OK) return undo(rc);
        if (!old.empty()) {
            auto src = layerItems(old[(size_t)l]), dst = layerItems(t);
            for (size_t i = 0; i < src.size(); ++i) {
                const int64_t rows = src[i].perSlot ? oldHSlots : oldCapCh;
                if (hipMemcpyAsync(dst[i].ptr, src[i].ptr, (size_t)(rows * src[i].rowBytes), hipMemcpyDeviceToDevice, e->stream) != hipSuccess)
                    return undo(fail(e, CPQ_ERR_DEVICE, "plan group rows could not be copied"));
            }
        }
    }
    if (hipStreamSynchronize(e->stream) != hipSuccess) return undo(fail(e, CPQ_ERR_DEVICE, "plan group resize: stream error"));
    const int tabCap = nucTabEntries(fresh.data(), fresh.size(), e->maxCall, e->B);  // table size of the new geometry
    {
        const int rc = allocAll(e, { { chMapNew, (size_t)newCapCh }, { irSlotNew, (size_t)newCapCh }, { tabNew, (size_t)tabCap } },
                                "plan group tables could not be allocated");
        if (rc != CPQ_OK) return undo(rc);
    }
    // success: swap (the move assignments free what the group held, in the order layers, channel map, IR slots, tables)
    g.layers = std::move(fresh);
    g.chMapDev = std::move(chMapNew);
    g.irSlotDev = std::move(irSlotNew);
    g.tabDev = std::move(tabNew);
    g.capCh = newCapCh;
    g.streamOfPair.resize((size_t)capPairs, -1);
    g.tabCap = tabCap;
    return uploadGroupMaps(e, g);
}

// zero the run-time rows of one stereo pair (a stream that joins, or leaves, a group starts from silence like a new NUC)
int zeroPairState(cpq_engine* e, PlanGroup& g, int pair)
{
    for (NativeLayer& t : g.layers) {
        auto items = layerItems(t);
        for (const BufItem& it : items) {
            if (it.perSlot) continue;
            CPQ_HIP(e, hipMemsetAsync((char*)it.ptr + (int64_t)2 * pair * it.rowBytes, 0, (size_t)(2 * it.rowBytes), e->stream));
        }
    }
    return CPQ_OK;
}

}  // namespace

int resetGroups(cpq_engine* e)
{
    for (const auto& gp : e->groups) {
        PlanGroup& g = *gp;
        for (NativeLayer& t : g.layers) {
            auto items = layerItems(t);
            for (const BufItem& it : items)
                if (!it.perSlot) CPQ_HIP(e, hipMemsetAsync(it.ptr, 0, (size_t)(it.rowBytes * g.capCh), e->stream));
        }
        resetGroupHost(g);
        g.frozen = false;       // resting is processor-level state: the next processor-level call re-establishes it (enqueueConvProc)
    }
    return CPQ_OK;
}

int leaveNativeGroup(cpq_engine* e, int stream)
{
    const int gi = e->groupOf[(size_t)stream];
    if (gi < 0) return CPQ_OK;
    PlanGroup& g = *e->groups[(size_t)gi];
    for (size_t p = 0; p < g.streamOfPair.size(); ++p)
        if (g.streamOfPair[p] == stream) {
            g.streamOfPair[p] = -1;
            CPQ_TRY(zeroPairState(e, g, (int)p));
        }
    e->groupOf[(size_t)stream] = -1;
    bool empty = true;
    for (int s : g.streamOfPair) empty = empty && s < 0;
    if (empty) {
        CPQ_HIP(e, hipStreamSynchronize(e->stream));
        e->groups.erase(e->groups.begin() + gi);        // frees the group's buffers
        for (int& go : e->groupOf) if (go > gi) --go;
        return CPQ_OK;
    }
    return uploadGroupMaps(e, g);
}

// The stream gets a plan group of its own with its state and phase as they are (rows copied, host replay state copied):
// what a processor-level bypass needs, which stops ONE stream's Add / Get while the others go on (the reference's
// ConvolverProcessor does not call its convolver while bypassed or dry-only, Runtime.cpp:123-186, 573-585; on release the
// NUC resumes with the history it had).
static int isolateStream(cpq_engine* e, int stream)
{
    const int gi = e->groupOf[(size_t)stream];
    if (gi < 0) return CPQ_ERR_INVALID_ARG;
    PlanGroup& g = *e->groups[(size_t)gi];
    int members = 0, pair = -1;
    for (size_t p = 0; p < g.streamOfPair.size(); ++p) {
        if (g.streamOfPair[p] >= 0) ++members;
        if (g.streamOfPair[p] == stream) pair = (int)p;
    }
    if (members <= 1 || pair < 0) return CPQ_OK;
    std::unique_ptr<PlanGroup> n(new (std::nothrow) PlanGroup());
    if (!n) return fail(e, CPQ_ERR_OOM, "host allocation failed");
    n->plan = g.plan;
    n->hasSpec = g.hasSpec;
    n->spec = g.spec;
    n->shared = g.shared;
    n->samplesSinceReset = std::max<long long>(g.samplesSinceReset, 1);        // not fresh: nobody else may join its phase
    n->lastGot = g.lastGot;
    n->lastCall = g.lastCall;
    CPQ_TRY(sizeGroup(e, *n, 1));
    for (size_t l = 0; l < g.layers.size(); ++l) {
        const NativeLayer& src = g.layers[l];
        NativeLayer& dst = n->layers[l];
        auto si = layerItems(src), di = layerItems(dst);
        for (size_t i = 0; i < si.size(); ++i) {
            const int64_t rows = 2, from = si[i].perSlot ? (g.shared ? 0 : 2 * pair) : 2 * pair;
            if (hipMemcpyAsync(di[i].ptr, (char*)si[i].ptr + from * si[i].rowBytes, (size_t)(rows * si[i].rowBytes),
                               hipMemcpyDeviceToDevice, e->stream) != hipSuccess) {
                (void)hipStreamSynchronize(e->stream);          // before the new group's buffers go
                return fail(e, CPQ_ERR_DEVICE, "plan group rows could not be copied");
            }
        }
        static_cast<LayerState&>(dst) = src;
    }
    n->streamOfPair[0] = stream;
    // the stream is the new group's from here on, whatever happens below: the engine stays consistent
    g.streamOfPair[(size_t)pair] = -1;
    PlanGroup& isolated = *n;
    e->groups.push_back(std::move(n));
    e->groupOf[(size_t)stream] = (int)e->groups.size() - 1;
    CPQ_TRY(zeroPairState(e, g, pair));
    CPQ_TRY(uploadGroupMaps(e, g));
    return uploadGroupMaps(e, isolated);
}

// frozen: the stream's convolver is not called (bypass / dry-only at the processor level); its state waits as it is
int setStreamFrozen(cpq_engine* e, int stream, bool frozen)
{
    int gi = e->groupOf[(size_t)stream];
    if (gi < 0) return fail(e, CPQ_ERR_UNSUPPORTED, "a per-stream bypass needs the stream on the reference's own layer plan "
                                                   "(CPQ_CALLS_ANY, CPQ_SCHED_REFERENCE_NUC or a FilterSpec plan with tail layers); "
                                                   "on the uniform path set it for CPQ_ALL_STREAMS");
    if (e->groups[(size_t)gi]->frozen == frozen) return CPQ_OK;      // (a frozen group has one member: it was isolated first)
    CPQ_TRY(isolateStream(e, stream));
    gi = e->groupOf[(size_t)stream];
    e->groups[(size_t)gi]->frozen = frozen;
    return CPQ_OK;
}

void clearFrozen(cpq_engine* e)
{
    for (const auto& g : e->groups) g->frozen = false;
}

// SetImpulse of one stream (or of all streams with one shared stereo IR) on the reference's own layer plan
int nativeSetImpulse(cpq_engine* e, int stream, const double* irL, const double* irR, int irLen, double scale, int headTaps,
                     const cpq_filter_spec* spec, const cpq_nuc_plan& pl)
{
    if (pl.part_size[0] > 4096)
        return fail(e, CPQ_ERR_UNSUPPORTED, "layer-0 partition %d > 4096", pl.part_size[0]);
    for (int l = 1; l < pl.num_layers; ++l)
        if (pl.part_size[l] > 131072 || (pl.part_size[l] & (pl.part_size[l] - 1)))
            return fail(e, CPQ_ERR_UNSUPPORTED, "tail layer %d has partition size %d; supported: powers of two up to 131072", l, pl.part_size[l]);
    const int S = e->desc.n_streams;
    const bool shared = stream == CPQ_ALL_STREAMS;
    const int s0 = shared ? 0 : stream, s1 = shared ? S : stream + 1;
    for (int s = s0; s < s1; ++s) CPQ_TRY(leaveNativeGroup(e, s));

    // a fresh group with the same plan takes the stream(s); anything else would put them on another group's phase
    PlanGroup* g = nullptr;
    int gi = -1;
    if (!shared)
        for (size_t i = 0; i < e->groups.size() && !g; ++i) {
            PlanGroup& c = *e->groups[i];
            const bool sameSpec = c.hasSpec == (spec != nullptr) && (!spec || std::memcmp(&c.spec, spec, sizeof(*spec)) == 0);
            if (!c.shared && !c.frozen && c.samplesSinceReset == 0 && sameSpec && std::memcmp(&c.plan, &pl, sizeof(pl)) == 0) { g = &c; gi = (int)i; }     // (a resting group holds one isolated stream: nobody joins it)
        }
    if (!g) {
        std::unique_ptr<PlanGroup> made(new (std::nothrow) PlanGroup());
        if (!made) return fail(e, CPQ_ERR_OOM, "host allocation failed");
        g = made.get();
        g->plan = pl;
        g->hasSpec = spec != nullptr;
        if (spec) g->spec = *spec;
        g->shared = shared;
        CPQ_TRY(sizeGroup(e, *g, shared ? S : 1));     // one pair, doubled as members join: 256 one-member groups (256 IR lengths) cost what they use
        e->groups.push_back(std::move(made));
        gi = (int)e->groups.size() - 1;
    }
    // pair slots
    std::vector<int> pairOf;
    for (int s = s0; s < s1; ++s) {
        int pair = -1;
        for (size_t p = 0; p < g->streamOfPair.size() && pair < 0; ++p) if (g->streamOfPair[p] < 0) pair = (int)p;
        if (pair < 0) {
            pair = (int)g->streamOfPair.size();
            CPQ_TRY(sizeGroup(e, *g, std::min(S, std::max(2 * pair, 2))));
        }
        g->streamOfPair[(size_t)pair] = s;
        e->groupOf[(size_t)s] = gi;
        pairOf.push_back(pair);
    }
    CPQ_TRY(uploadGroupMaps(e, *g));

    // partition spectra of every layer (:919-946), the direct head's taps left out of the FFT path (:730-731), scaled
    // (:939-940), FilterSpec gains at the layer's own FFT size (:336-443), air absorption on the tail layers (:1060-1097)
    const double* irs[2] = { irL, irR };
    std::vector<double> seg, gains, air;
    const int hPair = shared ? 0 : pairOf[0];
    for (int ch = 0; ch < 2; ++ch) {
        const int slot = shared ? ch : 2 * hPair + ch;
        for (int l = 0; l < pl.num_layers; ++l) {
            NativeLayer& t = g->layers[(size_t)l];
            // the head zeroed, then scaled (:730-731 in front of :939-940): -0.0 taps at a negative scale
            prepareSegment(irs[ch] + pl.offset[l], pl.len[l], scale, l == 0 ? headTaps : 0, true, seg);
            if (spec) cpq::spectrumFilterGains(*spec, 2 * t.P, gains);
            const bool damped = spec && l > 0 && cpq::airAbsorptionGains(*spec, l, t.P + 1, air);
            const SpectraRows rows{ t.H + (int64_t)slot * t.hRows * t.P, t.HDN + (int64_t)slot * t.hRows, t.tables(), t.P, t.K, t.scratch, t.gainDev };
            CPQ_TRY(loadSpectra(e, l, seg, rows, t.hRows, spec ? &gains : nullptr, damped ? &air : nullptr));
        }
    }
    return CPQ_OK;
}

// ---------------------------------------------------------------------------------------------------- per call
// nuc_replay.hpp plans a call: planNucCall, run once per group in groupsAppend, replays the reference's Add / Get bookkeeping and
// makes every decision.  The three functions enqueueConv calls at three points of a call -- groupsAppend, groupsRunLayer0,
// groupsRunTails -- carry that plan out and decide nothing; what is left to them are the launchers' own limits
// (rfft_fwd_can_carry_side, kGatherTabMax).

// the group sits this call out: only the processor-level call rests a stream (ConvolverProcessor does not call its NUC then); a
// NUC-level call runs every stream
static bool resting(const cpq_engine* e, const PlanGroup& g) { return g.frozen && e->honourFrozen; }

// the call is whole partitions of layer t and its accumulator is empty: its forward transforms run straight from the call's input
static void fftFromInput(cpq_engine* e, const PlanGroup& g, const NativeLayer& t, const double* dIn, int n)
{
    ProfScope p(e, CPQ_K_RFFT_FWD);
    cpq::launch_rfft_fwd_ols(e->stream, dIn, (int64_t)n, t.hist[t.histSel], t.hist[t.histSel ^ 1], t.X, t.XDN,
                             t.tables(), t.P, g.usedCh, n / t.P, t.head, t.ringSlots, t.scratch);
}

static int appendGroup(cpq_engine* e, PlanGroup& g, const double* dIn, int n)
{
    NucCallPlan& c = g.call;
    planNucCall(c, g.layers.data(), g.layers.size(), n, NucCallFacts{ e->B, e->nCh, g.usedCh, g.identityMap, e->anyDirect, cpq::kP });
    if ((int)c.tab.size() > g.tabCap) return fail(e, CPQ_ERR_INVALID_ARG, "call of %d samples exceeds the engine's call capacity", n);
    // the straight layers' transforms run right here (before anything can write dOut, which may alias dIn) and runLayerBlocks
    // continues behind them; a held-back layer 0 follows below
    for (size_t l = c.hold0 ? 1 : 0; l < c.L; ++l)
        if (c.layer[l].straight) fftFromInput(e, g, g.layers[l], dIn, n);
    // every other layer accumulates the same input (Add(), :1431-1446): one pass over it
    double* dst[kNucMaxLayers];
    int64_t stride[kNucMaxLayers], off[kNucMaxLayers];
    for (int a = 0; a < c.nAcc; ++a) {
        const NativeLayer& t = g.layers[(size_t)c.accLayer[a]];
        dst[a] = t.acc[t.accSel];
        stride[a] = t.accCap;
        off[a] = t.fill;
    }
    // a small table leaves with the launch below (kernel arguments) instead of a host -> device copy of its own in front of layer 0
    const bool ride = (int)c.tab.size() <= cpq::kGatherTabMax && g.usedCh > 0 && n > 0;
    const int nTab = ride ? (int)c.tab.size() : 0;
    bool gathered = c.nAcc == 0, rode = false;
    if (c.hold0 && cpq::rfft_fwd_can_carry_side(g.layers[0].P, c.nAcc, stride, off, nTab)) {
        const NativeLayer& t = g.layers[0];
        ProfScope p(e, CPQ_K_RFFT_FWD);
        cpq::launch_rfft_fwd_ols_side(e->stream, dIn, (int64_t)n, t.hist[t.histSel], t.hist[t.histSel ^ 1], t.X, t.XDN,
                                      t.tables(), g.usedCh, n / t.P, t.head, t.ringSlots, c.nAcc, dst,
                                      stride, off, ride ? g.tabDev : nullptr, c.tab.data(), nTab);
        gathered = true;
        rode = ride;
    } else if (c.hold0) {
        fftFromInput(e, g, g.layers[0], dIn, n);
    }
    if (!gathered) {
        ProfScope p(e, CPQ_K_MIX);
        cpq::launch_rows_gather_multi(e->stream, dIn, n, g.chMapDev, c.nAcc, dst, stride, off, n, g.usedCh,
                                      ride ? g.tabDev : nullptr, c.tab.data(), nTab);
        rode = ride;
    }
    c.tabOnDevice = rode;       // the one launch outcome on the plan: from here on it is read-only
    return CPQ_OK;
}

int groupsAppend(cpq_engine* e, const double* dIn, int n)
{
    for (const auto& gp : e->groups)
        if (!resting(e, *gp)) CPQ_TRY(appendGroup(e, *gp, dIn, n));
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

// layer l: every partition that filled up in this call is convolved (FFT, FDL push, MAC over the layer's partitions,
// IFFT; NUC.cpp:1245-1336 / :1456-1544) and stored in the layer's output ring / delay line at the replayed positions
// directOut != nullptr (layer 0 only, the plan's `direct`): the inverse transform writes the members' output rows themselves and
// the output ring is passed by; with the plan's addTails it also adds the delay-line blocks of the tail layers, which have run
// ahead of layer 0 then
static int runLayerBlocks(cpq_engine* e, PlanGroup& g, const NucCallPlan& c, size_t l, double* directOut = nullptr)
{
    NativeLayer& t = g.layers[l];
    const int nb = c.layer[l].nb, rem = c.layer[l].rem;
    const int nCh = g.usedCh;
    if (nb > 0) {
        const cpq::FftTables tw = t.tables();
        bool remMoved = false;
        if (!c.layer[l].straight) {        // (else: transformed straight from the call's input in groupsAppend)
            ProfScope p(e, CPQ_K_RFFT_FWD);
            if (t.P == cpq::kP) {      // the 512-sample transform also moves the accumulator's remainder (no copy launch behind it)
                cpq::launch_rfft_fwd_ols_side(e->stream, t.acc[t.accSel], t.accCap, t.hist[t.histSel], t.hist[t.histSel ^ 1], t.X, t.XDN, tw, nCh, nb,
                                              t.head, t.ringSlots, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, t.acc[t.accSel ^ 1], t.accCap, rem);
                remMoved = true;
            } else {
                cpq::launch_rfft_fwd_ols(e->stream, t.acc[t.accSel], t.accCap, t.hist[t.histSel], t.hist[t.histSel ^ 1], t.X, t.XDN, tw,
                                         t.P, nCh, nb, t.head, t.ringSlots, t.scratch);
            }
        }
        {
            ProfScope p(e, CPQ_K_FDL_MAC);
            cpq::launch_fdl_mac(e->stream, e->macTile, t.X, t.H, g.irSlotDev, t.Y, t.P, nCh, t.K, t.ringSlots, t.head, nb,
                                (int64_t)t.hRows * t.P, !g.shared);
        }
        if (cpq::fdl_mac_needs_dcnyq(e->macTile, nb)) {
            ProfScope p(e, CPQ_K_DCNYQ);
            cpq::launch_fdl_mac_dcnyq(e->stream, t.XDN, t.HDN, g.irSlotDev, t.Y, t.P, nCh, t.K, t.ringSlots, t.head, nb, t.hRows);
        }
        {
            // the finished blocks go where the reference puts them: layer 0 straight to the members' output rows (directOut:
            // read and write positions advanced together by the replay), otherwise into the layer's output ring (layer 0: from
            // its write position before the call) / delay line (the table's put positions), written by the transform itself
            ProfScope p(e, CPQ_K_RFFT_INV);
            if (directOut && c.addTails) cpq::launch_rfft_inv_ols_add(e->stream, t.Y, directOut, (int64_t)c.n, tw, nCh, nb, g.tap(1), g.tap(2));
            else if (directOut) cpq::launch_rfft_inv_ols(e->stream, t.Y, directOut, (int64_t)c.n, tw, t.P, nCh, nb, t.scratch);
            else cpq::launch_rfft_inv_ols_ring(e->stream, t.Y, t.ring, t.outRing, l == 0 ? nullptr : g.tabDev + c.offs[2 * l + 1],
                                               l == 0 ? c.w0 : 0, tw, t.P, nCh, nb, t.scratch);
        }
        if (!remMoved && rem > 0) {
            ProfScope p(e, CPQ_K_MIX);
            cpq::launch_rows_copy(e->stream, t.acc[t.accSel], t.accCap, (int64_t)nb * t.P, t.acc[t.accSel ^ 1], t.accCap, 0, rem, nCh);
        }
        t.head = (t.head + nb) & (t.ringSlots - 1);
        t.histSel ^= 1;
        t.accSel ^= 1;
    }
    t.fill = rem;
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

static int runTailBlocks(cpq_engine* e, PlanGroup& g, const NucCallPlan& c)
{
    for (size_t l = 1; l < c.L; ++l) CPQ_TRY(runLayerBlocks(e, g, c, l));
    return CPQ_OK;
}

// layer 0 of every group: blocks, then the chunk-wise ring read into the members' output rows (which it overwrites)
int groupsRunLayer0(cpq_engine* e, double* dOut, int n)
{
    for (const auto& gp : e->groups) {
        PlanGroup& g = *gp;
        if (resting(e, g)) continue;
        const NucCallPlan& c = g.call;
        if (!c.tabOnDevice) CPQ_TRY(stageUpload(e, g.tabDev, c.tab.data(), c.tab.size() * sizeof(long long)));
        if (c.addTails) CPQ_TRY(runTailBlocks(e, g, c));        // ahead of layer 0, whose transform adds their blocks
        CPQ_TRY(runLayerBlocks(e, g, c, 0, c.direct ? dOut : nullptr));
        if (!c.direct && !c.getDeferred) {
            ProfScope p(e, CPQ_K_MIX);
            cpq::launch_ring_chunks(e->stream, dOut, n, g.chMapDev, n, e->B, g.layers[0].ring, g.layers[0].outRing,
                                    g.tabDev + c.offs[0], g.tabDev + c.offs[1], cpq::RingTap{}, cpq::RingTap{}, g.usedCh);
        }
        g.samplesSinceReset += n;
        g.lastCall = n;
        g.lastGot = c.lastGot;
    }
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

// tail layers of every group: blocks into the delay lines, then the chunk-wise read-add with the layer gain (:1620-1633)
int groupsRunTails(cpq_engine* e, double* dOut, int n)
{
    for (const auto& gp : e->groups) {
        PlanGroup& g = *gp;
        if (resting(e, g)) continue;
        const NucCallPlan& c = g.call;
        if (c.addTails) continue;       // (ran ahead of layer 0, whose transform added their blocks: groupsRunLayer0)
        CPQ_TRY(runTailBlocks(e, g, c));
        // one pass over the output: layer 0's chunk-wise ring read where it was deferred, then the delay lines (layer 1 first, as
        // Get() adds them)
        ProfScope p(e, CPQ_K_MIX);
        const NativeLayer& z = g.layers[0];
        if (c.getDeferred)
            cpq::launch_ring_chunks(e->stream, dOut, n, g.chMapDev, n, e->B, z.ring, z.outRing, g.tabDev + c.offs[0], g.tabDev + c.offs[1],
                                    g.tap(1), g.tap(2), g.usedCh);
        else if (c.L >= 2)
            cpq::launch_ring_chunks(e->stream, dOut, n, g.chMapDev, n, e->B, nullptr, 0, nullptr, nullptr, g.tap(1), g.tap(2), g.usedCh);
    }
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

}  // namespace cpqi
