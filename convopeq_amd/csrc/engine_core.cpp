// engine_core.cpp -- C ABI of libconvopeq_mi355x.so (see include/convopeq_mi355x.h): engine life cycle, routing, profiling.
//
// Host side of the engine: the device arena (the reference's per-buffer mkl_malloc manager,
// src/AlignedAllocation.h:22-163 + src/MKLNonUniformConvolver.h:288-365, collapsed into one HBM
// allocation laid out from (streams, partitions, ring slots, blocks per call)), the per-call kernel
// sequence, and the prepare/set_impulse/set_params control surface.  No CPU fallback exists: without a
// HIP device cpq_engine_create fails with CPQ_ERR_NO_DEVICE and nothing else can be called.
#include "engine_internal.hpp"

namespace {

std::string g_createError;
std::mutex g_createErrorMutex;

struct ArenaItem { void** ptr; int64_t bytes; };

// the arena slices of one cascade's tables (layouts: cpq::CascadeTables), in the order they lie in the arena
void cascadeSlices(cpq::CascadeTables& t, int64_t nCh, std::vector<ArenaItem>& items)
{
    const int64_t d = (int64_t)sizeof(double);
    items.push_back({ (void**)&t.coef, nCh * kBands * 6 * d });
    items.push_back({ (void**)&t.flags, nCh * kBands * (int64_t)sizeof(int) });
    items.push_back({ (void**)&t.satGain, nCh * 2 * d });
    items.push_back({ (void**)&t.state, (int64_t)t.stateDoubles((int)nCh) * d });
    items.push_back({ (void**)&t.tp, (nCh / 2) * kBands * cpq::kSvfTpTableDoubles * d });
}

}  // namespace

namespace cpqi {

int fail(cpq_engine* e, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (e) e->lastError = buf;
    else { std::lock_guard<std::mutex> lk(g_createErrorMutex); g_createError = buf; }
    return code;
}

int checkCurrentDevice()
{
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || nDev <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, CPQ_ERR_NO_DEVICE, "no HIP device visible: the gfx950 kernels cannot run (no CPU fallback)");
    }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return fail(nullptr, CPQ_ERR_NO_DEVICE, "hipGetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, CPQ_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, CPQ_ERR_NO_DEVICE, "device %d is %s; this library ships gfx950 code only", device, prop.gcnArchName);
    return CPQ_OK;
}

int nextPow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }
int64_t alignUp(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

cpq::FftTables tables(const cpq_engine* e) { return cpq::FftTables{ e->tw512, e->tw1024 }; }


int checkCall(cpq_engine* e, const void* in, const void* out, int nSamples)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!in || !out) return fail(e, CPQ_ERR_INVALID_ARG, "null buffer");
    if (e->anyCalls) {
        if (nSamples <= 0 || nSamples > e->maxCall)
            return fail(e, CPQ_ERR_INVALID_ARG, "n_samples=%d outside 1..%d (max_blocks_per_call * block_size)", nSamples, e->maxCall);
    } else {
        if (nSamples <= 0 || nSamples % e->P != 0)
            return fail(e, CPQ_ERR_INVALID_ARG, "n_samples=%d is not a positive multiple of the partition size %d "
                        "(create the engine with CPQ_CALLS_ANY for other call sizes)", nSamples, e->P);
        if (nSamples / e->P > e->tMax)
            return fail(e, CPQ_ERR_INVALID_ARG, "n_samples=%d exceeds max_blocks_per_call=%d blocks of %d", nSamples,
                        e->desc.max_blocks_per_call, e->B);
    }
    if ((reinterpret_cast<uintptr_t>(in) & 15u) || (reinterpret_cast<uintptr_t>(out) & 15u))
        return fail(e, CPQ_ERR_INVALID_ARG, "buffers must be 16-byte aligned");
    return CPQ_OK;
}

int checkBaseRows(cpq_engine* e, const void* in, const void* out, int n, bool on, const char* offText, bool wholeCallbacks)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!on) return fail(e, CPQ_ERR_NOT_READY, "%s", offText);
    if (!in || !out) return fail(e, CPQ_ERR_INVALID_ARG, "null buffer");
    if (n <= 0 || n > e->maxCall / e->osFactor)
        return fail(e, CPQ_ERR_INVALID_ARG, "n_samples=%d outside 1..%d", n, e->maxCall / e->osFactor);
    if (wholeCallbacks && !e->anyCalls && n % callbackLen(e) != 0)
        return fail(e, CPQ_ERR_INVALID_ARG, "n_samples=%d is not a multiple of the callback length %d", n, callbackLen(e));
    if ((reinterpret_cast<uintptr_t>(in) & 15u) || (reinterpret_cast<uintptr_t>(out) & 15u))
        return fail(e, CPQ_ERR_INVALID_ARG, "buffers must be 16-byte aligned");
    return CPQ_OK;
}

int refreshBaseRateStages(cpq_engine* e)
{
    CPQ_TRY(refreshMeters(e));          // truePeakDetector.prepare / loudnessMeter.prepare: coefficients for the base rate, everything cleared
    CPQ_TRY(refreshOutStage(e));        // dcBlockers().output*.init / peakLimiter.prepare + reset at the base rate
    return refreshDither(e);            // the shaper's prepare(rate, bits)
}


// Call-sized buffers that only some entry points need are allocated when first used: the staging pair of the host-pointer
// entry points, the hand-off buffer of the EQ -> convolver order (3 x 2 GB at 256 streams and 524288-sample calls).
int ensureCallBuffer(cpq_engine* e, DeviceBuffer<double>& buf, const char* what)
{
    if (buf) return CPQ_OK;
    const size_t count = (size_t)e->nCh * e->tMax * e->P;
    return allocAll(e, { { buf, count } }, "%s buffer of %zu bytes could not be allocated", what, count * sizeof(double));
}

int hostRoundTrip(cpq_engine* e, const double* in, size_t inLen, double* out, size_t outLen, bool inPlace,
                  const std::function<int(const double*, double*)>& body)
{
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_TRY(ensureCallBuffer(e, e->stageIn, "upload staging"));
    if (!inPlace) CPQ_TRY(ensureCallBuffer(e, e->stageOut, "download staging"));
    double* dst = inPlace ? e->stageIn : e->stageOut;
    CPQ_HIP(e, hipMemcpyAsync(e->stageIn, in, sizeof(double) * (size_t)e->nCh * inLen, hipMemcpyHostToDevice, e->stream));
    CPQ_TRY(body(e->stageIn, dst));
    if (outLen) CPQ_HIP(e, hipMemcpyAsync(out, dst, sizeof(double) * (size_t)e->nCh * outLen, hipMemcpyDeviceToHost, e->stream));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

void hostTwiddles(int P, std::vector<double2>& w1, std::vector<double2>& w2)
{
    w1.resize((size_t)P);
    w2.resize((size_t)P);
    const long double twoPi = 6.283185307179586476925286766559005768L;
    for (int m = 0; m < P; ++m) {
        const long double a = -twoPi * m / (long double)P, b = -twoPi * m / (long double)(2 * P);
        w1[(size_t)m] = make_double2((double)cosl(a), (double)sinl(a));
        w2[(size_t)m] = make_double2((double)cosl(b), (double)sinl(b));
    }
}

int streamRange(cpq_engine* e, int stream, int& s0, int& s1)
{
    if (stream != CPQ_ALL_STREAMS && (stream < 0 || stream >= e->desc.n_streams))
        return fail(e, CPQ_ERR_INVALID_ARG, "stream %d out of range", stream);
    s0 = (stream == CPQ_ALL_STREAMS) ? 0 : stream;
    s1 = (stream == CPQ_ALL_STREAMS) ? e->desc.n_streams : stream + 1;
    return CPQ_OK;
}

int zeroRuntimeState(cpq_engine* e, bool conv, bool eq)
{
    CPQ_HIP(e, hipSetDevice(e->device));
    if (conv) {
        CPQ_HIP(e, hipMemsetAsync(e->X, 0, (size_t)e->nCh * e->ringSlots * e->P * sizeof(double2), e->stream));
        CPQ_HIP(e, hipMemsetAsync(e->XDN, 0, (size_t)e->nCh * e->ringSlots * sizeof(double2), e->stream));
        CPQ_HIP(e, hipMemsetAsync(e->hist[0], 0, (size_t)e->nCh * e->P * sizeof(double), e->stream));
        CPQ_HIP(e, hipMemsetAsync(e->hist[1], 0, (size_t)e->nCh * e->P * sizeof(double), e->stream));
        e->head = 0;
        e->histSel = 0;
        CPQ_TRY(resetGroups(e));
        for (const auto& h : e->directHist)
            if (h) CPQ_HIP(e, hipMemsetAsync(h, 0, sizeof(double) * 32 * e->nCh, e->stream));
        if (e->tailState) CPQ_HIP(e, hipMemsetAsync(e->tailState, 0, 4 * sizeof(long long), e->stream));
        if (e->tailRing) CPQ_HIP(e, hipMemsetAsync(e->tailRing, 0, sizeof(double) * (size_t)(e->layerPlan.num_layers - 1) * e->nCh * e->tailRingSlots, e->stream));
        if (e->dryRing) CPQ_HIP(e, hipMemsetAsync(e->dryRing, 0, (size_t)e->nCh * e->dryRingSize * sizeof(double), e->stream));
        e->dryPos = 0;
        for (auto& f : e->latFade) f = LatencyFade{};
    }
    if (eq) {
        for (const cpq::CascadeTables* t : { &e->eqTab, &e->ofTab })
            CPQ_HIP(e, hipMemsetAsync(t->state, 0, t->stateDoubles(e->nCh) * sizeof(double), e->stream));
        if (e->agcState) CPQ_TRY(agcStateReset(e, 0, e->desc.n_streams));
    }
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}


}  // namespace cpqi

using namespace cpqi;

extern "C" {

int32_t cpq_abi_version(void) { return CPQ_ABI_VERSION; }
int32_t cpq_abi_revision(void) { return CPQ_ABI_REVISION; }

const char* cpq_status_string(int32_t s)
{
    switch (s) {
        case CPQ_OK: return "ok";
        case CPQ_ERR_INVALID_ARG: return "invalid argument";
        case CPQ_ERR_NO_DEVICE: return "no usable HIP device";
        case CPQ_ERR_OOM: return "out of device memory";
        case CPQ_ERR_DEVICE: return "HIP runtime error";
        case CPQ_ERR_UNSUPPORTED: return "not supported by this engine version";
        case CPQ_ERR_NOT_READY: return "engine not ready";
        case CPQ_ERR_SILENT_IR: return "silent impulse response";
        default: return "unknown status";
    }
}

const char* cpq_last_error(const cpq_engine* e)
{
    if (e) return e->lastError.c_str();
    std::lock_guard<std::mutex> lk(g_createErrorMutex);
    static thread_local std::string copy;
    copy = g_createError;
    return copy.c_str();
}

const char* cpq_kernel_name(int32_t id)
{
    switch (id) {
        case CPQ_K_RFFT_FWD: return "k_rfft_fwd_ols";
        case CPQ_K_FDL_MAC: return "k_fdl_mac";
        case CPQ_K_DCNYQ: return "k_fdl_mac_dcnyq";
        case CPQ_K_RFFT_INV: return "k_rfft_inv_ols";
        case CPQ_K_SVF: return "k_svf_cascade";
        case CPQ_K_SVF_TP: return "k_svf_cascade_tp";
        case CPQ_K_MIX: return "k_convproc_mix";
        case CPQ_K_OUTFILT: return "k_outfilter_cascade";
        case CPQ_K_OS: return "k_os_halfband";
        case CPQ_K_METER: return "k_meter";
        case CPQ_K_PCM: return "k_pcm";
        case CPQ_K_OUT: return "k_out";
        case CPQ_K_DITHER: return "k_dither";
        case CPQ_K_SOFTCLIP: return "k_soft_clip";
        default: return "?";
    }
}

// ------------------------------------------------------------------ host-only helpers
int32_t cpq_nuc_plan_compute(int32_t irLen, int32_t blockSize, int32_t direct, const cpq_filter_spec* spec,
                             cpq_nuc_plan* plan)
{
    return cpq::computeNucPlan(irLen, blockSize, direct != 0, spec, plan);
}

int32_t cpq_nuc_heff(const double* ir, int32_t irLen, int32_t blockSize, double scale, const cpq_filter_spec* spec,
                     double* heff, int32_t cap)
{
    if (!ir) return CPQ_ERR_INVALID_ARG;
    std::vector<double> h;
    cpq_nuc_plan p;
    CPQ_TRY(cpq::buildHeff(ir, irLen, blockSize, scale, spec, h, &p));
    if (heff && cap > 0) std::memcpy(heff, h.data(), sizeof(double) * (size_t)std::min<int>(cap, (int)h.size()));
    return (int32_t)h.size();
}

int32_t cpq_eq_design_svf(int32_t type, float freq, float gainDb, float q, double sr, cpq_svf_coeffs* out)
{
    if (!out) return CPQ_ERR_INVALID_ARG;
    cpq::designSvf(type, freq, gainDb, q, sr, out);
    return CPQ_OK;
}

void cpq_eq_params_default(cpq_eq_params* p) { if (p) cpq::defaultEqParams(p); }

// ------------------------------------------------------------------------------ engine
int32_t cpq_engine_create(const cpq_engine_desc* d, cpq_engine** out)
{
    if (!d || !out) return fail(nullptr, CPQ_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (d->struct_size != (int32_t)sizeof(cpq_engine_desc))
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "struct_size %d != %zu", d->struct_size, sizeof(cpq_engine_desc));
    if (d->n_streams <= 0 || d->max_ir_len <= 0 || d->max_blocks_per_call <= 0)
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "n_streams, max_ir_len and max_blocks_per_call must be positive");
    if (d->call_mode != CPQ_CALLS_WHOLE_BLOCKS && d->call_mode != CPQ_CALLS_ANY)
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "call_mode must be CPQ_CALLS_WHOLE_BLOCKS or CPQ_CALLS_ANY");
    const bool anyCalls = d->call_mode == CPQ_CALLS_ANY;
    if (anyCalls) {
        if (d->block_size < 1 || d->block_size > 4096)
            return fail(nullptr, CPQ_ERR_INVALID_ARG, "block_size (the call quantum) must be in [1, 4096]");
        if (d->semantics != CPQ_SEM_REFERENCE || (d->partition_size != 0 && d->partition_size != CPQ_PARTITION_AUTO))
            return fail(nullptr, CPQ_ERR_INVALID_ARG, "CPQ_CALLS_ANY runs the reference's own layer plan: reference semantics, partition_size 0");
    } else if (d->block_size < 64 || d->block_size > 4096 || (d->block_size & (d->block_size - 1)))
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "block_size must be a power of two in [64, 4096] (any quantum from 1 to 4096: call_mode = CPQ_CALLS_ANY)");
    if (d->semantics != CPQ_SEM_REFERENCE && d->semantics != CPQ_SEM_EXACT)
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "bad semantics");
    if (d->mac_tile != 0 && d->mac_tile != 4 && d->mac_tile != 8 && d->mac_tile != 16 && d->mac_tile != 32)
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "mac_tile must be 0, 4, 8, 16 or 32");
    if (d->schedule != CPQ_SCHED_UNIFORM && d->schedule != CPQ_SCHED_REFERENCE_NUC)
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "schedule must be CPQ_SCHED_UNIFORM or CPQ_SCHED_REFERENCE_NUC");
    if (d->schedule == CPQ_SCHED_REFERENCE_NUC &&
        (d->semantics != CPQ_SEM_REFERENCE ||
         (d->partition_size != 0 && d->partition_size != CPQ_PARTITION_AUTO && d->partition_size != d->block_size)))
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "the non-uniform schedule needs reference semantics and partition_size == block_size");

    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || nDev <= 0)
        return fail(nullptr, CPQ_ERR_NO_DEVICE, "no HIP device visible: the gfx950 kernels cannot run (no CPU fallback)");
    if (d->device < 0 || d->device >= nDev)
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "device %d out of range (%d visible)", d->device, nDev);
    if (hipSetDevice(d->device) != hipSuccess) return fail(nullptr, CPQ_ERR_NO_DEVICE, "hipSetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d->device) != hipSuccess)
        return fail(nullptr, CPQ_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, CPQ_ERR_NO_DEVICE, "device %d is %s; this library ships gfx950 code only", d->device,
                    prop.gcnArchName);

    cpq_engine* e = new (std::nothrow) cpq_engine();
    if (!e) return fail(nullptr, CPQ_ERR_OOM, "host allocation failed");
    e->desc = *d;
    e->device = d->device;
    e->sampleRate = d->sample_rate > 0.0 ? d->sample_rate : 48000.0;
    e->nCh = 2 * d->n_streams;
    e->B = d->block_size;
    e->anyCalls = anyCalls;
    e->P0 = nextPow2(std::max(d->block_size, 64));
    e->maxCall = (int)std::min<int64_t>((int64_t)d->max_blocks_per_call * d->block_size, (int64_t)1 << 30);
    int32_t partition = d->partition_size;
    if (partition == CPQ_PARTITION_AUTO) {
        // the larger partition wins wherever the calls allow it (profiles/r02b_sweep_partition_x_blocks_per_call.txt:
        // K shrinks by P / B, the FFT cost per sample stays): 4096 for calls of at least eight such partitions (below
        // that the MAC streams the same IR + FDL bytes per call at either size and the 512-point kernels do it faster:
        // profiles/r02e_small_calls.txt), else 512, else the block itself.  The reference's own
        // schedule and ragged calls keep the reference's layer-0 partition.  (Blocks of 1024 and more, whose reference plan
        // is time-varying, run one convolution per layer: those take the larger partition as well.)
        partition = 0;
        if (!anyCalls && d->schedule == CPQ_SCHED_UNIFORM)
            for (int32_t cand : { 4096, 512 })
                if (cand > d->block_size && e->maxCall % cand == 0 && (cand == 512 || e->maxCall >= 8 * cand)) { partition = cand; break; }
    }
    e->desc.partition_size = partition;
    e->P = partition ? partition : (anyCalls ? e->P0 : d->block_size);
    if (!anyCalls && (e->P < e->B || e->P > 4096 || (e->P & (e->P - 1)) || ((int64_t)d->max_blocks_per_call * e->B) % e->P != 0)) {
        const int p = e->P;
        delete e;
        return fail(nullptr, CPQ_ERR_INVALID_ARG,
                    "partition_size %d must be a power of two in [block_size, 4096] dividing block_size*max_blocks_per_call", p);
    }
    e->tMax = (int)(((int64_t)e->maxCall + e->P - 1) / e->P);     // partitions per call (rounded up for ragged calls)
    e->macTile = d->mac_tile;     // 0 = automatic (the rule: fdl_mac_variant, mac_kernels.hip)

    // partition capacity from the longest h_eff the plan can produce for max_ir_len
    cpq_nuc_plan pl;
    if (cpq::computeNucPlan(d->max_ir_len, d->block_size, false, nullptr, &pl) != CPQ_OK) {
        delete e;
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "cannot plan max_ir_len=%d", d->max_ir_len);
    }
    const int taps = (d->semantics == CPQ_SEM_REFERENCE) ? std::max(pl.heff_len, d->max_ir_len) : d->max_ir_len;
    // engines whose every stream runs in a plan group (engine_native.cpp) keep only a token main-path arena
    const bool allNative = anyCalls || d->schedule == CPQ_SCHED_REFERENCE_NUC;
    const int kReal = allNative ? 1 : (taps + e->P - 1) / e->P;
    e->kCap = (int)alignUp(kReal, cpq::kMacMaxTile);
    e->hRows = e->kCap + 4 * cpq::kMacMaxTile;   // zero rows read by the prefetch past the last partition (per layer in layered mode)
    e->ringSlots = nextPow2(e->kCap + cpq::kMacMaxTile + e->tMax);
    e->heffCap = std::max<int64_t>((int64_t)e->kCap * e->P, d->max_ir_len);

    // ---- arena layout
    const int64_t nCh = e->nCh;
    {
        int nCu = 0;
        if (hipDeviceGetAttribute(&nCu, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess) { (void)hipGetLastError(); nCu = 0; }
        e->svfChainGrid = 2 * nCu;          // the span kernel keeps 76 KB of LDS: two workgroups per CU
    }
    // One workgroup per channel runs whole rounds of svfChainGrid workgroups: a last round of r workgroups costs 0.70 of a full
    // one up to half the slots (the workgroups are alone on their CUs) and a whole one beyond.  Chained spans deal (span,
    // channel) tasks to the slots whatever the count, at 6 % more per task (hand-over polls, tables per task).  Measured
    // (profiles/r04x_eq_stream_counts.txt): 300 streams 7.63 -> chained; 255 / 256 / 512 / 1024 streams stay as they are.
    bool chained = false;
    if (e->svfChainGrid > 0 && e->maxCall >= 2 * 8192) {
        const int64_t full = nCh / e->svfChainGrid, r = nCh % e->svfChainGrid;
        const double perChannel = (double)full + (r == 0 ? 0.0 : (2 * r <= e->svfChainGrid ? 0.70 : 1.0));
        chained = 1.06 * (double)nCh / (double)e->svfChainGrid < perChannel;
    }
    std::vector<ArenaItem> items = {
        { (void**)&e->X, nCh * e->ringSlots * e->P * (int64_t)sizeof(double2) },
        { (void**)&e->XDN, nCh * e->ringSlots * (int64_t)sizeof(double2) },
        { (void**)&e->H, nCh * e->hRows * e->P * (int64_t)sizeof(double2) },
        { (void**)&e->HDN, nCh * e->hRows * (int64_t)sizeof(double2) },
        { (void**)&e->Y, nCh * e->tMax * e->P * (int64_t)sizeof(double2) },
        { (void**)&e->hist[0], nCh * e->P * (int64_t)sizeof(double) },
        { (void**)&e->hist[1], nCh * e->P * (int64_t)sizeof(double) },
        { (void**)&e->heffDev, e->heffCap * (int64_t)sizeof(double) },
        { (void**)&e->gainDev, (e->P + 1) * (int64_t)sizeof(double) },
        { (void**)&e->tw512, e->P * (int64_t)sizeof(double2) },
        { (void**)&e->tw1024, e->P * (int64_t)sizeof(double2) },
        { (void**)&e->irSlot, nCh * (int64_t)sizeof(int) },
    };
    cascadeSlices(e->eqTab, nCh, items);
    cascadeSlices(e->ofTab, nCh, items);
    // scheduling words of the time-parallel cascade (svf_kernels.hip): header, the arrival counters of the CUs, and -- only
    // for engines that chain their spans (the rule above) -- the band states handed from span to span
    items.push_back({ (void**)&e->svfChain, (int64_t)cpq::svf_chain_bytes((int)nCh, chained ? e->maxCall : 0) });
    e->svfChainSpans = chained ? cpq::svf_chain_spans(e->maxCall) : 0;
    int64_t total = 0;
    for (const ArenaItem& it : items) total += alignUp(it.bytes, 256);
    if (!e->arena.alloc((size_t)total)) {
        delete e;
        return fail(nullptr, CPQ_ERR_OOM, "device arena of %lld bytes could not be allocated", (long long)total);
    }
    e->arenaBytes = total;
    int64_t off = 0;
    for (const ArenaItem& it : items) { *it.ptr = e->arena + off; off += alignUp(it.bytes, 256); }

    // everything starts zero: FDL, history, IR spectra (incl. padding rows), SVF state
    if (hipMemset(e->arena, 0, (size_t)total) != hipSuccess) {
        cpq_engine_destroy(e);
        return fail(nullptr, CPQ_ERR_DEVICE, "hipMemset of the arena failed");
    }
    std::vector<double2> w512, w1024;
    hostTwiddles(e->P, w512, w1024);
    if (hipMemcpy(e->tw512, w512.data(), e->P * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(e->tw1024, w1024.data(), e->P * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess) {
        cpq_engine_destroy(e);
        return fail(nullptr, CPQ_ERR_DEVICE, "twiddle upload failed");
    }
    e->irSlotHost.assign(e->nCh, 0);
    for (int c = 0; c < e->nCh; ++c) e->irSlotHost[c] = c;
    e->irLoaded.assign(e->nCh, 0);
    e->irParts.assign(e->nCh, 0);
    e->groupOf.assign(d->n_streams, -1);
    e->eqTpSafe.assign(d->n_streams, 1);   // no active band yet: trivially guard-free
    e->eqMidSide.assign(d->n_streams, 0);
    e->eqParamsHost.assign(d->n_streams, cpq_eq_params{});
    e->eqParamsSet.assign(d->n_streams, 0);
    e->eqBypass.assign(d->n_streams, EqBypass{});
    e->eqResetPending.assign(d->n_streams, 0u);
    e->agcResetPending.assign(d->n_streams, 0);
    e->latFade.assign(d->n_streams, LatencyFade{});
    e->trimHost.assign(d->n_streams, 1.0);
    e->makeupHost.assign(d->n_streams, 1.0);
    e->ofPass.assign(d->n_streams, 0);
    e->ofModesHost.assign(d->n_streams, cpq_engine::OfModes{ 0, 1, 0, 1 });
    e->ofModesSet.assign(d->n_streams, 0);
    e->procParams.assign(d->n_streams, cpq_convproc_params{ 1.0f, 0, 0, 0.0f });
    e->procBypass.assign(d->n_streams, 0);
    e->procDryOnly.assign(d->n_streams, 0);
    e->mixRamp.assign(d->n_streams, MixRamp{});
    e->agcOnHost.assign(d->n_streams, 0);
    e->gainRamp.assign(d->n_streams, GainRamp{});
    e->scOnHost.assign(d->n_streams, 0);
    e->scAmountHost.assign(d->n_streams, 0.0f);
    if (hipMemcpy(e->irSlot, e->irSlotHost.data(), sizeof(int) * e->nCh, hipMemcpyHostToDevice) != hipSuccess) {
        cpq_engine_destroy(e);
        return fail(nullptr, CPQ_ERR_DEVICE, "irSlot upload failed");
    }
    *out = e;
    return CPQ_OK;
}

void cpq_engine_destroy(cpq_engine* e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    for (auto& s : e->prof) {
        for (auto& ev : s.pending) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
        for (auto& ev : s.freeList) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    }
    freePinnedRing(e);      // its events
    if (e->copyIn) {
        (void)hipStreamDestroy(e->copyIn);
        (void)hipStreamDestroy(e->copyOut);
        for (int i = 0; i < 4; ++i) { (void)hipEventDestroy(e->evIn[i]); (void)hipEventDestroy(e->evDone[i]); }
    }
    delete e;
}

int32_t cpq_engine_set_stream(cpq_engine* e, void* s)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    e->stream = reinterpret_cast<hipStream_t>(s);
    return CPQ_OK;
}

int32_t cpq_engine_synchronize(cpq_engine* e)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

int64_t cpq_engine_arena_bytes(const cpq_engine* e) { return e ? e->arenaBytes : 0; }
int32_t cpq_engine_partition_size(const cpq_engine* e) { return e ? e->P : 0; }

int32_t cpq_engine_prepare(cpq_engine* e, double sampleRate, int32_t maxBlock)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (sampleRate <= 0.0) return fail(e, CPQ_ERR_INVALID_ARG, "sample rate must be positive");
    if (maxBlock <= 0 || maxBlock > e->maxCall)
        return fail(e, CPQ_ERR_INVALID_ARG, "max_block %d exceeds block_size*max_blocks_per_call", maxBlock);
    if (e->osFactor > 1 && sampleRate > 768000.0)
        return fail(e, CPQ_ERR_INVALID_ARG, "processing rate %.1f Hz above 768 kHz with oversampling factor %d", sampleRate, e->osFactor);
    const bool rateChanged = sampleRate != e->sampleRate;
    e->sampleRate = sampleRate;
    if (rateChanged) {
        // coefficients follow the rate: re-design what was set (one call when every stream shares the parameters)
        const int S = e->desc.n_streams;
        bool same = S > 0 && e->eqParamsSet[0];
        for (int s = 1; s < S && same; ++s)
            same = e->eqParamsSet[s] && std::memcmp(&e->eqParamsHost[s], &e->eqParamsHost[0], sizeof(cpq_eq_params)) == 0;
        if (same) {
            const cpq_eq_params p = e->eqParamsHost[0];
            CPQ_TRY(cpq_eq_set_params(e, CPQ_ALL_STREAMS, &p));
        } else {
            for (int s = 0; s < S; ++s)
                if (e->eqParamsSet[s]) {
                    const cpq_eq_params p = e->eqParamsHost[s];
                    CPQ_TRY(cpq_eq_set_params(e, s, &p));
                }
        }
        for (int s = 0; s < S; ++s)
            if (e->ofModesSet[s]) {
                const auto m = e->ofModesHost[s];
                CPQ_TRY(cpq_outfilter_set_params(e, s, m.convIsLast, m.hc, m.lc, m.lp));
            }
    }
    e->eqProcessed = false;
    e->procProcessed = false;
    syncEqBypass(e);
    for (size_t s = 0; s < e->mixRamp.size(); ++s) e->mixRamp[s].ramp.setCurrentAndTargetValue((double)e->procParams[s].mix);   // Lifecycle.cpp:370-371
    for (auto& r : e->gainRamp) r.snap();       // setCurrentAndTargetValue (Core.cpp:765)
    CPQ_TRY(resetOversampler(e));       // oversampling.prepare -> release(): histories and flags cleared, counters kept
    CPQ_TRY(resetSoftClipStage(e));     // softClipOS.prepareSingleStage -> release(): the same for the clipper's local 2x stage
    CPQ_TRY(refreshBaseRateStages(e));
    return zeroRuntimeState(e, true, true);
}

int32_t cpq_host_register(void* ptr, size_t bytes)
{
    if (!ptr || bytes == 0) return CPQ_ERR_INVALID_ARG;
    return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? CPQ_OK : CPQ_ERR_DEVICE;
}

int32_t cpq_host_unregister(void* ptr)
{
    if (!ptr) return CPQ_ERR_INVALID_ARG;
    return hipHostUnregister(ptr) == hipSuccess ? CPQ_OK : CPQ_ERR_DEVICE;
}

int32_t cpq_engine_set_order(cpq_engine* e, int32_t order)
{
    if (!e || (order != CPQ_ORDER_CONV_THEN_EQ && order != CPQ_ORDER_EQ_THEN_CONV)) return CPQ_ERR_INVALID_ARG;
    e->order = order;
    return CPQ_OK;
}


}  // extern "C"

// ------------------------------------------------------------------------ whole path
int cpqi::enqueueBoth(cpq_engine* e, const double* a, double* b, int n)
{
    int rc = CPQ_OK;
    auto conv = [e](const double* x, double* y, int t) {
        return e->convLevel == CPQ_LEVEL_PROCESSOR ? enqueueConvProc(e, x, y, t) : enqueueConv(e, x, y, t);
    };
    if (e->order == CPQ_ORDER_CONV_THEN_EQ) {
        if (!e->convBypassed) rc = conv(a, b, n);
        else if (a != b) cpq::launch_rows_copy(e->stream, a, n, 0, b, n, 0, n, e->nCh);
        if (rc == CPQ_OK) rc = enqueueEq(e, b, b, n);
    } else if (e->convBypassed) {
        rc = enqueueEq(e, a, b, n);
    } else {
        rc = ensureCallBuffer(e, e->mid, "EQ -> convolver hand-off");
        if (rc == CPQ_OK) rc = enqueueEq(e, a, e->mid, n);
        if (rc == CPQ_OK && e->anyTrim) {       // scaleBlockFallback(block, convolverInputTrimGain) (:440-447)
            ProfScope p(e, CPQ_K_MIX);
            cpq::launch_rows_scale(e->stream, e->mid, n, n, e->nCh, e->trimDev);
        }
        if (rc == CPQ_OK) rc = conv(e->mid, b, n);
    }
    if (rc == CPQ_OK && e->ofInPath) {
        // outputFilter.process runs when the convolver or the EQ is active (:453-463); a stream with both bypassed
        // keeps its filter state untouched
        bool anyActive = false;
        for (int s = 0; s < e->desc.n_streams; ++s) {
            const char pass = (e->convBypassed && e->eqBypass[s].requested) ? 1 : 0;
            anyActive = anyActive || !pass;
            if (pass == e->ofPass[s] || !e->ofModesSet[s]) continue;
            CPQ_TRY(setOutFilterPass(e, s, pass != 0));
        }
        if (anyActive) rc = enqueueOutFilter(e, b, b, n);
    }
    if (rc == CPQ_OK && e->anyMakeup) {         // scaleBlockFallback(block, outputMakeupGain) (:465-469)
        ProfScope p(e, CPQ_K_MIX);
        cpq::launch_rows_scale(e->stream, b, n, n, e->nCh, e->makeupDev);
        CPQ_HIP(e, hipGetLastError());
    }
    return rc;
}

extern "C" {

int32_t cpq_engine_set_gains(cpq_engine* e, int32_t stream, double convInputTrimGain, double outputMakeupGain)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    int s0 = 0, s1 = 0;
    CPQ_TRY(streamRange(e, stream, s0, s1));
    if (!std::isfinite(convInputTrimGain) || !std::isfinite(outputMakeupGain))
        return fail(e, CPQ_ERR_INVALID_ARG, "gains must be finite");
    CPQ_HIP(e, hipSetDevice(e->device));
    const int S = e->desc.n_streams;
    if (!e->trimDev) {
        CPQ_TRY(allocAll(e, { { e->trimDev, (size_t)S }, { e->makeupDev, (size_t)S } }, "gain buffers could not be allocated"));
    }
    for (int s = s0; s < s1; ++s) {
        // the trim is applied only when it differs from 1 by more than 1e-12 (:440)
        e->trimHost[s] = std::fabs(convInputTrimGain - 1.0) > 1e-12 ? convInputTrimGain : 1.0;
        e->makeupHost[s] = outputMakeupGain;
    }
    e->anyTrim = e->anyMakeup = false;
    for (int s = 0; s < S; ++s) { e->anyTrim = e->anyTrim || e->trimHost[s] != 1.0; e->anyMakeup = e->anyMakeup || e->makeupHost[s] != 1.0; }
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    CPQ_HIP(e, hipMemcpy(e->trimDev, e->trimHost.data(), sizeof(double) * S, hipMemcpyHostToDevice));
    CPQ_HIP(e, hipMemcpy(e->makeupDev, e->makeupHost.data(), sizeof(double) * S, hipMemcpyHostToDevice));
    return CPQ_OK;
}

int32_t cpq_engine_set_conv_bypass(cpq_engine* e, int32_t bypassed)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    e->convBypassed = bypassed != 0;
    return CPQ_OK;
}

}  // extern "C"

// the meters read the base-rate rows the call delivers, after everything that writes them (DSPCoreDouble.cpp:695-701); with
// the output stage on that is where the reference's meters sit: after the scrub (:665-693), before the limiter (:703-710)
int cpqi::meteredChain(cpq_engine* e, const double* a, double* b, int n)
{
    const bool localClip = e->osFactor == 1 && e->anySoftClip;       // factor > 1: enqueueOsChain clips the oversampled block
    if (localClip) CPQ_TRY(ensureSoftClipStage(e));                   // what the local 2x stage owns, before anything is enqueued
    int rc = e->osFactor > 1 ? enqueueOsChain(e, a, b, n) : enqueueBoth(e, a, b, n);
    if (rc == CPQ_OK && localClip) rc = enqueueSoftClipLocal(e, b, n);
    const bool dither = e->ditherShaper != CPQ_DITHER_OFF;            // the shaper then applies the headroom and the scrub itself
    if (rc == CPQ_OK) rc = enqueueOutPre(e, b, n, b, n, n, !dither);  // each half returns at once when its flags are off
    if (rc == CPQ_OK && dither) rc = enqueueDither(e, b, n, b, n, n);
    if (rc == CPQ_OK && e->meterFlags) rc = enqueueMeters(e, b, n, n);
    if (rc == CPQ_OK) rc = enqueueOutPost(e, b, n, b, n, n);
    return rc;
}

// n_samples of the whole-chain call are base-rate samples: the routing runs on n_samples * factor, which the call limit bounds
static int checkOversampledLimit(cpq_engine* e, int nSamples)
{
    if (e && e->osFactor > 1 && nSamples > e->maxCall / e->osFactor)
        return fail(e, CPQ_ERR_INVALID_ARG, "n_samples=%d times the oversampling factor %d exceeds the call limit %d", nSamples,
                    e->osFactor, e->maxCall);
    return CPQ_OK;
}

int cpqi::checkBlockCall(cpq_engine* e, const void* in, const void* out, int nSamples)
{
    CPQ_TRY(checkOversampledLimit(e, nSamples));
    CPQ_TRY(checkCall(e, in, out, nSamples * (e ? e->osFactor : 1)));
    return checkMeterCall(e, nSamples);
}

extern "C" {

int32_t cpq_engine_process_block_device(cpq_engine* e, const double* dIn, double* dOut, int32_t nSamples)
{
    CPQ_TRY(checkBlockCall(e, dIn, dOut, nSamples));
    CPQ_HIP(e, hipSetDevice(e->device));
    return meteredChain(e, dIn, dOut, nSamples);
}

int32_t cpq_engine_process_block(cpq_engine* e, const double* in, double* out, int32_t nSamples)
{
    CPQ_TRY(checkOversampledLimit(e, nSamples));
    if (e && nSamples > 0) CPQ_TRY(checkMeterCall(e, nSamples));    // before checkCall here, after it in the device variant
    return viaStaging(e, in, out, nSamples, [e](const double* a, double* b, int n) { return meteredChain(e, a, b, n); },
                      e ? e->osFactor : 1);
}

// -------------------------------------------------------------------------- profiling
int32_t cpq_profile_enable(cpq_engine* e, int32_t on)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    e->profiling = on != 0;
    if (e->profiling) {
        // event pool up front, so that no hipEventCreate runs inside a timed region (ProfScope only creates on exhaustion)
        CPQ_HIP(e, hipSetDevice(e->device));
        constexpr size_t kPool = 96;
        for (auto& s : e->prof)
            while (s.freeList.size() + s.pending.size() < kPool) {
                std::pair<hipEvent_t, hipEvent_t> ev;
                CPQ_HIP(e, hipEventCreate(&ev.first));
                CPQ_HIP(e, hipEventCreate(&ev.second));
                s.freeList.push_back(ev);
            }
    }
    return CPQ_OK;
}

static int drainProfile(cpq_engine* e)
{
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    for (auto& s : e->prof) {
        for (auto& ev : s.pending) {
            float ms = 0.0f;
            CPQ_HIP(e, hipEventElapsedTime(&ms, ev.first, ev.second));
            s.totalMs += ms;
            s.launches += 1;
            s.freeList.push_back(ev);
        }
        s.pending.clear();
    }
    return CPQ_OK;
}

int32_t cpq_profile_reset(cpq_engine* e)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    const int rc = drainProfile(e);
    for (auto& s : e->prof) { s.launches = 0; s.totalMs = 0.0; }
    return rc;
}

int32_t cpq_profile_read(cpq_engine* e, int32_t id, int64_t* launches, double* totalMs)
{
    if (!e || id < 0 || id >= CPQ_K_COUNT) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(drainProfile(e));
    if (launches) *launches = e->prof[id].launches;
    if (totalMs) *totalMs = e->prof[id].totalMs;
    return CPQ_OK;
}

}  // extern "C"
