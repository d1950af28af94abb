// engine_diag.cpp -- the launchers of mix_kernels.hip in isolation (tests/test_gpu_mix_kernels.py): cpq_diag_direct_head, _agc,
// _ring_chunks, _convproc_mix, _tail_reader and _rows of include/convopeq_mi355x.h.  Same conventions as the FFT and MAC
// diagnostics of engine_core.cpp: host pointers, own device buffers of exactly the documented sizes, the null stream, no engine;
// what a kernel may write is filled with 0xFF bytes unless the caller supplies its contents, and comes back whole; every
// argument set with which a kernel would leave a buffer is refused before anything is allocated or a device is looked for.
#include "engine_internal.hpp"

namespace {

using cpqi::DeviceBuffer;

constexpr size_t kMaxElems = (size_t)1 << 28;      // per buffer: test tools
constexpr long long kMaxPos = 1LL << 62;           // ring positions, cursors and schedule entries

bool pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }
bool fits(long long a, long long b) { return a >= 0 && b >= 0 && (b == 0 || a <= (long long)kMaxElems / b); }      // a * b <= 2^28
bool haveDevice()
{
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || nDev <= 0) { (void)hipGetLastError(); return false; }
    return true;
}

// the device buffers of one diagnostic call: one allocation each, of exactly the size asked for (an empty one holds one element)
struct Scope {
    std::vector<DeviceBuffer<char>> bufs;
    int32_t rc = CPQ_OK;
    bool ok(hipError_t err)
    {
        if (err != hipSuccess && rc == CPQ_OK) { (void)hipGetLastError(); rc = CPQ_ERR_DEVICE; }
        return err == hipSuccess;
    }
    // host == nullptr: filled with `fill` bytes
    template <typename T> T* put(const T* host, size_t count, int fill = 0xFF)
    {
        if (rc != CPQ_OK) return nullptr;
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        bufs.emplace_back();
        if (!bufs.back().allocBytes(bytes)) { rc = CPQ_ERR_DEVICE; return nullptr; }
        T* p = reinterpret_cast<T*>(bufs.back().get());
        if (host && count) ok(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
        else ok(hipMemset(p, fill, bytes));
        return p;
    }
    template <typename T> void get(T* host, const T* dev, size_t count)
    {
        if (rc == CPQ_OK && host && count) ok(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
    }
    bool launched()
    {
        ok(hipGetLastError());
        ok(hipDeviceSynchronize());
        return rc == CPQ_OK;
    }
};

const long long* ll(const int64_t* p) { return reinterpret_cast<const long long*>(p); }
static_assert(sizeof(long long) == sizeof(int64_t), "tables travel as long long");

// chMap: every entry -1 or a row below `rows`, no row named twice
bool chMapValid(const int32_t* chMap, int nCh, int rows)
{
    for (int c = 0; c < nCh; ++c) {
        if (chMap[c] < -1 || chMap[c] >= rows) return false;
        for (int u = 0; u < c; ++u)
            if (chMap[c] >= 0 && chMap[u] == chMap[c]) return false;
    }
    return true;
}

}  // namespace

extern "C" {

int32_t cpq_diag_direct_head(int32_t nCh, int32_t n, int64_t inStride, int32_t nSlots, const double* in, const double* irRev,
                             const int32_t* taps, const int32_t* irSlot, const double* histOld, const int32_t* wetOn, double* dout,
                             double* histNew, double* out, int64_t outStride)
{
    if (!in || !irRev || !taps || !irSlot || !histOld || !dout || !histNew) return CPQ_ERR_INVALID_ARG;
    if (nCh < 1 || nSlots < 1 || n < 1 || n > inStride) return CPQ_ERR_INVALID_ARG;
    if (wetOn && (nCh & 1)) return CPQ_ERR_INVALID_ARG;
    if (out && outStride < n) return CPQ_ERR_INVALID_ARG;
    if (!fits(nCh, inStride) || !fits(nSlots, 32) || (out && !fits(nCh, outStride))) return CPQ_ERR_INVALID_ARG;
    for (int s = 0; s < nSlots; ++s)
        if (taps[s] < 0 || taps[s] > 32) return CPQ_ERR_INVALID_ARG;
    for (int c = 0; c < nCh; ++c)
        if (irSlot[c] < 0 || irSlot[c] >= nSlots) return CPQ_ERR_INVALID_ARG;
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const size_t nIn = (size_t)nCh * inStride, nOut = out ? (size_t)nCh * outStride : 0;
    const double* dIn = d.put(in, nIn);
    const double* dIr = d.put(irRev, (size_t)nSlots * 32);
    const int* dTaps = d.put(taps, nSlots);
    const int* dSlot = d.put(irSlot, nCh);
    const double* dHistOld = d.put(histOld, (size_t)nCh * 32);
    const int* dWetOn = wetOn ? d.put(wetOn, nCh / 2) : nullptr;
    double* dDout = d.put<double>(nullptr, (size_t)nCh * n);
    double* dHistNew = d.put<double>(nullptr, (size_t)nCh * 32);
    double* dOut = out ? d.put(out, nOut) : nullptr;
    if (d.rc == CPQ_OK) {
        cpq::launch_direct_head(nullptr, dIn, inStride, n, dIr, dTaps, dSlot, dHistOld, dHistNew, dDout, nCh, dWetOn);
        if (out) cpq::launch_rows_add(nullptr, dOut, outStride, dDout, n, nCh);
        d.launched();
    }
    d.get(dout, dDout, (size_t)nCh * n);
    d.get(histNew, dHistNew, (size_t)nCh * 32);
    d.get(out, dOut, nOut);
    return d.rc;
}

int32_t cpq_diag_agc(int32_t op, int32_t nCh, int32_t B, int32_t T, int64_t chStride, double* data, const double* rmsIn,
                     const double* rmsOut, double* state, const int32_t* on, double* gains, double bAtt, double bRel, double bSm,
                     double* rms, int32_t* silent)
{
    if (op < 0 || op > 3 || !data) return CPQ_ERR_INVALID_ARG;
    if (nCh < 1 || B < 1 || T < 1 || !fits(B, T) || chStride < (int64_t)B * T || !fits(nCh, chStride)) return CPQ_ERR_INVALID_ARG;
    const int S = nCh / 2;
    if (op != 0 && ((nCh & 1) || S < 1)) return CPQ_ERR_INVALID_ARG;
    if (op == 0 && !rms) return CPQ_ERR_INVALID_ARG;
    if (op == 1 && (!rmsIn || !rmsOut || !state || !on || !gains)) return CPQ_ERR_INVALID_ARG;
    if (op == 2 && (!on || !gains)) return CPQ_ERR_INVALID_ARG;
    if (op == 3 && !silent) return CPQ_ERR_INVALID_ARG;
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const size_t nData = (size_t)nCh * chStride, nRms = (size_t)nCh * T, nGains = (size_t)S * T * 2;
    double* dData = d.put(data, nData);
    if (op == 0) {
        double* dRms = d.put<double>(nullptr, nRms);
        if (d.rc == CPQ_OK) { cpq::launch_agc_block_rms(nullptr, dData, chStride, nCh, B, T, dRms); d.launched(); }
        d.get(rms, dRms, nRms);
    } else if (op == 1) {
        const double* dRmsIn = d.put(rmsIn, nRms);
        const double* dRmsOut = d.put(rmsOut, nRms);
        double* dState = d.put(state, (size_t)S * 3);
        const int* dOn = d.put(on, S);
        double* dGains = d.put<double>(nullptr, nGains);
        if (d.rc == CPQ_OK) {
            cpq::launch_agc_apply(nullptr, dData, chStride, S, B, T, dRmsIn, dRmsOut, dState, dOn, dGains, bAtt, bRel, bSm);
            d.launched();
        }
        d.get(state, dState, (size_t)S * 3);
        d.get(gains, dGains, nGains);
    } else if (op == 2) {
        const double* dGains = d.put(gains, nGains);
        const int* dOn = d.put(on, S);
        if (d.rc == CPQ_OK) { cpq::launch_gain_ramp(nullptr, dData, chStride, S, B, T, dGains, dOn); d.launched(); }
    } else {
        int* dSilent = d.put<int>(nullptr, (size_t)S * T);
        if (d.rc == CPQ_OK) { cpq::launch_block_silence(nullptr, dData, chStride, B, T, S, dSilent); d.launched(); }
        d.get(silent, dSilent, (size_t)S * T);
    }
    d.get(data, dData, nData);
    return d.rc;
}

int32_t cpq_diag_ring_chunks(int32_t op, int32_t rows, int32_t nCh, int32_t n, int32_t q, int64_t outStride, double* out,
                             const int32_t* chMap, const double* ring0, int32_t size0, const int64_t* pos, const int64_t* cnt,
                             const double* ringA, int32_t sizeA, const int64_t* schedA, double gainA, const double* ringB,
                             int32_t sizeB, const int64_t* schedB, double gainB, int32_t nDst, const int64_t* dstStride,
                             const int64_t* dstOff, double* dst0, double* dst1, double* dst2, const int64_t* tab, int32_t nTab,
                             int64_t* tabOut)
{
    if (op < 0 || op > 4 || !out || !chMap) return CPQ_ERR_INVALID_ARG;
    if (rows < 1 || nCh < 1 || n < 1 || q < 1 || outStride < n || !fits(rows, outStride)) return CPQ_ERR_INVALID_ARG;
    if (!chMapValid(chMap, nCh, rows)) return CPQ_ERR_INVALID_ARG;
    const int nCb = (int)(((int64_t)n + q - 1) / q);
    double* dstHost[3] = { dst0, dst1, dst2 };
    auto ringValid = [&](const double* r, int size) { return r && pow2(size) && size >= 2 && fits(nCh, size); };
    auto schedValid = [&](const int64_t* s) {
        if (!s) return false;
        for (int i = 0; i < nCb; ++i) if (s[i] > kMaxPos) return false;
        return true;
    };
    const bool useGet = op == 1 || op == 4, useA = op >= 2, useB = op == 3 || (op == 4 && ringB);
    if (op == 0) {
        if (nDst < 1 || nDst > 3 || !dstStride || !dstOff || nTab < 0 || nTab > cpq::kGatherTabMax || (nTab > 0 && (!tab || !tabOut)))
            return CPQ_ERR_INVALID_ARG;
        for (int l = 0; l < nDst; ++l)
            if (!dstHost[l] || dstOff[l] < 0 || dstOff[l] > dstStride[l] - n || !fits(nCh, dstStride[l])) return CPQ_ERR_INVALID_ARG;
    }
    if (useGet) {
        if (!ringValid(ring0, size0) || !pos || !cnt) return CPQ_ERR_INVALID_ARG;
        for (int i = 0; i < nCb; ++i)
            if (cnt[i] < 0 || cnt[i] > q || pos[i] < 0 || pos[i] > kMaxPos) return CPQ_ERR_INVALID_ARG;
    }
    if (useA && (!ringValid(ringA, sizeA) || !schedValid(schedA))) return CPQ_ERR_INVALID_ARG;
    if (useB && (!ringValid(ringB, sizeB) || !schedValid(schedB))) return CPQ_ERR_INVALID_ARG;
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const size_t nOut = (size_t)rows * outStride;
    double* dOut = d.put(out, nOut);
    const int* dMap = d.put(chMap, nCh);
    if (op == 0) {
        double* dDst[3] = { nullptr, nullptr, nullptr };
        for (int l = 0; l < nDst; ++l) dDst[l] = d.put<double>(nullptr, (size_t)nCh * dstStride[l]);
        long long* dTab = d.put<long long>(nullptr, cpq::kGatherTabMax);
        if (d.rc == CPQ_OK) {
            cpq::launch_rows_gather_multi(nullptr, dOut, outStride, dMap, nDst, dDst, dstStride, dstOff, n, nCh, dTab, ll(tab), nTab);
            d.launched();
        }
        for (int l = 0; l < nDst; ++l) d.get(dstHost[l], dDst[l], (size_t)nCh * dstStride[l]);
        d.get(reinterpret_cast<long long*>(tabOut), dTab, cpq::kGatherTabMax);
    } else {
        const double* dRing0 = useGet ? d.put(ring0, (size_t)nCh * size0) : nullptr;
        const long long* dPos = useGet ? d.put(ll(pos), nCb) : nullptr;
        const long long* dCnt = useGet ? d.put(ll(cnt), nCb) : nullptr;
        const double* dRingA = useA ? d.put(ringA, (size_t)nCh * sizeA) : nullptr;
        const long long* dSchedA = useA ? d.put(ll(schedA), nCb) : nullptr;
        const double* dRingB = useB ? d.put(ringB, (size_t)nCh * sizeB) : nullptr;
        const long long* dSchedB = useB ? d.put(ll(schedB), nCb) : nullptr;
        if (d.rc == CPQ_OK) {
            if (op == 1) cpq::launch_ring_get_chunks(nullptr, dOut, outStride, dMap, n, q, dRing0, size0, dPos, dCnt, nCh);
            else if (op == 2) cpq::launch_ring_add_chunks(nullptr, dOut, outStride, dMap, n, q, dRingA, sizeA, dSchedA, gainA, nCh);
            else if (op == 3)
                cpq::launch_ring_add_chunks2(nullptr, dOut, outStride, dMap, n, q, dRingA, sizeA, dSchedA, gainA, dRingB, sizeB, dSchedB,
                                             gainB, nCh);
            else
                cpq::launch_ring_get_add_chunks(nullptr, dOut, outStride, dMap, n, q, dRing0, size0, dPos, dCnt, dRingA, sizeA, dSchedA,
                                                gainA, dRingB, useB ? sizeB : 2, dSchedB, gainB, nCh);
            d.launched();
        }
    }
    d.get(out, dOut, nOut);
    return d.rc;
}

int32_t cpq_diag_convproc_mix(int32_t nCh, int32_t n, int64_t chStride, const double* wet, double* out, int32_t inPlace,
                              const double* gains, double* ring, int32_t ringSize, int64_t pos0, const int32_t* dNew,
                              const int32_t* dOld, const int32_t* xLen, const double* xGains, int32_t xCap, int32_t wetValid,
                              const int32_t* rampLen, const double* rampGains, int32_t rampCap, int32_t rampOff, const int32_t* wetOn,
                              const double* oldRing, int32_t oldSize, int64_t regrowEnd, const double* ringIn, int64_t ringInStride,
                              int32_t nPut)
{
    if (!wet || !out || !gains || !ring || !dNew || !dOld) return CPQ_ERR_INVALID_ARG;
    if (nCh < 2 || (nCh & 1) || n < 0 || chStride < 1 || chStride < n || !fits(nCh, chStride)) return CPQ_ERR_INVALID_ARG;
    if (!pow2(ringSize) || ringSize < 2 || !fits(nCh, ringSize) || pos0 < 0 || pos0 > kMaxPos) return CPQ_ERR_INVALID_ARG;
    const int S = nCh / 2;
    for (int s = 0; s < S; ++s)
        if (dNew[s] < 0 || dNew[s] >= ringSize || dOld[s] < 0 || dOld[s] >= ringSize) return CPQ_ERR_INVALID_ARG;
    if (xLen) {
        if (!xGains || xCap < 1 || !fits(S, xCap)) return CPQ_ERR_INVALID_ARG;
        for (int s = 0; s < S; ++s)
            if (xLen[s] < 0 || xLen[s] > std::min(n, xCap)) return CPQ_ERR_INVALID_ARG;
    }
    if (rampLen) {
        if (!rampGains || rampCap < 1 || !fits(S, 2LL * rampCap) || rampOff < 0) return CPQ_ERR_INVALID_ARG;
        for (int s = 0; s < S; ++s)
            if ((int64_t)rampLen[s] - rampOff > (int64_t)rampCap - rampOff) return CPQ_ERR_INVALID_ARG;
    }
    if (oldRing && (!pow2(oldSize) || oldSize < 2 || ringSize < oldSize || regrowEnd < 0 || regrowEnd > kMaxPos)) return CPQ_ERR_INVALID_ARG;
    if (ringIn && (nPut < 1 || nPut > ringInStride || nPut > ringSize || !fits(nCh, ringInStride))) return CPQ_ERR_INVALID_ARG;
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const size_t nRows = (size_t)nCh * chStride, nRing = (size_t)nCh * ringSize;
    double* dWet = d.put(wet, nRows);
    double* dOut = inPlace ? dWet : d.put<double>(nullptr, nRows);
    const double* dGains = d.put(gains, (size_t)S * 2);
    double* dRing = oldRing ? d.put<double>(nullptr, nRing, 0) : d.put(ring, nRing);      // regrow: into a zeroed ring
    const double* dOldRing = oldRing ? d.put(oldRing, (size_t)nCh * oldSize) : nullptr;
    const double* dRingIn = ringIn ? d.put(ringIn, (size_t)nCh * ringInStride) : nullptr;
    const int* dDNew = d.put(dNew, S);
    const int* dDOld = d.put(dOld, S);
    const int* dXLen = xLen ? d.put(xLen, S) : nullptr;
    const double* dXGains = xLen ? d.put(xGains, (size_t)S * xCap) : nullptr;
    const int* dRampLen = rampLen ? d.put(rampLen, S) : nullptr;
    const double* dRampGains = rampLen ? d.put(rampGains, (size_t)S * rampCap * 2) : nullptr;
    const int* dWetOn = wetOn ? d.put(wetOn, S) : nullptr;
    if (d.rc == CPQ_OK) {
        if (oldRing) cpq::launch_ring_regrow(nullptr, dOldRing, oldSize, dRing, ringSize, regrowEnd, nCh);
        if (ringIn) cpq::launch_ring_put(nullptr, dRingIn, ringInStride, nPut, dRing, ringSize, pos0, nCh);
        cpq::launch_convproc_mix(nullptr, dWet, dOut, chStride, nCh, n, dGains, dRing, ringSize, pos0, dDNew, dDOld, dXLen, dXGains,
                                 xLen ? xCap : 0, wetValid, dRampLen, dRampGains, rampLen ? rampCap : 0, rampLen ? rampOff : 0, dWetOn);
        d.launched();
    }
    d.get(out, dOut, nRows);
    d.get(ring, dRing, nRing);
    return d.rc;
}

int32_t cpq_diag_tail_reader(int32_t nCalls, const int32_t* T, int32_t B, int32_t nTail, int32_t pl1, int32_t ol1, int32_t d1,
                             int32_t pl2, int32_t ol2, int32_t d2, const int64_t* stateIn, int64_t* schedOut, int64_t* statesOut,
                             int32_t nCh, int32_t nSamples, const double* layerOut, double* ring, int32_t ringSize)
{
    if (!T || !stateIn || !schedOut || !statesOut || nCalls < 1 || nCalls > 4096) return CPQ_ERR_INVALID_ARG;
    if (B < 1 || nTail < 1 || nTail > 2) return CPQ_ERR_INVALID_ARG;
    const int pl[2] = { pl1, pl2 }, ol[2] = { ol1, ol2 }, dd[2] = { d1, d2 };
    for (int l = 0; l < nTail; ++l)
        if (pl[l] < B || pl[l] % B != 0 || ol[l] < 0 || dd[l] < 0) return CPQ_ERR_INVALID_ARG;
    long long total = 0;
    for (int i = 0; i < nCalls; ++i) {
        if (T[i] < 1 || T[i] > (1 << 20)) return CPQ_ERR_INVALID_ARG;
        total += T[i];
    }
    if (total > (1 << 20)) return CPQ_ERR_INVALID_ARG;
    for (int i = 0; i < 4; ++i)
        if (stateIn[i] < 0 || stateIn[i] > kMaxPos) return CPQ_ERR_INVALID_ARG;
    if (layerOut && (!ring || nCh < 1 || nSamples < 1 || !pow2(ringSize) || ringSize < 2 || !fits((long long)nTail * nCh, nSamples) ||
                     !fits((long long)nTail * nCh, ringSize)))
        return CPQ_ERR_INVALID_ARG;
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    long long* dState = d.put(ll(stateIn), 4);
    long long* dSched = d.put<long long>(nullptr, (size_t)nTail * total);
    long long* dStates = d.put<long long>(nullptr, (size_t)nCalls * 4);
    const size_t nLayer = layerOut ? (size_t)nTail * nCh * nSamples : 0, nRing = layerOut ? (size_t)nTail * nCh * ringSize : 0;
    const double* dLayer = layerOut ? d.put(layerOut, nLayer) : nullptr;
    double* dRing = layerOut ? d.put(ring, nRing) : nullptr;
    if (d.rc == CPQ_OK) {
        size_t at = 0;
        for (int i = 0; i < nCalls; ++i) {          // call i's schedule: [nTail][T[i]] behind those of the calls before it
            cpq::launch_tail_schedule(nullptr, dState, dSched + at, T[i], B, nTail, pl1, ol1, d1, pl2, ol2, d2);
            d.ok(hipMemcpyAsync(dStates + (size_t)i * 4, dState, 4 * sizeof(long long), hipMemcpyDeviceToDevice, nullptr));
            at += (size_t)nTail * T[i];
        }
        if (layerOut) cpq::launch_tail_append(nullptr, dState, dLayer, dRing, nCh, nSamples, ringSize, nTail);
        d.launched();
    }
    d.get(reinterpret_cast<long long*>(schedOut), dSched, (size_t)nTail * total);
    d.get(reinterpret_cast<long long*>(statesOut), dStates, (size_t)nCalls * 4);
    d.get(ring, dRing, nRing);
    return d.rc;
}

int32_t cpq_diag_rows(int32_t op, int32_t nCh, int32_t n, const double* src, int64_t srcStride, int64_t srcOff, double* dst,
                      int64_t dstStride, int64_t dstOff, const double* gain, const int32_t* on, const int32_t* len,
                      const double* gEnd, const double* gains, int32_t cap)
{
    if (op < 0 || op > 2 || !dst || nCh < 1 || n < 1) return CPQ_ERR_INVALID_ARG;
    if (dstOff < 0 || dstOff > dstStride - n || !fits(nCh, dstStride)) return CPQ_ERR_INVALID_ARG;
    if (op != 1 && (!src || srcOff < 0 || srcOff > srcStride - n || !fits(nCh, srcStride))) return CPQ_ERR_INVALID_ARG;
    if (op != 0 && ((nCh & 1) || srcOff != 0 || dstOff != 0)) return CPQ_ERR_INVALID_ARG;
    const int S = nCh / 2;
    if (op == 1 && !gain) return CPQ_ERR_INVALID_ARG;
    if (op == 2) {
        if (!on || !len || !gEnd || !gains || cap < 1 || !fits(S, cap)) return CPQ_ERR_INVALID_ARG;
        for (int s = 0; s < S; ++s)
            if (len[s] < 0 || len[s] > cap) return CPQ_ERR_INVALID_ARG;
    }
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const size_t nDst = (size_t)nCh * dstStride;
    double* dDst = d.put(dst, nDst);
    if (op == 0) {
        const double* dSrc = d.put(src, (size_t)nCh * srcStride);
        if (d.rc == CPQ_OK) { cpq::launch_rows_copy(nullptr, dSrc, srcStride, srcOff, dDst, dstStride, dstOff, n, nCh); d.launched(); }
    } else if (op == 1) {
        const double* dGain = d.put(gain, S);
        if (d.rc == CPQ_OK) { cpq::launch_rows_scale(nullptr, dDst, dstStride, n, nCh, dGain); d.launched(); }
    } else {
        const double* dSrc = d.put(src, (size_t)nCh * srcStride);
        const int* dOn = d.put(on, S);
        const int* dLen = d.put(len, S);
        const double* dGEnd = d.put(gEnd, S);
        const double* dG = d.put(gains, (size_t)S * cap);
        if (d.rc == CPQ_OK) {
            cpq::launch_bypass_blend(nullptr, dDst, dstStride, dSrc, srcStride, n, nCh, dOn, dLen, dGEnd, dG, cap);
            d.launched();
        }
    }
    d.get(dst, dDst, nDst);
    return d.rc;
}

}  // extern "C"
