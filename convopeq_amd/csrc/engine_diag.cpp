// engine_diag.cpp -- every cpq_diag_* entry of include/convopeq_mi355x.h: launchers on their own, for the tests of single kernels.
//   partition FFT, FDL MAC           cpq_diag_partition_fft(_split), _fdl_mac      tests/test_gpu_fft.py, _fft_p4_frames.py, _fdl_mac.py
//   FFT launch variants, IR spectra  cpq_diag_fft_forward, _fft_inverse_store, _ir_spectra                tests/test_gpu_fft_variants.py
//   mix_kernels.hip                  cpq_diag_direct_head, _agc, _ring_chunks, _convproc_mix, _tail_reader, _rows    test_gpu_mix_kernels.py
//   score_kernels.hip                cpq_diag_score_spectrum, _score_lattice, _score_reduce                 tests/test_gpu_score_kernels.py
//   learn_kernels.hip                cpq_diag_learn_tell                                                    tests/test_gpu_learn_kernels.py
//   prog_kernels.hip                 cpq_diag_prog_finish                                                   tests/test_gpu_prog_finish.py
//   chained EQ spans of an engine    cpq_diag_eq_chain_status                                             tests/test_gpu_eq_chained.py
// One convention for all but the last: host pointers, own device buffers of exactly the documented sizes (Scope), the null
// stream, no engine; what a kernel may write is filled with 0xFF bytes (NaN) unless the caller supplies its contents, and comes
// back whole; every argument set with which a kernel would leave a buffer is refused (CPQ_ERR_INVALID_ARG) before a device is
// looked for (CPQ_ERR_NO_DEVICE) and before anything is allocated; an allocation or HIP failure is CPQ_ERR_DEVICE.  An entry
// reads: validate, put, launch, get.
#include "engine_internal.hpp"

namespace {

using cpqi::DeviceBuffer;
using cpqi::fail;

constexpr size_t kMaxElems = (size_t)1 << 28;      // per buffer: test tools
constexpr long long kMaxPos = 1LL << 62;           // ring positions, cursors and schedule entries

bool pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }
bool partition(int P) { return P >= 64 && P <= 131072 && pow2(P); }
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
const double2* c2(const double* p) { return reinterpret_cast<const double2*>(p); }      // spectra travel as [..][2] doubles
double2* c2(double* p) { return reinterpret_cast<double2*>(p); }

// the twiddle tables of one partition size on the device; second halves (P > 4096): the reordered tables of the four-step transforms
cpq::FftTables twiddles(Scope& d, int P)
{
    std::vector<double2> w1, w2;
    cpqi::hostTwiddles(P, w1, w2);
    w1.resize((size_t)2 * P);
    w2.resize((size_t)2 * P);
    if (P > 4096) cpq::fill_big_twiddles(w1.data(), w2.data(), P, w1.data() + P, w2.data() + P);
    const double2* tw = d.put(w1.data(), w1.size());
    const double2* tw2 = d.put(w2.data(), w2.size());
    if (d.rc != CPQ_OK || P <= 4096) return cpq::FftTables{ tw, tw2 };
    return cpq::FftTables{ tw, tw2, tw + P, tw2 + P };
}

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

// The partition FFT kernels in isolation (tests/test_gpu_fft.py): forward of every overlap-save frame from a silent history,
// inverse of the same spectra.
int32_t cpq_diag_partition_fft(int32_t P, int32_t nCh, int32_t T, const double* in, double* spectra, double* out)
{
    return cpq_diag_partition_fft_split(P, nCh, T, 0, in, spectra, out);
}

// split > 0 at P = 4096: that many workgroups walk the frames of a channel (at most one per frame), so that a small test decides
// how many consecutive frames one workgroup transforms; otherwise the launchers' own choice
int32_t cpq_diag_partition_fft_split(int32_t P, int32_t nCh, int32_t T, int32_t split, const double* in, double* spectra, double* out)
{
    if (P != 4096 || split < 0) split = 0;
    if (split > T || !partition(P) || nCh <= 0 || T <= 0 || !in || !spectra || !out) return CPQ_ERR_INVALID_ARG;
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const int ringSlots = cpqi::nextPow2(T);
    const size_t nTime = (size_t)nCh * T * P, nSpec = (size_t)nCh * ringSlots * P;
    const cpq::FftTables tw = twiddles(d, P);
    const double* dIn = d.put(in, nTime);
    double* dHist = d.put<double>(nullptr, (size_t)2 * nCh * P, 0);
    double2* dX = d.put<double2>(nullptr, nSpec, 0);
    double2* dXdn = d.put<double2>(nullptr, (size_t)nCh * ringSlots);
    double2* dScratch = d.put<double2>(nullptr, P > 4096 ? nTime : 0);
    double2* dY = d.put<double2>(nullptr, nTime);
    double* dOut = d.put<double>(nullptr, nTime);
    if (d.rc == CPQ_OK) {
        cpq::launch_rfft_fwd_ols(nullptr, dIn, (int64_t)T * P, dHist, dHist + (size_t)nCh * P, dX, dXdn, tw, P, nCh, T, 0, ringSlots, dScratch, split);
        // the ring holds block t of channel c at [c][t] of ringSlots slots: [c][t] of T slots for the inverse and the caller
        for (int c = 0; c < nCh && d.rc == CPQ_OK; ++c)
            d.ok(hipMemcpyAsync(dY + (size_t)c * T * P, dX + (size_t)c * ringSlots * P, (size_t)T * P * sizeof(double2), hipMemcpyDeviceToDevice, nullptr));
        cpq::launch_rfft_inv_ols(nullptr, dY, dOut, (int64_t)T * P, tw, P, nCh, T, dScratch, split);
        d.launched();
    }
    d.get(c2(spectra), dY, nTime);
    d.get(out, dOut, nTime);
    return d.rc;
}

// The FDL multiply-accumulate kernels in isolation (tests/test_gpu_fdl_mac.py): what engine_conv.cpp / engine_native.cpp launch
// for one call -- launch_fdl_mac, then launch_fdl_mac_dcnyq when the variant leaves packed bin 0 to it -- on buffers the caller
// fills in the kernels' own layouts (extents: kernels.hpp, launch_fdl_mac).
int32_t cpq_diag_fdl_mac(int32_t P, int32_t nCh, int32_t K, int32_t T, int32_t tile, int32_t head, int32_t ringSlots,
                         int32_t nIrSlots, int32_t hRows, int32_t hPrivate, const double* x, const double* h,
                         const int32_t* irSlot, double* y, int32_t* variantUsed)
{
    if (!x || !h || !irSlot || !y || !variantUsed) return CPQ_ERR_INVALID_ARG;
    if (!partition(P) || P > 4096 || nCh < 1 || K < 1 || T < 1 || nIrSlots < 1) return CPQ_ERR_INVALID_ARG;
    if (tile != 0 && tile != 4 && tile != 8 && tile != 16 && tile != 32 && tile != cpq::kMacTileCoop && tile != cpq::kMacTileRows128)
        return CPQ_ERR_INVALID_ARG;
    // the engines' own sizing rules (engine_core.cpp: ringSlots; engine_native.cpp layerGeometry: hRows, the smaller of the two)
    const int64_t kPad32 = cpqi::alignUp(K, cpq::kMacMaxTile);
    int64_t ringMin = 1;
    while (ringMin < kPad32 + cpq::kMacMaxTile + T) ringMin <<= 1;
    if (!pow2(ringSlots) || ringSlots < ringMin) return CPQ_ERR_INVALID_ARG;
    if (hRows < kPad32 + 16) return CPQ_ERR_INVALID_ARG;
    if (head < 0 || head >= ringSlots) return CPQ_ERR_INVALID_ARG;
    for (int c = 0; c < nCh; ++c)
        if (irSlot[c] < 0 || irSlot[c] >= nIrSlots) return CPQ_ERR_INVALID_ARG;
    const size_t nX = (size_t)nCh * ringSlots * P, nH = (size_t)nIrSlots * hRows * P, nY = (size_t)nCh * T * P;
    if (nX > kMaxElems || nH > kMaxElems || nY > kMaxElems) return CPQ_ERR_INVALID_ARG;
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;
    *variantUsed = cpq::fdl_mac_variant(tile, T);

    // compact (DC, Nyquist) rows: element 0 of every spectrum, which is what the forward FFT and launch_ir_spectra store there
    std::vector<double2> xdn((size_t)nCh * ringSlots), hdn((size_t)nIrSlots * hRows);
    for (size_t i = 0; i < xdn.size(); ++i) xdn[i] = c2(x)[i * P];
    for (size_t i = 0; i < hdn.size(); ++i) hdn[i] = c2(h)[i * P];

    Scope d;
    const double2* dX = d.put(c2(x), nX);
    const double2* dH = d.put(c2(h), nH);
    const double2* dXdn = d.put(xdn.data(), xdn.size());
    const double2* dHdn = d.put(hdn.data(), hdn.size());
    const int* dSlot = d.put(irSlot, nCh);
    double2* dY = d.put<double2>(nullptr, nY);          // NaN: an element no kernel stores cannot pass for a result
    if (d.rc == CPQ_OK) {
        cpq::launch_fdl_mac(nullptr, tile, dX, dH, dSlot, dY, P, nCh, K, ringSlots, head, T, (int64_t)hRows * P, hPrivate != 0);
        if (cpq::fdl_mac_needs_dcnyq(tile, T))
            cpq::launch_fdl_mac_dcnyq(nullptr, dXdn, dHdn, dSlot, dY, P, nCh, K, ringSlots, head, T, hRows);
        d.launched();
    }
    d.get(c2(y), dY, nY);
    return d.rc;
}

// The forward transform launches in isolation (tests/test_gpu_fft_variants.py): launch_rfft_fwd_ols, or with side != 0
// launch_rfft_fwd_ols_side, as engine_conv.cpp / engine_native.cpp make them -- a moving head, a carried history, a ring that
// wraps.
int32_t cpq_diag_fft_forward(int32_t P, int32_t nCh, int32_t T, int32_t head, int32_t ringSlots, int32_t tailLen, const double* in,
                             const double* histOld, int32_t side, int32_t nSide, const int64_t* sideStride, const int64_t* sideOff,
                             const int64_t* tab, int32_t nTab, int32_t tailStride, double* ring, double* xdn, double* histNew,
                             double* sideOut0, double* sideOut1, int64_t* tabOut, double* tailOut)
{
    if (!in || !histOld || !ring || !xdn || !histNew) return CPQ_ERR_INVALID_ARG;
    if (!partition(P) || nCh < 1 || T < 1 || tailLen < 0) return CPQ_ERR_INVALID_ARG;
    if (!pow2(ringSlots) || ringSlots < T || head < 0 || head >= ringSlots) return CPQ_ERR_INVALID_ARG;
    const size_t rowLen = (size_t)T * P + (size_t)tailLen;
    const size_t inStride = rowLen + (rowLen & 1);          // even: every channel's row starts on 16 bytes (the kernels load double2)
    const size_t nRing = (size_t)nCh * ringSlots * P, nHist = (size_t)nCh * P, nTail = side ? (size_t)nCh * tailStride : 0;
    if (nRing > kMaxElems || (size_t)nCh * inStride > kMaxElems) return CPQ_ERR_INVALID_ARG;
    size_t nSideElems[2] = { 0, 0 };
    double* sideOut[2] = { sideOut0, sideOut1 };
    if (side) {
        // the launcher's own precondition first (P = 512, at most two even-placed destinations, a table of <= 64 entries)
        if (nSide < 0 || nSide > 2 || (nSide > 0 && (!sideStride || !sideOff))) return CPQ_ERR_INVALID_ARG;
        if (!cpq::rfft_fwd_can_carry_side(P, nSide, sideStride, sideOff, nTab)) return CPQ_ERR_INVALID_ARG;
        if (nTab > 0 && (!tab || !tabOut)) return CPQ_ERR_INVALID_ARG;
        if (!tailOut || tailStride < 1 || tailLen > tailStride || nTail > kMaxElems) return CPQ_ERR_INVALID_ARG;
        for (int a = 0; a < nSide; ++a) {          // destination a: [nCh][stride] doubles, the T blocks at off inside every row
            if (!sideOut[a] || sideStride[a] < 1 || sideOff[a] < 0 || sideOff[a] + (int64_t)T * P > sideStride[a]) return CPQ_ERR_INVALID_ARG;
            if ((uint64_t)sideStride[a] > kMaxElems / (size_t)nCh) return CPQ_ERR_INVALID_ARG;
            nSideElems[a] = (size_t)nCh * (size_t)sideStride[a];
        }
    } else if (tailLen != 0) return CPQ_ERR_INVALID_ARG;      // only the side launch moves a tail
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const cpq::FftTables tw = twiddles(d, P);
    double* dIn = d.put<double>(nullptr, (size_t)nCh * inStride);      // (the pad element of an odd row stays NaN)
    for (int c = 0; c < nCh && d.rc == CPQ_OK; ++c)
        d.ok(hipMemcpy(dIn + (size_t)c * inStride, in + (size_t)c * rowLen, rowLen * sizeof(double), hipMemcpyHostToDevice));
    const double* dHistOld = d.put(histOld, nHist);
    double* dHistNew = d.put<double>(nullptr, nHist);
    double2* dX = d.put<double2>(nullptr, nRing);
    double2* dXdn = d.put<double2>(nullptr, (size_t)nCh * ringSlots);
    double2* dScratch = d.put<double2>(nullptr, P > 4096 ? (size_t)nCh * T * P : 0);
    double* dSide[2] = { d.put<double>(nullptr, nSideElems[0]), d.put<double>(nullptr, nSideElems[1]) };
    double* dTail = d.put<double>(nullptr, nTail);
    long long* dTab = d.put<long long>(nullptr, cpq::kGatherTabMax);
    if (d.rc == CPQ_OK) {
        if (side)
            cpq::launch_rfft_fwd_ols_side(nullptr, dIn, (int64_t)inStride, dHistOld, dHistNew, dX, dXdn, tw, nCh, T, head, ringSlots, nSide,
                                          dSide, sideStride, sideOff, nTab > 0 ? dTab : nullptr, ll(tab), nTab, dTail, tailStride, tailLen);
        else
            cpq::launch_rfft_fwd_ols(nullptr, dIn, (int64_t)inStride, dHistOld, dHistNew, dX, dXdn, tw, P, nCh, T, head, ringSlots, dScratch);
        d.launched();
    }
    d.get(c2(ring), dX, nRing);
    d.get(c2(xdn), dXdn, (size_t)nCh * ringSlots);
    d.get(histNew, dHistNew, nHist);
    if (side) {
        for (int a = 0; a < nSide; ++a) d.get(sideOut[a], dSide[a], nSideElems[a]);
        d.get(reinterpret_cast<long long*>(tabOut), dTab, cpq::kGatherTabMax);
        d.get(tailOut, dTail, nTail);
    }
    return d.rc;
}

// The inverse transform's store modes in isolation: launch_rfft_inv_ols_ring (mode 1), launch_rfft_inv_ols_tail (mode 2) and
// launch_rfft_inv_ols_add (mode 3) on spectra, rings, position tables and schedules the caller fills.
int32_t cpq_diag_fft_inverse_store(int32_t mode, int32_t P, int32_t nCh, int32_t T, const double* spectra, double* ringA,
                                   int32_t ringSizeA, const int64_t* posA, int64_t pos0, double* ringB, int32_t ringSizeB,
                                   const int64_t* posB, const double* layerOut, const double* tailRing, int32_t tailRingSize,
                                   const int64_t* tailState, const int64_t* sched, int32_t B, int32_t nTail, double g1, double g2,
                                   double* out)
{
    if (mode < 1 || mode > 3 || !spectra) return CPQ_ERR_INVALID_ARG;
    if (!partition(P) || nCh < 1 || T < 1) return CPQ_ERR_INVALID_ARG;
    const size_t nTime = (size_t)nCh * T * P;
    if (nTime > kMaxElems) return CPQ_ERR_INVALID_ARG;
    int nCb = 0;
    if (mode == 1) {
        // a ring of at least one block and of two elements, so that i and i + 1 are distinct; blocks that are written lie at
        // least P apart on the ring (two workgroups never store to one element: every engine's positions advance by P)
        if (!ringA || !pow2(ringSizeA) || ringSizeA < P || ringSizeA < 2 || (size_t)nCh * ringSizeA > kMaxElems) return CPQ_ERR_INVALID_ARG;
        if (!posA && (pos0 < 0 || pos0 > kMaxPos)) return CPQ_ERR_INVALID_ARG;
        for (int t = 0; t < T; ++t) {
            const long long pt = posA ? posA[t] : pos0 + (long long)t * P;
            if (pt > kMaxPos) return CPQ_ERR_INVALID_ARG;
            if (pt < 0) continue;
            for (int u = 0; u < t; ++u) {
                const long long pu = posA ? posA[u] : pos0 + (long long)u * P;
                if (pu < 0) continue;
                const long long gap = (pt - pu) & (ringSizeA - 1);
                if (gap < P || ringSizeA - gap < P) return CPQ_ERR_INVALID_ARG;
            }
        }
    } else if (mode == 2) {
        if (P > 4096 || !out || !layerOut || !tailRing || !tailState || !sched) return CPQ_ERR_INVALID_ARG;
        if (nTail < 1 || nTail > 2 || !pow2(B) || ((int64_t)T * P) % B != 0) return CPQ_ERR_INVALID_ARG;
        if (!pow2(tailRingSize) || tailRingSize < 2 || (size_t)nTail * nCh * tailRingSize > kMaxElems) return CPQ_ERR_INVALID_ARG;
        if ((size_t)nTail * nTime > kMaxElems) return CPQ_ERR_INVALID_ARG;
        const long long g0 = tailState[3], nSamples = (long long)T * P;
        if (g0 < 0 || g0 > kMaxPos) return CPQ_ERR_INVALID_ARG;
        nCb = (int)(nSamples / B);
        // an entry's B samples end inside the call (samples at or behind g0 come from layerOut[.. nSamples); older ones from the ring)
        for (long long i = 0; i < (long long)nTail * nCb; ++i)
            if (sched[i] >= 0 && sched[i] + B > g0 + nSamples) return CPQ_ERR_INVALID_ARG;
    } else {
        if (P != cpq::kP || !out || !ringA || !posA) return CPQ_ERR_INVALID_ARG;
        if (!pow2(ringSizeA) || ringSizeA < P || ringSizeA < 2 || (size_t)nCh * ringSizeA > kMaxElems) return CPQ_ERR_INVALID_ARG;
        if (ringB && (!posB || !pow2(ringSizeB) || ringSizeB < P || ringSizeB < 2 || (size_t)nCh * ringSizeB > kMaxElems)) return CPQ_ERR_INVALID_ARG;
        for (int t = 0; t < T; ++t)
            if (posA[t] > kMaxPos || (ringB && posB[t] > kMaxPos)) return CPQ_ERR_INVALID_ARG;
    }
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const cpq::FftTables tw = twiddles(d, P);
    const int64_t stride = (int64_t)T * P;
    const size_t nRingA = (size_t)nCh * ringSizeA, nRingB = (size_t)nCh * ringSizeB;
    const double2* dY = d.put(c2(spectra), nTime);
    double2* dScratch = d.put<double2>(nullptr, P > 4096 ? nTime : 0);
    double* dOut = mode != 1 ? d.put<double>(nullptr, nTime) : nullptr;
    double* dRingA = mode != 2 ? d.put(ringA, nRingA) : nullptr;          // initial contents: the caller's
    if (mode == 1) {
        const long long* dPosA = posA ? d.put(ll(posA), T) : nullptr;
        if (d.rc == CPQ_OK) { cpq::launch_rfft_inv_ols_ring(nullptr, dY, dRingA, ringSizeA, dPosA, pos0, tw, P, nCh, T, dScratch); d.launched(); }
    } else if (mode == 2) {
        const double* dLayer = d.put(layerOut, (size_t)nTail * nTime);
        const double* dTailRing = d.put(tailRing, (size_t)nTail * nCh * tailRingSize);
        const long long* dSched = d.put(ll(sched), (size_t)nTail * nCb);
        const long long* dState = d.put(ll(tailState), 4);
        if (d.rc == CPQ_OK) {
            cpq::launch_rfft_inv_ols_tail(nullptr, dY, dOut, stride, tw, P, nCh, T, dScratch, dLayer, dTailRing, tailRingSize, dState, dSched,
                                          nCb, B, nTail, g1, g2);
            d.launched();
        }
    } else {
        const long long* dPosA = d.put(ll(posA), T);
        double* dRingB = ringB ? d.put(ringB, nRingB) : nullptr;
        const long long* dPosB = ringB ? d.put(ll(posB), T) : nullptr;
        if (d.rc == CPQ_OK) {
            const cpq::RingTap b = ringB ? cpq::RingTap{ dRingB, ringSizeB, dPosB, g2 } : cpq::RingTap{};
            cpq::launch_rfft_inv_ols_add(nullptr, dY, dOut, stride, tw, nCh, T, cpq::RingTap{ dRingA, ringSizeA, dPosA, g1 }, b);
            d.launched();
        }
        d.get(ringB, dRingB, nRingB);
    }
    if (mode != 1) d.get(out, dOut, nTime);
    if (mode != 2) d.get(ringA, dRingA, nRingA);
    return d.rc;
}

// launch_ir_spectra and, with a gain, launch_spectrum_gain behind it, on one h_eff.  The device copy of h_eff holds
// nParts * P elements, NaN from heffLen on: a load past the end cannot pass for a zero.
int32_t cpq_diag_ir_spectra(int32_t P, int32_t nParts, const double* heff, int32_t heffLen, const double* gain, double* H, double* HDN,
                            double* Hg, double* HDNg)
{
    if (!heff || !H || !HDN || (gain && (!Hg || !HDNg))) return CPQ_ERR_INVALID_ARG;
    if (!partition(P) || nParts < 1) return CPQ_ERR_INVALID_ARG;
    const size_t n = (size_t)nParts * P;
    if (n > kMaxElems || heffLen < 1 || (size_t)heffLen > n) return CPQ_ERR_INVALID_ARG;
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const cpq::FftTables tw = twiddles(d, P);
    double* dHeff = d.put<double>(nullptr, n);
    if (d.rc == CPQ_OK) d.ok(hipMemcpy(dHeff, heff, (size_t)heffLen * sizeof(double), hipMemcpyHostToDevice));
    const double* dGain = gain ? d.put(gain, (size_t)P + 1) : nullptr;
    double2* dH = d.put<double2>(nullptr, n);
    double2* dHdn = d.put<double2>(nullptr, nParts);
    double2* dScratch = d.put<double2>(nullptr, P > 4096 ? n : 0);
    if (d.rc == CPQ_OK) { cpq::launch_ir_spectra(nullptr, dHeff, heffLen, dH, dHdn, tw, P, nParts, dScratch); d.launched(); }
    d.get(c2(H), dH, n);
    d.get(c2(HDN), dHdn, nParts);
    if (gain && d.rc == CPQ_OK) {          // only now: the ungained spectra are with the caller
        cpq::launch_spectrum_gain(nullptr, dH, dHdn, dGain, P, nParts);
        d.launched();
        d.get(c2(Hg), dH, n);
        d.get(c2(HDNg), dHdn, nParts);
    }
    return d.rc;
}

// ---------------------------------------------------------------- the launchers of mix_kernels.hip (tests/test_gpu_mix_kernels.py)
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
            const cpq::RingTap a = useA ? cpq::RingTap{ dRingA, sizeA, dSchedA, gainA } : cpq::RingTap{};
            const cpq::RingTap b = useB ? cpq::RingTap{ dRingB, sizeB, dSchedB, gainB } : cpq::RingTap{};
            cpq::launch_ring_chunks(nullptr, dOut, outStride, dMap, n, q, dRing0, size0, dPos, dCnt, a, b, nCh);
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

// ---------------------------------------------------------------- the scorer's kernels (tests/test_gpu_score_kernels.py)
// launch_score_spectrum as engine_score.cpp makes it, with the tables of `rate` (the scorer's own upload), on caller-filled rows,
// thresholds and evaluation table
int32_t cpq_diag_score_spectrum(double rate, int32_t nRows, const double* rows, int32_t nThr, double* thr, int32_t nEvals,
                                const cpq_diag_score_eval* evals, int32_t nSlots, int32_t thresholdsOnly, cpq_score_parts* parts,
                                double* blended)
{
    if (!rows || !thr || !evals || !parts || !blended) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_spectrum: null buffer");
    if (!(rate > 0.0) || !std::isfinite(rate)) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_spectrum: sample rate must be finite and > 0");
    if (nRows < 1 || nThr < 1 || nEvals < 1 || nSlots < 1) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_spectrum: n_rows, n_thr, n_evals and n_slots must be >= 1");
    if (!fits(nRows, 2 * cpq::kScoreLen) || !fits(nThr, cpq::kScoreBins) || !fits(nEvals, 1) || !fits(nSlots, 1))
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_spectrum: a buffer above 2^28 elements");
    std::vector<char> slotSeen(nSlots, 0), thrSeen(nThr, 0);
    std::vector<cpq::ScoreEval> table(nEvals);
    for (int i = 0; i < nEvals; ++i) {
        const cpq_diag_score_eval& ev = evals[i];
        if (ev.row < 0 || ev.row >= nRows) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_spectrum: eval %d names row %d outside 0..%d", i, ev.row, nRows - 1);
        if (ev.thr < 0 || ev.thr >= nThr) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_spectrum: eval %d names thr %d outside 0..%d", i, ev.thr, nThr - 1);
        if (ev.slot < 0 || ev.slot >= nSlots) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_spectrum: eval %d names slot %d outside 0..%d", i, ev.slot, nSlots - 1);
        if (slotSeen[ev.slot]) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_spectrum: slot %d named twice", ev.slot);
        if (thresholdsOnly && thrSeen[ev.thr]) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_spectrum: thr %d written twice", ev.thr);
        slotSeen[ev.slot] = thrSeen[ev.thr] = 1;
        table[i] = cpq::ScoreEval{ ev.row, ev.thr, ev.slot, ev.alpha };
    }
    cpq::ScoreTables t;
    if (!cpq::scoreTables(rate, t)) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_spectrum: no Bark band layout at %g Hz", rate);
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    cpqi::ScoreTableBuffers tables;
    std::string error;
    const int rc = cpqi::uploadScoreTables(t, tables, error);
    if (rc != CPQ_OK) return fail(nullptr, CPQ_ERR_DEVICE, "score_spectrum: %s", error.c_str());
    const double* dRows = d.put(rows, (size_t)nRows * 2 * cpq::kScoreLen);
    double* dThr = d.put(thr, (size_t)nThr * cpq::kScoreBins);
    const cpq::ScoreEval* dEvals = d.put(table.data(), table.size());
    cpq_score_parts* dParts = d.put<cpq_score_parts>(nullptr, nSlots);
    double* dBlended = d.put<double>(nullptr, nSlots);
    if (d.rc == CPQ_OK) {
        cpq::launch_score_spectrum(nullptr, dRows, dThr, dEvals, nEvals, tables.dev, dParts, dBlended, thresholdsOnly != 0);
        d.launched();
    }
    d.get(thr, dThr, (size_t)nThr * cpq::kScoreBins);
    d.get(parts, dParts, (size_t)nSlots);
    d.get(blended, dBlended, (size_t)nSlots);
    return d.rc;
}

// launch_score_lattice with the shaper parameters cpq_scorer_create derives from `bits`, on caller-filled rows and chain table
int32_t cpq_diag_score_lattice(int32_t bits, int32_t nSrc, const double* seg, int32_t nDst, double* err, int32_t nChains,
                               const cpq_diag_score_chain* chains, int32_t nCoef, const double* coef, int32_t nRng, const uint64_t* rng)
{
    if (!seg || !err || !chains || !coef || !rng) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_lattice: null buffer");
    if (bits < 1 || bits > 32) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_lattice: bit depth %d outside 1..32", bits);
    if (nSrc < 1 || nDst < 1 || nChains < 1 || nCoef < 1 || nRng < 1) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_lattice: n_src, n_dst, n_chains, n_coef and n_rng must be >= 1");
    if (!fits(nSrc, cpq::kScoreLen) || !fits(nDst, cpq::kScoreLen) || !fits(nChains, 4) || !fits(nCoef, cpq::kLatticeOrder) || !fits(nRng, 4))
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_lattice: a buffer above 2^28 elements");
    std::vector<char> dstSeen(nDst, 0);
    std::vector<cpq::ScoreChain> table(nChains);
    for (int i = 0; i < nChains; ++i) {
        const cpq_diag_score_chain& c = chains[i];
        if (c.src < 0 || c.src >= nSrc) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_lattice: chain %d names src %d outside 0..%d", i, c.src, nSrc - 1);
        if (c.dst < 0 || c.dst >= nDst) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_lattice: chain %d names dst %d outside 0..%d", i, c.dst, nDst - 1);
        if (c.coef < 0 || c.coef >= nCoef) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_lattice: chain %d names coef %d outside 0..%d", i, c.coef, nCoef - 1);
        if (c.rng < 0 || c.rng >= nRng) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_lattice: chain %d names rng %d outside 0..%d", i, c.rng, nRng - 1);
        if (dstSeen[c.dst]) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_lattice: dst %d named twice", c.dst);
        dstSeen[c.dst] = 1;
        table[i] = cpq::ScoreChain{ c.src, c.dst, c.coef, c.rng };
    }
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "generator words travel as unsigned long long");
    const double* dSeg = d.put(seg, (size_t)nSrc * cpq::kScoreLen);
    double* dErr = d.put<double>(nullptr, (size_t)nDst * cpq::kScoreLen);
    const cpq::ScoreChain* dChains = d.put(table.data(), table.size());
    const double* dCoef = d.put(coef, (size_t)nCoef * cpq::kLatticeOrder);
    const unsigned long long* dRng = d.put(reinterpret_cast<const unsigned long long*>(rng), (size_t)nRng * 4);
    if (d.rc == CPQ_OK) {
        cpq::launch_score_lattice(nullptr, dSeg, dErr, dChains, nChains, dCoef, dRng, cpqi::scoreDitherParams(bits));
        d.launched();
    }
    d.get(err, dErr, (size_t)nDst * cpq::kScoreLen);
    return d.rc;
}

// launch_score_reduce on caller-filled counts, states and blended rows
int32_t cpq_diag_score_reduce(int32_t nLearners, int32_t nCand, const int32_t* counts, const int32_t* state, const double* blended,
                              const double* weights, double* scores)
{
    if (!counts || !state || !blended || !weights || !scores) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_reduce: null buffer");
    if (nLearners < 1 || nCand < 1 || (int64_t)nLearners * nCand > (1 << 20))
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_reduce: n_learners and n_cand must be >= 1, their product <= 2^20");
    for (int l = 0; l < nLearners; ++l) {
        int sum = 0;
        for (int i = 0; i < cpq::kScoreLevels; ++i) {
            const int c = counts[l * cpq::kScoreLevels + i];
            if (c < 0 || c > cpq::kScoreMaxSegments) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_reduce: learner %d, level %d: count %d outside 0..%d", l, i, c, cpq::kScoreMaxSegments);
            sum += c;
        }
        if (sum > cpq::kScoreMaxSegments) return fail(nullptr, CPQ_ERR_INVALID_ARG, "score_reduce: learner %d: counts sum to %d, above %d", l, sum, cpq::kScoreMaxSegments);
    }
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const size_t nPairs = (size_t)nLearners * nCand;
    const double* dBlended = d.put(blended, nPairs * cpq::kScoreMaxSegments);
    const int* dCounts = d.put(counts, (size_t)nLearners * cpq::kScoreLevels);
    const int* dState = d.put(state, nPairs);
    double* dScores = d.put<double>(nullptr, nPairs);
    if (d.rc == CPQ_OK) {
        cpq::launch_score_reduce(nullptr, dBlended, dCounts, dState, nLearners, nCand, weights, dScores);
        d.launched();
    }
    d.get(scores, dScores, nPairs);
    return d.rc;
}

int32_t cpq_diag_learn_tell(int32_t nLearners, cpq_learn_state* states, const cpq_learn_params* params, const double* candidates,
                            const double* mapped, const double* fitness)
{
    if (!states || !params || !candidates || !mapped || !fitness) return fail(nullptr, CPQ_ERR_INVALID_ARG, "learn_tell: null buffer");
    if (nLearners < 1 || nLearners > (1 << 20)) return fail(nullptr, CPQ_ERR_INVALID_ARG, "learn_tell: n_learners outside 1..2^20");
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    Scope d;
    const size_t L = (size_t)nLearners;
    const std::vector<int> ones(L, 1);
    cpq_learn_state* dStates = d.put(states, L);
    const int* dActive = d.put(ones.data(), L);
    const double* dCand = d.put(candidates, L * cpq::kLearnVars);
    const double* dMapped = d.put(mapped, L * cpq::kLearnVars);
    const double* dFitness = d.put(fitness, L * cpq::kLearnPop);
    int* dOrder = d.put<int>(nullptr, L * cpq::kLearnPop);
    double* dHistory = d.put<double>(nullptr, L);
    if (d.rc == CPQ_OK) {
        cpq::launch_learn_tell(nullptr, dStates, dActive, nLearners, *params, dCand, dMapped, dFitness, dOrder, dHistory, 1, 0);
        d.launched();
    }
    d.get(states, dStates, L);
    return d.rc;
}

// k_prog_finish alone on caller-filled hop sums: the ProgFinish engine_prog.cpp builds, with n_hops and max_hops the caller's
int32_t cpq_diag_prog_finish(int32_t nStreams, int32_t nHops, int32_t maxHops, double sampleRate, const double* hops,
                             cpq_loudness_result* out, double* z, int32_t* counts)
{
    if (!hops || !out) return fail(nullptr, CPQ_ERR_INVALID_ARG, "prog_finish: null buffer");
    if (nStreams < 1 || nStreams > 32767) return fail(nullptr, CPQ_ERR_INVALID_ARG, "prog_finish: n_streams %d outside 1..32767", nStreams);
    if (maxHops < 1 || nHops < 0 || nHops > maxHops)
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "prog_finish: max_hops %d must be >= 1 and n_hops %d in 0..max_hops", maxHops, nHops);
    cpq::ProgFinish f;
    f.H = cpq::progHop(sampleRate);
    if (!f.H) return fail(nullptr, CPQ_ERR_INVALID_ARG, "prog_finish: sample_rate %g is not a whole number of Hz in 8000..768000 that is divisible by 10", sampleRate);
    if (cpq::progShortCount(nHops) > cpq::kProgSortMax)
        return fail(nullptr, CPQ_ERR_INVALID_ARG, "prog_finish: n_hops %d holds more than %d short-term blocks at the 1 s step", nHops, cpq::kProgSortMax);
    if (!fits(nStreams, maxHops)) return fail(nullptr, CPQ_ERR_INVALID_ARG, "prog_finish: n_streams * max_hops above 2^28");
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;
    f.nHops = nHops; f.maxHops = maxHops; f.zAbs = cpq::progAbsGate();

    Scope d;
    const size_t S = (size_t)nStreams;
    const double* dHops = d.put(hops, S * (size_t)maxHops);
    cpq::ProgRecord* dRec = d.put<cpq::ProgRecord>(nullptr, S);
    if (d.rc == CPQ_OK) {
        cpq::launch_prog_finish(nullptr, dHops, f, nStreams, dRec);
        d.launched();
    }
    std::vector<cpq::ProgRecord> rec(S);
    d.get(rec.data(), dRec, S);
    if (d.rc != CPQ_OK) return d.rc;
    for (size_t s = 0; s < S; ++s) {
        const cpq::ProgRecord& r = rec[s];
        out[s] = cpq::progResult(r, nHops);
        if (z) { const double v[6] = { r.zInt, r.zGate, r.zMomMax, r.zShortMax, r.zLo, r.zHi }; std::copy_n(v, 6, z + 6 * s); }
        if (counts) { const int32_t v[4] = { r.nAbs, r.nRel, r.nShortAbs, r.nShortKept }; std::copy_n(v, 4, counts + 4 * s); }
    }
    return CPQ_OK;
}

// ---------------------------------------------------------------- the complex transforms of minphase_kernels.hip (tests/test_gpu_ir_minphase.py)
// `rows` transforms of 2^log2n points, natural order in and out, on the path minphase_plan.hpp gives the size: up to the LDS bound
// the row pass alone (kRowsFwd; kRowsInv with the 1 / N scale), above it columns then rows (forward) or rows then columns
// (inverse).  The four-step forward leaves X[k1 + N1 k2] at [k1][k2] and the inverse reads that layout; the reordering between it
// and natural order is done here, on the host.
int32_t cpq_diag_cfft(const double* re_im, int32_t log2n, int32_t rows, int32_t inverse, double* out)
{
    if (!re_im || !out || log2n < 1 || log2n > 23 || rows < 1 || !fits(rows, 2LL << log2n)) return CPQ_ERR_INVALID_ARG;
    if (!haveDevice()) return CPQ_ERR_NO_DEVICE;

    int lg1 = 0, lg2 = 0;
    cpq::minphaseFactor(log2n, lg1, lg2);
    const size_t N = (size_t)1 << log2n, N1 = (size_t)1 << lg1, N2 = (size_t)1 << lg2, total = (size_t)rows * N;
    std::vector<double> hi, lo, host;
    const std::vector<double> roots = cpq::minphaseStageRoots();
    cpq::minphaseSplitRoots(log2n, hi, lo);
    const double* src = re_im;
    if (lg1 > 0 && inverse) {       // natural order -> [k1][k2]
        host.resize(2 * total);
        for (size_t r = 0; r < (size_t)rows; ++r)
            for (size_t k = 0; k < N; ++k) {
                const size_t at = r * N + (k & (N1 - 1)) * N2 + (k >> lg1);
                host[2 * at] = re_im[2 * (r * N + k)];
                host[2 * at + 1] = re_im[2 * (r * N + k) + 1];
            }
        src = host.data();
    }

    Scope d;
    const cpq::MinphaseTables t{ c2(d.put(roots.data(), roots.size())), c2(d.put(hi.data(), hi.size())), c2(d.put(lo.data(), lo.size())) };
    double2* z = c2(d.put(src, 2 * total));
    if (d.rc == CPQ_OK) {
        if (lg1 == 0) cpq::launch_cfft_rows(nullptr, inverse ? cpq::kRowsInv : cpq::kRowsFwd, z, nullptr, t, 0, lg2, rows, 1.0 / (double)N);
        else if (inverse) {
            cpq::launch_cfft_rows(nullptr, cpq::kRowsInv, z, nullptr, t, lg1, lg2, rows, 1.0);
            cpq::launch_cfft_cols(nullptr, cpq::kColsInvComplex, z, nullptr, nullptr, nullptr, nullptr, t, lg1, lg2, rows);
        } else {
            cpq::launch_cfft_cols(nullptr, cpq::kColsFwdComplex, z, nullptr, nullptr, nullptr, nullptr, t, lg1, lg2, rows);
            cpq::launch_cfft_rows(nullptr, cpq::kRowsFwd, z, nullptr, t, lg1, lg2, rows, 1.0);
        }
        d.launched();
    }
    if (lg1 > 0 && !inverse) {      // [k1][k2] -> natural order
        host.resize(2 * total);
        d.get(host.data(), reinterpret_cast<const double*>(z), 2 * total);
        if (d.rc == CPQ_OK)
            for (size_t r = 0; r < (size_t)rows; ++r)
                for (size_t k = 0; k < N; ++k) {
                    const size_t at = r * N + (k & (N1 - 1)) * N2 + (k >> lg1);
                    out[2 * (r * N + k)] = host[2 * at];
                    out[2 * (r * N + k) + 1] = host[2 * at + 1];
                }
    } else d.get(out, reinterpret_cast<const double*>(z), 2 * total);
    return d.rc;
}

// needs the engine: the header of its chained-span launches
int32_t cpq_diag_eq_chain_status(cpq_engine* e, uint32_t* launches, uint32_t* gaveUp)
{
    if (!e || !launches || !gaveUp) return CPQ_ERR_INVALID_ARG;
    *launches = 0;
    *gaveUp = 0;
    if (!e->svfChain || e->svfChainSpans <= 0) return CPQ_OK;
    (void)hipSetDevice(e->device);
    uint32_t hdr[4] = { 0, 0, 0, 0 };          // generation, finished workgroups, ticket, error (svf_kernels.hip: TpvChainHeader)
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    CPQ_HIP(e, hipMemcpy(hdr, e->svfChain, sizeof(hdr), hipMemcpyDeviceToHost));
    *launches = hdr[0];
    *gaveUp = hdr[3];
    return CPQ_OK;
}

}  // extern "C"
