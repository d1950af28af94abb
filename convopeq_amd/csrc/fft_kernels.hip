// fft_kernels.hip -- fp64 real FFT kernels for gfx950 (CDNA4, wave64): the partition transforms of the convolver.
//
// A P-sample partition is transformed as the 2P-point real FFT of an overlap-save frame, computed as a P-point complex
// FFT of z[n] = x[2n] + i x[2n+1] followed by the real-FFT split.  The overlap-save framing of the reference (copy
// [prev|cur], src/MKLNonUniformConvolver.cpp:1256-1258), its CCS de-interleave (:132-139, :1270-1283) and the output half
// selection (:1332) are fused into the loads/stores, so a frame is read once from HBM and a spectrum written once.
//
// Replaces ippsFFTFwd_RToCCS_64f / ippsFFTInv_CCSToR_64f (src/FFTBackend.cpp:123-150) with the same
// scaling convention (IPP_FFT_DIV_INV_BY_N: forward unscaled, inverse 1/N, :33-35).
//
// Spectrum layout ("packed"): P complex per transform; bin k (1..P-1) = X[k]; bin 0 = (X[0], X[P]) (DC and Nyquist are
// both real).  Up to P = 2048 element k is bin k; from P = 4096 up the spectrum is stored PERMUTED, element
// k1 * 512 + k2 = bin k1 + (P / 512) k2 (the MAC is element-wise; forward, IR and inverse transforms agree on it).
//
// Five families, chosen from P by fftFamily() for all three launchers (forward, IR spectra, inverse):
//
//   P              family       kernels                                             complex FFT
//   64, 128, 256   Stockham     k_rfft_fwd_lds<StockhamFft, FRAME>,                 radix-2 Stockham, two LDS buffers
//                               k_rfft_inv_lds<MODE, StockhamFft>
//   512            Wave512      k_rfft_fwd_ols<SIDE>, k_ir_spectra,                 wave_cfft512: one wave, 8 points per lane
//                               k_rfft_inv_ols<MODE>
//   1024, 2048     MixedRadix   k_rfft_fwd_lds<MixedRadixFft, FRAME>,               wg_cfft: radix 8 (+ 4 or 2), one padded
//                               k_rfft_inv_lds<MODE, MixedRadixFft>                 LDS buffer
//   4096           P4           k_rfft_fwd_ols_p4, k_ir_spectra_p4,                 four-step inside a workgroup: dft8, then
//                               k_rfft_inv_ols_p4<MODE>                             wave_cfft512 per wave
//   8192 ... 2^17  FourStep     k_big_cols_fwd<FRAME>, k_big_rows_fwd,              four-step through scratch: col_fft, then
//                               k_big_rows_inv, k_big_cols_inv<MODE>                wave_cfft512 per row (FourStepGeom)
//
// (FRAME = true: overlap-save frames; false: zero-padded IR partitions.  MODE: where store_block2 puts a block.)
//
// Written once and shared by every family, so that they stay bit-identical to one another (the engine mixes families
// inside one plan group; tests/test_gpu_fft_variants.py and tests/test_gpu_fft_p4_frames.py compare the launch paths bit
// for bit, tests/test_gpu_fft_bits.py every size with a recorded digest):
//   rfft_split / pack_dcnyq       Z[k], Z[M-k], w -> X[k]; the packed element 0
//   rfft_unsplit / unpack_dcnyq   the inverse of the two
//                                 (Stockham, MixedRadix, FourStep call them; Wave512 and P4 carry the same expressions as
//                                 inline text, marked at the four sites: through the helpers the compiler orders those
//                                 unrolled loops differently, and the P4 kernels sit at their register limit -- RESULTS.md)
//   OlsFrame::load, ir_part_load  complex element n of a frame (with the history store) / of an IR partition
//                                 (Stockham, MixedRadix, FourStep; Wave512 and P4 load whole register halves instead)
//   stage8 / stage_small          one Stockham radix-8 / radix-2,4 stage over an LDS index map (wg_cfft: WgMap, col_fft: ColMap)
//   dft8, mul_powers, wave_cfft512, store_block2
// Each site keeps its own way of finding the partner element and the twiddle.
#include "kernels.hpp"

namespace cpq {

namespace {

typedef double v2d __attribute__((ext_vector_type(2)));      // 16-byte streaming (non-temporal) loads / stores

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// a * w (INV = false) or a * conj(w) (INV = true)
__device__ __forceinline__ double2 cmul(double2 a, double2 b)
{
    return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x));
}

// exp(-2 pi i q / 16), q < 8 (correctly rounded constants)
__device__ __forceinline__ double2 w16(int q)
{
    constexpr double c1 = 0.92387953251128673848, s1 = 0.38268343236508978178, r = 0.70710678118654752440;
    switch (q) {
        case 0: return make_double2(1.0, 0.0);
        case 1: return make_double2(c1, -s1);
        case 2: return make_double2(r, -r);
        case 3: return make_double2(s1, -c1);
        case 4: return make_double2(0.0, -1.0);
        case 5: return make_double2(-s1, -c1);
        case 6: return make_double2(-r, -r);
        default: return make_double2(-c1, -s1);
    }
}

template <bool INV>
__device__ __forceinline__ double2 cmulw(double2 a, double2 w)
{
    if (INV) return make_double2(fma(a.x, w.x, a.y * w.y), fma(a.y, w.x, -(a.x * w.y)));
    return make_double2(fma(a.x, w.x, -(a.y * w.y)), fma(a.x, w.y, a.y * w.x));
}

// real-FFT split: Z = M-point FFT of (even + i odd) samples -> bin k of the 2M-point real frame,
// X[k] = E + w O with E = (Z[k] + conj Z[M-k]) / 2, O = -i (Z[k] - conj Z[M-k]) / 2, w = exp(-2 pi i k / 2M); zm = Z[M-k]
// (twiddle() gives w: a callable, so that w is fetched where the sites fetched it, between the sums and the product)
template <typename W>
__device__ __forceinline__ double2 rfft_split(double2 zk, double2 zm, W twiddle)
{
    const double2 e = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));   // (Z[k] + conj Z[M-k]) / 2
    const double2 d = make_double2(0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y));   // (Z[k] - conj Z[M-k]) / 2
    const double2 o = make_double2(d.y, -d.x);                                  // -i d
    const double2 w = twiddle();
    return make_double2(e.x + fma(o.x, w.x, -(o.y * w.y)), e.y + fma(o.x, w.y, o.y * w.x));
}
// element 0 of a packed spectrum from Z[0]: (DC, Nyquist), both real
__device__ __forceinline__ double2 pack_dcnyq(double2 z0) { return make_double2(z0.x + z0.y, z0.x - z0.y); }

// inverse of the split: packed spectrum Y -> z[k] = E + i O, the input of the M-point inverse FFT; ym = Y[M-k], same w
template <typename W>
__device__ __forceinline__ double2 rfft_unsplit(double2 yk, double2 ym, W twiddle)
{
    const double2 e = make_double2(0.5 * (yk.x + ym.x), 0.5 * (yk.y - ym.y));
    const double2 d = make_double2(0.5 * (yk.x - ym.x), 0.5 * (yk.y + ym.y));
    const double2 w = twiddle();
    const double2 o = make_double2(fma(d.x, w.x, d.y * w.y), fma(d.y, w.x, -(d.x * w.y)));   // d * conj(w)
    return make_double2(e.x - o.y, e.y + o.x);                                               // E + i O
}
// z[0] from the packed element 0 = (DC, Nyquist)
__device__ __forceinline__ double2 unpack_dcnyq(double2 y0) { return make_double2(0.5 * (y0.x + y0.y), 0.5 * (y0.x - y0.y)); }

// The overlap-save frame [previous block | block t] of channel c as P complex points (copy [prev|cur],
// src/MKLNonUniformConvolver.cpp:1256-1258); the previous block of t = 0 is the history of the call before
struct OlsFrame {
    const double* cur; const double* prev; double* hist; int halfP; bool last;
    __device__ __forceinline__ OlsFrame(const double* in, int64_t chStride, const double* histOld, double* histNew, int P, int T,
                                        int c, int t)
        : cur(in + (int64_t)c * chStride + (int64_t)t * P), prev((t > 0) ? (cur - P) : (histOld + (int64_t)c * P)),
          hist(histNew + (int64_t)c * P), halfP(P >> 1), last(t == T - 1)
    {
    }
    // element n into dst (a register or LDS: written first, the kernels' loops were timed in that order); the call's last block
    // also goes to the overlap history of the next call (prevInputBuf, NUC.cpp:1258)
    __device__ __forceinline__ void load(int n, double2& dst) const
    {
        const double* src = (n < halfP) ? (prev + 2 * n) : (cur + 2 * (n - halfP));
        const double2 v = *reinterpret_cast<const double2*>(src);
        dst = v;
        if (last && n >= halfP) *reinterpret_cast<double2*>(hist + 2 * (n - halfP)) = v;
    }
};

// complex element n (< P) of the zero-padded IR partition `part` of heff: [h[part P .. (part+1) P) | 0] (NUC.cpp:921-928)
__device__ __forceinline__ double2 ir_part_load(const double* __restrict__ heff, int heffLen, int part, int P, int n)
{
    double2 v = make_double2(0.0, 0.0);
    if (n < (P >> 1)) {
        const int64_t i = (int64_t)part * P + 2 * n;
        v = make_double2(i < heffLen ? heff[i] : 0.0, (i + 1) < heffLen ? heff[i + 1] : 0.0);
    }
    return v;
}

// 4-point DFT of (t0..t3) -> (t0..t3), natural order
template <bool INV>
__device__ __forceinline__ void dft4(double2& t0, double2& t1, double2& t2, double2& t3)
{
    const double2 e0 = cadd(t0, t2), e1 = csub(t0, t2);
    const double2 o0 = cadd(t1, t3), d = csub(t1, t3);
    const double2 o1 = INV ? make_double2(-d.y, d.x) : make_double2(d.y, -d.x);   // * (+i) / * (-i)
    t0 = cadd(e0, o0);
    t1 = cadd(e1, o1);
    t2 = csub(e0, o0);
    t3 = csub(e1, o1);
}

// 8-point DFT in registers: v[p] <- sum_a W8^(a p) v[a], natural order in and out
template <bool INV>
__device__ __forceinline__ void dft8(double2 (&v)[8])
{
    constexpr double h = 0.70710678118654752440;
    double2 s0 = cadd(v[0], v[4]), d0 = csub(v[0], v[4]);
    double2 s1 = cadd(v[1], v[5]), d1 = csub(v[1], v[5]);
    double2 s2 = cadd(v[2], v[6]), d2 = csub(v[2], v[6]);
    double2 s3 = cadd(v[3], v[7]), d3 = csub(v[3], v[7]);
    if (INV) {
        d1 = make_double2(h * (d1.x - d1.y), h * (d1.x + d1.y));
        d2 = make_double2(-d2.y, d2.x);
        d3 = make_double2(-h * (d3.x + d3.y), h * (d3.x - d3.y));
    } else {
        d1 = make_double2(h * (d1.x + d1.y), h * (d1.y - d1.x));
        d2 = make_double2(d2.y, -d2.x);
        d3 = make_double2(h * (d3.y - d3.x), -h * (d3.x + d3.y));
    }
    dft4<INV>(s0, s1, s2, s3);
    dft4<INV>(d0, d1, d2, d3);
    v[0] = s0; v[2] = s1; v[4] = s2; v[6] = s3;
    v[1] = d0; v[3] = d1; v[5] = d2; v[7] = d3;
}

constexpr int kLdsPerWave = 72 * 8;   // complex elements

// 512-point complex FFT of one wave.  In: v[j] = z[lane + 64 j].  Out: v[r] = Z[lane + 64 r].
// n = 64a + 8b + c, k = p + 8q + 64r:
//   pass 1 over a (registers), twiddle W512^((8b+c) p); exchange -> lane (p, c), registers over b
//   pass 2 over b, twiddle W64^(c q);                   exchange -> lane (p + 8q), registers over c
//   pass 3 over c.
// LDS traffic between the lanes of ONE wave: the hardware keeps a wave's DS operations in order; this keeps the compiler
// from moving them across each other
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// v[p] *= w^p (INV: conj(w)^p), p = 1..7, the powers formed by multiplication (depth <= 3 products: a few ulp) rather than
// read from a table: the transforms below are bound by LDS bandwidth (a frame of the P = 4096 kernels moved 106 16-byte
// LDS accesses per lane, 42 of them twiddle-table reads), not by the VALU
template <bool INV>
__device__ __forceinline__ void mul_powers(double2 (&v)[8], double2 w1)
{
    const double2 w2 = cmul(w1, w1), w3 = cmul(w2, w1), w4 = cmul(w2, w2);
    v[1] = cmulw<INV>(v[1], w1);
    v[2] = cmulw<INV>(v[2], w2);
    v[3] = cmulw<INV>(v[3], w3);
    v[4] = cmulw<INV>(v[4], w4);
    v[5] = cmulw<INV>(v[5], cmul(w4, w1));
    v[6] = cmulw<INV>(v[6], cmul(w3, w3));
    v[7] = cmulw<INV>(v[7], cmul(w4, w3));
}

// 512-point complex FFT of one wave: v[p] = z[lane + 64 p] in, Z[lane + 64 c] out (three radix-8 passes, two exchanges
// through `lds`).  wa = W512^lane, wb = W64^(lane & 7) (W_N = exp(-2 pi i / N)).
// WAVE: the wave is part of a larger workgroup and `lds` is its private slice: wave-level synchronisation instead of
// workgroup barriers
template <bool INV, bool WAVE = false>
__device__ __forceinline__ void wave_cfft512(double2 (&v)[8], double2* lds, int lane, double2 wa, double2 wb)
{
    auto sync = [] { if (WAVE) wave_sync(); else __syncthreads(); };
    dft8<INV>(v);
    mul_powers<INV>(v, wa);
#pragma unroll
    for (int p = 0; p < 8; ++p) lds[72 * p + lane] = v[p];
    sync();
    const int pp = lane >> 3, cc = lane & 7;
#pragma unroll
    for (int b = 0; b < 8; ++b) v[b] = lds[72 * pp + 8 * b + cc];
    sync();
    dft8<INV>(v);
    mul_powers<INV>(v, wb);
#pragma unroll
    for (int q = 0; q < 8; ++q) lds[66 * cc + pp + 8 * q] = v[q];
    sync();
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = lds[66 * c + lane];
    dft8<INV>(v);
}

// real-FFT split: Z (512-pt FFT of even+i*odd samples) -> packed spectrum of the 1024-pt real frame
__device__ __forceinline__ void wave_split_store(double2 (&v)[8], double2* lds, double2 wl,
                                                 int lane, double2* __restrict__ spec, double2* __restrict__ dcnyq)
{
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) lds[lane + 64 * r] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int k = lane + 64 * r;
        const double2 zk = v[r];
        const double2 zm = lds[(512 - k) & 511];
        // rfft_split / pack_dcnyq, inline: through the helpers the compiler orders this loop's instructions differently (RESULTS.md)
        const double2 e = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));   // (Z[k] + conj Z[512-k]) / 2
        const double2 d = make_double2(0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y));   // (Z[k] - conj Z[512-k]) / 2
        const double2 o = make_double2(d.y, -d.x);                                  // -i d
        const double2 w = cmul(wl, w16(r));                                         // exp(-2 pi i (lane + 64 r) / 1024)
        double2 xk = make_double2(e.x + fma(o.x, w.x, -(o.y * w.y)), e.y + fma(o.x, w.y, o.y * w.x));
        if (k == 0) {
            xk = make_double2(zk.x + zk.y, zk.x - zk.y);   // (DC, Nyquist)
            *dcnyq = xk;
        }
        // streaming store: an FDL row is next read by the MAC of this or a later call, never from cache (the MAC of the
        // same call runs 1 % faster with its L2 left alone)
        __builtin_nontemporal_store(v2d{ xk.x, xk.y }, reinterpret_cast<v2d*>(spec + k));      // one 16-byte store per lane
    }
}

// side: a plan group's call on its first launch -- the block also goes into the input accumulators of the group's other layers
// (Add()'s per-layer accumulation, src/MKLNonUniformConvolver.cpp:1431-1446: what k_rows_gather_multi would do in a launch of
// its own) and the call's chunk tables, riding along as kernel arguments, are stored for the kernels behind this one.
// tail*: the samples behind the last whole block of the source rows (a layer's input accumulator) go to the front of the other
// accumulator buffer -- the remainder move that would be a k_rows_copy launch of its own.
struct FwdSide {
    double* dst[2]; long long stride[2], off[2]; int n;
    long long* tabDst; int nTab; long long tab[kGatherTabMax];
    double* tailDst; long long tailStride; int tailLen;
};
template <bool SIDE>
__global__ __launch_bounds__(64) void k_rfft_fwd_ols(const double* __restrict__ in, int64_t chStride,
                                                     const double* __restrict__ histOld,
                                                     double* __restrict__ histNew, double2* __restrict__ X,
                                                     double2* __restrict__ XDN, FftTables tw, int T, int head,
                                                     int ringMask, FwdSide side)
{
    __shared__ double2 lds[kLdsPerWave];
    const int lane = threadIdx.x;
    const int c = blockIdx.x / T;
    const int t = blockIdx.x - c * T;
    const double* cur = in + (int64_t)c * chStride + (int64_t)t * kP;
    const double* prev = (t > 0) ? (cur - kP) : (histOld + (int64_t)c * kP);
    const double2 wl = tw.tw1024[lane], wa = tw.tw512[lane], wb = tw.tw512[8 * (lane & 7)];

    double2 v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const double2*>(prev + 2 * (lane + 64 * j));
#pragma unroll
    for (int j = 0; j < 4; ++j) v[4 + j] = *reinterpret_cast<const double2*>(cur + 2 * (lane + 64 * j));
    if (t == T - 1) {   // overlap history for the next call (prevInputBuf, NUC.cpp:1258)
        double* hn = histNew + (int64_t)c * kP;
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<double2*>(hn + 2 * (lane + 64 * j)) = v[4 + j];
    }
    if (SIDE) {
        if (blockIdx.x == 0 && lane < side.nTab) side.tabDst[lane] = side.tab[lane];
        if (t == T - 1 && side.tailLen > 0) {
            const double* ts = in + (int64_t)c * chStride + (int64_t)T * kP;
            double* td = side.tailDst + (int64_t)c * side.tailStride;
            for (int i = lane; i < side.tailLen; i += 64) td[i] = ts[i];
        }
        for (int a = 0; a < side.n; ++a) {          // (offsets even: 16-byte stores)
            double* d = side.dst[a] + (int64_t)c * side.stride[a] + side.off[a] + (int64_t)t * kP;
#pragma unroll
            for (int j = 0; j < 4; ++j) *reinterpret_cast<double2*>(d + 2 * (lane + 64 * j)) = v[4 + j];
        }
    }
    wave_cfft512<false>(v, lds, lane, wa, wb);
    const int slot = (head + t) & ringMask;
    const int64_t row = (int64_t)c * (ringMask + 1) + slot;
    wave_split_store(v, lds, wl, lane, X + row * kP, XDN + row);
}

__global__ __launch_bounds__(64) void k_ir_spectra(const double* __restrict__ heff, int heffLen,
                                                   double2* __restrict__ H, double2* __restrict__ HDN, FftTables tw)
{
    __shared__ double2 lds[kLdsPerWave];
    const int lane = threadIdx.x;
    const int k = blockIdx.x;
    const double2 wl = tw.tw1024[lane], wa = tw.tw512[lane], wb = tw.tw512[8 * (lane & 7)];
    double2 v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = k * kP + 2 * (lane + 64 * j);
        v[j] = make_double2(i < heffLen ? heff[i] : 0.0, (i + 1) < heffLen ? heff[i + 1] : 0.0);
    }
#pragma unroll
    for (int j = 4; j < 8; ++j) v[j] = make_double2(0.0, 0.0);   // zero-padded second half (NUC.cpp:921-928)
    wave_cfft512<false>(v, lds, lane, wa, wb);
    wave_split_store(v, lds, wl, lane, H + (int64_t)k * kP, HDN + k);
}

// Where an inverse transform puts block t of channel c (i = even sample index inside the block):
//   MODE 0: the call's output rows;
//   MODE 1: a per-channel ring at the position the block has there -- pos[t], or pos0 + t P when pos is null; a negative
//           position drops the block (ringWrite / delayLineWrite of the plan groups, src/MKLNonUniformConvolver.cpp:1341-1371,
//           :1639-1648, fused into the transform's stores);
//   MODE 2: the output rows PLUS what the replayed delay-line reader of the tail layers adds at those samples (layered
//           mode, mix_kernels.hip: k_tail_schedule has filled sched for the call; the additions come from this call's
//           natural-time tail outputs where the sample lies inside the call, from the layer's ring where it is older) --
//           the read-modify-write pass over the call's output that k_layer_combine would make is gone.
//   MODE 3: the output rows PLUS the delay-line read-add of a plan group's tail layers (Get(), :1620-1633: layer 1 first, then
//           layer 2, `dst += src` or `dst += src * gain`) where every block is one chunk of the call: what k_ring_chunks
//           would do in a pass of its own over the output.
struct OutSpec {
    double* ring; int mask; const long long* pos; long long pos0;                                  // MODE 1; MODE 3: ring A, its mask, its schedule
    const double* ringB; int maskB; const long long* schedB;                                      // MODE 3: ring B (or null)
    const double* layerOut; const double* tailRing; const long long* tailState; const long long* sched;      // MODE 2
    int nCb, B, log2B, tailMask, nTail, nChAll, nSamples; double g1, g2;
};
template <int MODE>
__device__ __forceinline__ void store_block2(double* out, int64_t chStride, const OutSpec& ro, int c, int t, int P, int i, double2 v)
{
    if (MODE == 0) { *reinterpret_cast<double2*>(out + (int64_t)c * chStride + (int64_t)t * P + i) = v; return; }
    if (MODE == 2) {
        const long long g0 = ro.tailState[3];          // TailState::g0: global index of the call's first sample
        auto tail = [&](int n, double y) {
            const int cbk = n >> ro.log2B, j = n & (ro.B - 1);          // (whole-block engines: B is a power of two)
            for (int l = 0; l < ro.nTail; ++l) {
                const long long s = ro.sched[(long long)l * ro.nCb + cbk];
                if (s >= 0) {
                    const double g = l == 0 ? ro.g1 : ro.g2;
                    const long long idx = s + j;
                    const double x = idx >= g0 ? ro.layerOut[((long long)l * ro.nChAll + c) * ro.nSamples + (idx - g0)]
                                               : ro.tailRing[((long long)l * ro.nChAll + c) * (ro.tailMask + 1) + (idx & ro.tailMask)];
                    // delayLineReadAdd: dst += src (gain within 1e-12 of 1) else dst += src * gain (:1673-1676)
                    y = (fabs(g - 1.0) < 1.0e-12) ? (y + x) : (y + x * g);
                }
            }
            return y;
        };
        const int n0 = t * P + i;
        v.x = tail(n0, v.x);
        v.y = tail(n0 + 1, v.y);
        *reinterpret_cast<double2*>(out + (int64_t)c * chStride + (int64_t)t * P + i) = v;
        return;
    }
    if (MODE == 3) {
        const long long sa = ro.pos[t], sb = ro.ringB ? ro.schedB[t] : -1;
        if (sa >= 0) {
            const double* ra = ro.ring + (int64_t)c * (ro.mask + 1);
            const double a0 = ra[(sa + i) & ro.mask], a1 = ra[(sa + i + 1) & ro.mask];
            const bool unity = fabs(ro.g1 - 1.0) < 1.0e-12;
            v.x = unity ? (v.x + a0) : (v.x + a0 * ro.g1);
            v.y = unity ? (v.y + a1) : (v.y + a1 * ro.g1);
        }
        if (sb >= 0) {
            const double* rb = ro.ringB + (int64_t)c * (ro.maskB + 1);
            const double b0 = rb[(sb + i) & ro.maskB], b1 = rb[(sb + i + 1) & ro.maskB];
            const bool unity = fabs(ro.g2 - 1.0) < 1.0e-12;
            v.x = unity ? (v.x + b0) : (v.x + b0 * ro.g2);
            v.y = unity ? (v.y + b1) : (v.y + b1 * ro.g2);
        }
        *reinterpret_cast<double2*>(out + (int64_t)c * chStride + (int64_t)t * P + i) = v;
        return;
    }
    const long long p = ro.pos ? ro.pos[t] : ro.pos0 + (long long)t * P;
    if (p < 0) return;
    double* r = ro.ring + (int64_t)c * (ro.mask + 1);
    const long long a = p + i;
    if ((p & 1) == 0) *reinterpret_cast<double2*>(r + (a & ro.mask)) = v;
    else { r[a & ro.mask] = v.x; r[(a + 1) & ro.mask] = v.y; }
}

template <int MODE>
__global__ __launch_bounds__(64) void k_rfft_inv_ols(const double2* __restrict__ Y, double* __restrict__ out,
                                                     int64_t chStride, FftTables tw, int T, OutSpec ro)
{
    __shared__ double2 lds[kLdsPerWave];
    const int lane = threadIdx.x;
    const int c = blockIdx.x / T;
    const int t = blockIdx.x - c * T;
    const double2* y = Y + (int64_t)blockIdx.x * kP;
    const double2 wl = tw.tw1024[lane], wa = tw.tw512[lane], wb = tw.tw512[8 * (lane & 7)];

    double2 v[8];
    const double2 y0 = y[0];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = lane + 64 * j;
        const double2 yk = y[k];
        const double2 ym = y[(512 - k) & 511];
        // rfft_unsplit / unpack_dcnyq, inline (as in wave_split_store)
        const double2 e = make_double2(0.5 * (yk.x + ym.x), 0.5 * (yk.y - ym.y));
        const double2 d = make_double2(0.5 * (yk.x - ym.x), 0.5 * (yk.y + ym.y));
        const double2 w = cmul(wl, w16(j));                                                     // exp(-2 pi i (lane + 64 j) / 1024)
        const double2 o = make_double2(fma(d.x, w.x, d.y * w.y), fma(d.y, w.x, -(d.x * w.y)));   // d * conj(w)
        double2 z = make_double2(e.x - o.y, e.y + o.x);                                          // E + i O
        if (k == 0) z = make_double2(0.5 * (y0.x + y0.y), 0.5 * (y0.x - y0.y));
        v[j] = z;
    }
    wave_cfft512<true>(v, lds, lane, wa, wb);
    // second half of the 1024-sample frame: z[n], n = lane + 64 r, r = 4..7  (NUC.cpp:1332)
    constexpr double s = 1.0 / 512.0;
#pragma unroll
    for (int r = 4; r < 8; ++r)
        store_block2<MODE>(out, chStride, ro, c, t, kP, 2 * (lane + 64 * (r - 4)), make_double2(v[r].x * s, v[r].y * s));
}


// ---------------------------------------------------------------------------------------------------------
// P = 64 ... 2048 except 512: one workgroup per transform with the whole transform in LDS.  Two complex FFTs, one set
// of kernels (k_rfft_fwd_lds, k_rfft_inv_lds) over a policy type F that supplies
//   F::at(i)              LDS address of logical element i
//   F::cfft<INV>(lds, M, twM)   the M-point FFT of the elements in LDS; returns the buffer that holds the result
//   F::kMaxThreads, F::threads(P), F::ldsBytes(P)     launch geometry
// Slower per byte than the wave-level 512-point kernels above; P <= 256 covers the block-size sweep of BASELINE.json configs[2].
// tw.tw512 holds exp(-2 pi i m / P) (m < P), tw.tw1024 holds exp(-2 pi i k / 2P) (k < P) for the engine's P.

// radix-2 Stockham autosort between two buffers a, b of M complex
template <bool INV>
__device__ __forceinline__ double2* stockham(double2* a, double2* b, int M, const double2* __restrict__ twM)
{
    const int half = M >> 1;
    for (int ns = 1; ns < M; ns <<= 1) {
        const int tstep = half / ns;                 // twiddle index scale: exp(-2 pi i k / (2 ns)) = twM[k * tstep]
        for (int j = threadIdx.x; j < half; j += blockDim.x) {
            const int k = j & (ns - 1);
            const double2 w = twM[k * tstep];
            const double2 u = a[j];
            const double2 v = cmulw<INV>(a[j + half], w);
            const int o = ((j - k) << 1) + k;
            b[o] = cadd(u, v);
            b[o + ns] = csub(u, v);
        }
        __syncthreads();
        double2* t = a; a = b; b = t;
    }
    return a;      // buffer holding the result, natural order
}

// Mixed-radix Stockham stages through ONE LDS buffer: every thread reads its 8 inputs, butterflies in registers, barrier,
// writes its 8 outputs, barrier.  Stage with radix R and Ns = product of earlier radices, butterfly j in [0, M/R):
//   k = j mod Ns,  in[j + q M/R] * exp(-2 pi i q k / (R Ns))  ->  out[(j - k) R + k + q Ns].
// MAP says where the M logical elements live and which butterflies the thread has:
//   m.at(i)     LDS address of element i
//   m.j, m.nj   the thread's first butterfly index and the number of threads along the element axis (M / 8)
//   kTwStep     exp(-2 pi i m / M) = twM[m * kTwStep]
// WgMap: one transform per workgroup (wg_cfft); ColMap: one transform per column of a tile (col_fft, below).
// WgMap pads one element per 8: the first radix-8 stage writes elements 8 j + q from consecutive lanes j (stride 128 B: an
// 8-way bank conflict unpadded, conflict-free at stride 9), the second one 64 a + b
__device__ __forceinline__ int wgp(int i) { return i + (i >> 3); }
struct WgMap {
    static constexpr int kTwStep = 1;
    int j, nj;
    __device__ __forceinline__ int at(int i) const { return wgp(i); }
};

// radix-8 stage; the first stage of a transform (ns = 1) has no twiddles
template <bool INV, typename MAP>
__device__ __forceinline__ void stage8(double2* lds, int M, int ns, const double2* __restrict__ twM, MAP m)
{
    const int j = m.j;
    const int stride = M >> 3;
    const int k = j & (ns - 1);
    double2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = lds[m.at(j + q * stride)];
    const int tstep = (M / (8 * ns)) * MAP::kTwStep;
    if (ns > 1) mul_powers<INV>(v, twM[k * tstep]);      // one root per lane and stage, its powers by multiplication
    dft8<INV>(v);
    __syncthreads();
    const int o = ((j - k) << 3) + k;
#pragma unroll
    for (int q = 0; q < 8; ++q) lds[m.at(o + q * ns)] = v[q];
    __syncthreads();
}

// final radix-R stage (R = 2 or 4) over all M points with M/8 threads: each thread does 8/R butterflies
template <bool INV, int R, typename MAP>
__device__ __forceinline__ void stage_small(double2* lds, int M, int ns, const double2* __restrict__ twM, MAP m)
{
    constexpr int NB = 8 / R;
    const int stride = M / R;
    const int tstep = (M / (R * ns)) * MAP::kTwStep;
    double2 v[NB][R];
    int outBase[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = m.j + b * m.nj;
        const int k = j & (ns - 1);
        outBase[b] = (j - k) * R + k;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            v[b][q] = lds[m.at(j + q * stride)];
            if (q > 0) v[b][q] = cmulw<INV>(v[b][q], twM[q * k * tstep]);
        }
        if (R == 4) dft4<INV>(v[b][0], v[b][1], v[b][2], v[b][3]);
        else { const double2 a = v[b][0], c = v[b][1]; v[b][0] = cadd(a, c); v[b][1] = csub(a, c); }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < R; ++q) lds[m.at(outBase[b] + q * ns)] = v[b][q];
    __syncthreads();
}

// M = 1024, 2048 (P/8 threads, 8 points per thread): radix-8 stages, then one radix-4 or radix-2 stage when M is not a power of 8
template <bool INV>
__device__ __forceinline__ void wg_cfft(double2* lds, int M, const double2* __restrict__ twM)
{
    const WgMap m{ (int)threadIdx.x, (int)blockDim.x };
    int ns = 1;
    while (ns * 8 <= M) { stage8<INV>(lds, M, ns, twM, m); ns *= 8; }
    if (ns * 4 == M) stage_small<INV, 4>(lds, M, ns, twM, m);
    else if (ns * 2 == M) stage_small<INV, 2>(lds, M, ns, twM, m);
}

struct StockhamFft {        // P <= 256: two buffers of P complex, natural order
    static constexpr int kMaxThreads = 256;
    static int threads(int P) { return P / 2 < 64 ? 64 : (P / 2 > 256 ? 256 : P / 2); }
    static size_t ldsBytes(int P) { return 2 * P * sizeof(double2); }
    static __device__ __forceinline__ int at(int i) { return i; }
    template <bool INV>
    static __device__ __forceinline__ double2* cfft(double2* lds, int M, const double2* __restrict__ twM)
    {
        return stockham<INV>(lds, lds + M, M, twM);
    }
};
struct MixedRadixFft {      // P = 1024, 2048: one padded buffer, in place
    static constexpr int kMaxThreads = 512;
    static int threads(int P) { return P / 8; }
    static size_t ldsBytes(int P) { return (size_t)(P + (P >> 3)) * sizeof(double2); }
    static __device__ __forceinline__ int at(int i) { return wgp(i); }
    template <bool INV>
    static __device__ __forceinline__ double2* cfft(double2* lds, int M, const double2* __restrict__ twM)
    {
        wg_cfft<INV>(lds, M, twM);
        return lds;
    }
};

// forward.  FRAME = true: overlap-save frame of (channel, block) = blockIdx.x, spectrum into the FDL ring at slot head + t;
// FRAME = false: zero-padded IR partition blockIdx.x of heff (in), spectrum into row blockIdx.x
template <typename F, bool FRAME>
__global__ __launch_bounds__(F::kMaxThreads) void k_rfft_fwd_lds(const double* __restrict__ in, int64_t chStride,
                                                                 const double* __restrict__ histOld,
                                                                 double* __restrict__ histNew, int heffLen,
                                                                 double2* __restrict__ X, double2* __restrict__ XDN,
                                                                 FftTables tw, int P, int T, int head, int ringMask)
{
    extern __shared__ double2 dyn[];
    const int nthr = blockDim.x;
    const int c = FRAME ? blockIdx.x / T : 0;
    const int t = FRAME ? blockIdx.x - c * T : 0;
    if (FRAME) {
        const OlsFrame frame(in, chStride, histOld, histNew, P, T, c, t);
        for (int n = threadIdx.x; n < P; n += nthr) frame.load(n, dyn[F::at(n)]);
    } else {
        for (int n = threadIdx.x; n < P; n += nthr) dyn[F::at(n)] = ir_part_load(in, heffLen, blockIdx.x, P, n);
    }
    __syncthreads();
    const double2* Z = F::template cfft<false>(dyn, P, tw.tw512);
    const int64_t row = FRAME ? (int64_t)c * (ringMask + 1) + ((head + t) & ringMask) : (int64_t)blockIdx.x;
    double2* spec = X + row * P;
    for (int k = threadIdx.x; k < P; k += nthr) {
        const double2 zk = Z[F::at(k)];
        const double2 zm = Z[F::at((P - k) & (P - 1))];
        double2 xk = rfft_split(zk, zm, [&] { return tw.tw1024[k]; });
        if (k == 0) {
            xk = pack_dcnyq(zk);
            XDN[row] = xk;
        }
        spec[k] = xk;
    }
}

template <int MODE, typename F>
__global__ __launch_bounds__(F::kMaxThreads) void k_rfft_inv_lds(const double2* __restrict__ Y, double* __restrict__ out,
                                                                 int64_t chStride, FftTables tw, int P, int T, OutSpec ro)
{
    extern __shared__ double2 dyn[];
    const int c = blockIdx.x / T;
    const int t = blockIdx.x - c * T;
    const double2* y = Y + (int64_t)blockIdx.x * P;
    const double2 y0 = y[0];
    for (int k = threadIdx.x; k < P; k += blockDim.x) {
        const double2 yk = y[k];
        const double2 ym = y[(P - k) & (P - 1)];
        double2 z = rfft_unsplit(yk, ym, [&] { return tw.tw1024[k]; });
        if (k == 0) z = unpack_dcnyq(y0);
        dyn[F::at(k)] = z;
    }
    __syncthreads();
    const double2* z = F::template cfft<true>(dyn, P, tw.tw512);
    const double s = 1.0 / (double)P;
    const int halfP = P >> 1;
    for (int n = halfP + threadIdx.x; n < P; n += blockDim.x)      // second half of the 2P-sample frame
        store_block2<MODE>(out, chStride, ro, c, t, P, 2 * (n - halfP), make_double2(z[F::at(n)].x * s, z[F::at(n)].y * s));
}

// ---------------------------------------------------------------------------------------------------------
// P = 4096 (8192-point real frames), the partition of the time-batched throughput path.  Four-step transform of the
// 4096 complex points z[n], n = n2 + 512 n1, inside ONE workgroup of eight waves, built on the wave-level 512-point
// transform above (which streams at 5-6 TB/s, twice what a Stockham pipeline with a workgroup barrier behind every stage
// reached at this size):
//   1. thread j = n2 holds z[j + 512 q], q < 8 (coalesced loads): 8-point DFT over n1 in registers, times W4096^(j k1)
//   2. ONE workgroup-level exchange hands row k1 (512 values) to wave k1
//   3. wave k1: 512-point transform over n2 in its own 9 KB slice of the exchange buffer (wave-local exchanges only)
//      -> Z[k1 + 8 k2]
// The spectrum is stored PERMUTED, element k1 * 512 + k2 = bin k1 + 8 k2 (contiguous per wave: coalesced stores), like
// the larger partitions below: the MAC is element-wise and the forward, IR and inverse transforms agree on it; element 0
// is still the packed (DC, Nyquist).  The real-FFT split pairs (k1, k2) with (8 - k1, 511 - k2) for k1 > 0 and with
// (0, (512 - k2) mod 512) for k1 = 0: a second exchange between partner waves.  Three workgroup barriers per frame
// (four in the inverse) instead of eight: forward 1.38 -> 1.33 ms, inverse 1.88 -> 1.70 ms per 1024-block call of 256 streams
// (starting the CU's second workgroup half a frame late changed nothing).  A workgroup walks consecutive frames of one channel; the forward transform
// keeps the half frame that frames t and t + 1 share in registers (every input block is read once).
// Twiddles never come from global memory inside the loop: W4096^(j k1) factors over the octal digits of j into entries of
// three 8 x 8 tables in LDS (3 KB, filled once per workgroup from the engine's extended-precision table; the first two
// are also the tables of the wave-level transform), the split twiddle is one per-thread constant times W16^r.
// Loading frame t + 1 while frame t computes (16 more registers forward, 32 inverse) was built and measured: no gain in
// either kernel, the CU's second workgroup already covers the loads (RESULTS.md, tools/variants/fft_p4_prefetch.patch).
constexpr int kP4 = 4096;
constexpr int kP4Row = kLdsPerWave;     // 576: row stride of the exchange buffer = one wave's scratch slice

// per-lane first powers; the rest of every twiddle set is formed by multiplication (mul_powers)
struct P4Tables { double2 w512[64], w4096[64], w64[8]; };      // W512^lane, W4096^lane, W64^k

__device__ __forceinline__ void p4_load_tables(P4Tables* T, const double2* __restrict__ twM)     // twM[m] = W4096^m
{
    const int i = threadIdx.x;
    if (i < 64) { T->w512[i] = twM[8 * i]; T->w4096[i] = twM[i]; }
    if (i < 8) T->w64[i] = twM[64 * i];
    __syncthreads();
}

// v[k1] *= W4096^(+-j k1), j = lane + 64 w
template <bool INV>
__device__ __forceinline__ void p4_twiddle(double2 (&v)[8], const P4Tables* T, int j)
{
    mul_powers<INV>(v, cmul(T->w4096[j & 63], T->w64[j >> 6]));
}

// partner of element (w, k2) in the real-FFT split, as an index into the exchange buffer
__device__ __forceinline__ int p4_partner(int w, int k2)
{
    return w == 0 ? ((512 - k2) & 511) : (8 - w) * kP4Row + (511 - k2);
}

// one forward frame: in v = z[j + 512 q]; out: the packed spectrum row (permuted) and its (DC, Nyquist) element
__device__ __forceinline__ void p4_forward_frame(double2 (&v)[8], double2* dyn, const P4Tables* tabs, double2 wk,
                                                 double2* __restrict__ spec, double2* __restrict__ dcnyq)
{
    const int j = threadIdx.x, w = j >> 6, lane = j & 63;
    dft8<false>(v);
    p4_twiddle<false>(v, tabs, j);
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) dyn[k1 * kP4Row + j] = v[k1];
    __syncthreads();
    double2* mine = dyn + w * kP4Row;
#pragma unroll
    for (int m = 0; m < 8; ++m) v[m] = mine[lane + 64 * m];
    wave_sync();                            // this wave's reads before it reuses its slice as scratch
    wave_cfft512<false, true>(v, mine, lane, tabs->w512[lane], tabs->w64[lane & 7]);
    // v[r] = Z[w + 8 (lane + 64 r)]; the split needs the partner wave's row
    wave_sync();
#pragma unroll
    for (int r = 0; r < 8; ++r) mine[lane + 64 * r] = v[r];
    __syncthreads();
    // (five of the eight partner addresses are spilled and reloaded per frame -- the kernel sits at its 128 registers; rebuilding
    // them per frame instead removes the scratch traffic and measured SLOWER, 1.15 -> 1.20-1.26 ms: profiles/r03q_ab_fft_partner.txt)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int k2 = lane + 64 * r;
        const double2 zk = v[r];
        const double2 zm = dyn[p4_partner(w, k2)];
        // rfft_split / pack_dcnyq, inline: the kernel sits at its register limit and the helpers change its instruction order
        const double2 e = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));   // (Z[k] + conj Z[4096-k]) / 2
        const double2 d = make_double2(0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y));   // (Z[k] - conj Z[4096-k]) / 2
        const double2 o = make_double2(d.y, -d.x);                                  // -i d
        const double2 tw = cmul(wk, w16(r));                                        // exp(-2 pi i (w + 8 lane + 512 r) / 8192)
        double2 xk = make_double2(e.x + fma(o.x, tw.x, -(o.y * tw.y)), e.y + fma(o.x, tw.y, o.y * tw.x));
        if (w == 0 && k2 == 0) {
            xk = make_double2(zk.x + zk.y, zk.x - zk.y);   // (DC, Nyquist)
            *dcnyq = xk;
        }
        // one 16-byte streaming store per lane: an FDL row is next read by the MAC, never from cache
        __builtin_nontemporal_store(v2d{ xk.x, xk.y }, reinterpret_cast<v2d*>(spec + w * 512 + k2));
    }
    __syncthreads();                        // the partners are done with this wave's slice before the next frame writes
}

__global__ __launch_bounds__(512, 4) void k_rfft_fwd_ols_p4(const double* __restrict__ in, int64_t chStride,
                                                          const double* __restrict__ histOld,
                                                          double* __restrict__ histNew, double2* __restrict__ X,
                                                          double2* __restrict__ XDN, FftTables tw, int T, int split,
                                                          int head, int ringMask)
{
    extern __shared__ double2 dyn[];
    __shared__ P4Tables tabs;
    const int j = threadIdx.x;
    const int c = blockIdx.x / split;
    const int part = blockIdx.x - c * split;
    const int per = (T + split - 1) / split;
    const int t0 = part * per, t1 = min(T, t0 + per);
    if (t0 >= t1) return;
    p4_load_tables(&tabs, tw.tw512);
    const double2 wk = tw.tw1024[(j >> 6) + 8 * (j & 63)];
    const double* base = in + (int64_t)c * chStride;
    // frame t = [block t-1 | block t]; thread j holds complex points n = j + 512 q: n < 2048 from the previous block
    double2 keep[4];
    {
        const double* prev = (t0 > 0) ? (base + (int64_t)(t0 - 1) * kP4) : (histOld + (int64_t)c * kP4);
#pragma unroll
        for (int q = 0; q < 4; ++q) keep[q] = *reinterpret_cast<const double2*>(prev + 2 * (j + 512 * q));
    }
    for (int t = t0; t < t1; ++t) {
        double2 v[8];
        const double* cur = base + (int64_t)t * kP4;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = keep[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[4 + q] = *reinterpret_cast<const double2*>(cur + 2 * (j + 512 * q));
#pragma unroll
        for (int q = 0; q < 4; ++q) keep[q] = v[4 + q];
        if (t == T - 1) {       // overlap history for the next call (prevInputBuf, NUC.cpp:1258)
            double* hn = histNew + (int64_t)c * kP4;
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<double2*>(hn + 2 * (j + 512 * q)) = v[4 + q];
        }
        const int slot = (head + t) & ringMask;
        const int64_t row = (int64_t)c * (ringMask + 1) + slot;
        p4_forward_frame(v, dyn, &tabs, wk, X + row * kP4, XDN + row);
    }
}

// IR partition spectra at P = 4096: frames [h[k P .. (k+1) P) | 0], same permuted layout
__global__ __launch_bounds__(512, 4) void k_ir_spectra_p4(const double* __restrict__ heff, int heffLen,
                                                        double2* __restrict__ H, double2* __restrict__ HDN, FftTables tw)
{
    extern __shared__ double2 dyn[];
    __shared__ P4Tables tabs;
    const int j = threadIdx.x;
    const int k = blockIdx.x;
    p4_load_tables(&tabs, tw.tw512);
    const double2 wk = tw.tw1024[(j >> 6) + 8 * (j & 63)];
    double2 v[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = k * kP4 + 2 * (j + 512 * q);
        v[q] = make_double2(i < heffLen ? heff[i] : 0.0, (i + 1) < heffLen ? heff[i + 1] : 0.0);
        v[4 + q] = make_double2(0.0, 0.0);          // zero-padded second half (NUC.cpp:921-928)
    }
    p4_forward_frame(v, dyn, &tabs, wk, H + (int64_t)k * kP4, HDN + k);
}

template <int MODE>
__global__ __launch_bounds__(512, 4) void k_rfft_inv_ols_p4(const double2* __restrict__ Y, double* __restrict__ out,
                                                          int64_t chStride, FftTables tw, int T, int split, OutSpec ro)
{
    extern __shared__ double2 dyn[];
    __shared__ P4Tables tabs;
    const int j = threadIdx.x, w = j >> 6, lane = j & 63;
    const int c = blockIdx.x / split;
    const int part = blockIdx.x - c * split;
    const int per = (T + split - 1) / split;
    const int t0 = part * per, t1 = min(T, t0 + per);
    if (t0 >= t1) return;
    p4_load_tables(&tabs, tw.tw512);
    const double2 wk = tw.tw1024[w + 8 * lane];
    const double2* ybase = Y + (int64_t)c * T * kP4;
    double2* mine = dyn + w * kP4Row;
    for (int t = t0; t < t1; ++t) {
        double2 v[8];
        const double2* yrow = ybase + (int64_t)t * kP4;
        const double2* y = yrow + w * 512;
        // wave w reads its row of the permuted spectrum and, a second time, the row of its partner wave for the element
        // Y[4096 - k] of the real-FFT split: the second read is served by the L2 (the workgroup reads each row twice within
        // microseconds) and spares the LDS -- the bound of this kernel -- 16 accesses per lane and two workgroup barriers
        double2 pa[8], pb[8];
        // (the partner offsets are rebuilt per frame from a value the compiler cannot see through: kept across the frame loop
        // they cost 16 registers, which were spilled and reloaded per frame)
        int laneP = lane;
        asm volatile("" : "+v"(laneP));
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k2 = lane + 64 * r;
            const int k2p = laneP + 64 * r;
            pa[r] = y[k2];
            pb[r] = yrow[w == 0 ? ((512 - k2p) & 511) : (8 - w) * 512 + (511 - k2p)];
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k2 = lane + 64 * r;
            const double2 a = pa[r], b = pb[r];
            // rfft_unsplit / unpack_dcnyq, inline (as in p4_forward_frame)
            const double2 e = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
            const double2 d = make_double2(0.5 * (a.x - b.x), 0.5 * (a.y + b.y));
            const double2 tk = cmul(wk, w16(r));
            const double2 o = make_double2(fma(d.x, tk.x, d.y * tk.y), fma(d.y, tk.x, -(d.x * tk.y)));   // d * conj(w)
            double2 z = make_double2(e.x - o.y, e.y + o.x);                                              // E + i O
            if (w == 0 && k2 == 0) z = make_double2(0.5 * (a.x + a.y), 0.5 * (a.x - a.y));
            v[r] = z;
        }
        wave_cfft512<true, true>(v, mine, lane, tabs.w512[lane], tabs.w64[lane & 7]);
        // v[m] = C[w][lane + 64 m]: hand column n2 = j to thread j
        wave_sync();
#pragma unroll
        for (int m = 0; m < 8; ++m) mine[lane + 64 * m] = v[m];
        __syncthreads();
#pragma unroll
        for (int k1 = 0; k1 < 8; ++k1) v[k1] = dyn[k1 * kP4Row + j];
        __syncthreads();                    // the next frame's row writes reuse the buffer
        p4_twiddle<true>(v, &tabs, j);
        dft8<true>(v);
        // second half of the 8192-sample frame: x[n], n = j + 512 n1, n1 = 4..7 (NUC.cpp:1332)
        constexpr double s = 1.0 / (double)kP4;
        if (MODE != 0) {
#pragma unroll
            for (int q = 4; q < 8; ++q)
                store_block2<MODE>(out, chStride, ro, c, t, kP4, 2 * (j + 512 * (q - 4)), make_double2(v[q].x * s, v[q].y * s));
        } else {
            double* o = out + (int64_t)c * chStride + (int64_t)t * kP4;
#pragma unroll
            for (int q = 4; q < 8; ++q)
                *reinterpret_cast<double2*>(o + 2 * (j + 512 * (q - 4))) = make_double2(v[q].x * s, v[q].y * s);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Partitions above 4096 samples (P = 8192, 16384, 32768: tail layers of a FilterSpec plan run at the reference's own
// partition size): four-step FFT of the M = P complex points z[n] = x[2n] + i x[2n+1], M = M1 * 512, n = n1 * 512 + n2:
//   column pass: for every column n2 the M1-point FFT over n1, times W_M^(n2 k1)          -> scratch A[k1][n2]
//   row pass   : for every row k1 the 512-point FFT over n2 (the wave-level kernel above) -> Z[k1 + M1 k2]
// The spectrum stays in that PERMUTED order, element k1 * 512 + k2 <-> bin k1 + M1 k2: the MAC is element-wise and
// the forward, IR and inverse transforms agree on it; element 0 is still the packed (DC, Nyquist).  The real-FFT split
// pairs (k1, k2) with (M1 - k1, 511 - k2) for k1 > 0 and with (0, (512 - k2) mod 512) for k1 = 0, so one workgroup of
// two waves transforms the row pair (k1, M1 - k1).  tools/fft_fourstep_proto.py is the numpy model of this scheme.
// tw.tw512 = exp(-2 pi i m / P) and tw.tw1024 = exp(-2 pi i k / 2P), P entries each.

// columns per workgroup in the column pass: a wave-width of them (coalesced 1 KB rows) up to 64-point columns, fewer for the
// 128- / 256-point columns of 65536- / 131072-sample partitions so that the tile stays at 64 KB and the workgroup at 512 threads
__host__ __device__ constexpr int bigCols(int M1) { return M1 <= 64 ? 64 : (M1 == 128 ? 32 : 16); }

// the M1 elements of a column in a [element][column] LDS tile of `cols` columns; thread = (column, j), j < M1 / 8;
// exp(-2 pi i m / M1) = twP[m * 512]
struct ColMap {
    static constexpr int kTwStep = 512;
    int j, nj, col, cols;
    __device__ __forceinline__ int at(int i) const { return i * cols + col; }
};

// M1-point FFT of the thread's column: the first radix-8 stage takes its inputs from registers (v[q] = element
// j + q M1/8), the result ends in LDS in natural order
template <bool INV>
__device__ __forceinline__ void col_fft(double2 (&v)[8], double2* lds, int M1, const double2* __restrict__ twP, ColMap m)
{
    dft8<INV>(v);
#pragma unroll
    for (int q = 0; q < 8; ++q) lds[m.at(8 * m.j + q)] = v[q];
    __syncthreads();
    if (M1 >= 64) {                  // 64 = 8 x 8, 128 = 8 x 8 x 2, 256 = 8 x 8 x 4
        stage8<INV>(lds, M1, 8, twP, m);
        if (M1 == 128) stage_small<INV, 2>(lds, M1, 64, twP, m);
        else if (M1 == 256) stage_small<INV, 4>(lds, M1, 64, twP, m);
    } else if (M1 == 32) stage_small<INV, 4>(lds, M1, 8, twP, m);
    else stage_small<INV, 2>(lds, M1, 8, twP, m);
}

// column pass, forward.  FRAME = true: overlap-save frame [previous P | current P] of (channel c, block t);
// FRAME = false: zero-padded IR partition blockIdx / 8 of heff.  grid = transforms * 8 column tiles, 8 M1 threads.
template <bool FRAME>
__global__ __launch_bounds__(512) void k_big_cols_fwd(const double* __restrict__ in, int64_t chStride,
                                                      const double* __restrict__ histOld, double* __restrict__ histNew,
                                                      int heffLen, double2* __restrict__ A, FftTables tw, int P, int T)
{
    extern __shared__ double2 dyn[];
    const int M1 = P >> 9;
    const int kBigCols = bigCols(M1), nTiles = 512 / kBigCols;
    const int tr = blockIdx.x / nTiles, tile = blockIdx.x - tr * nTiles;
    const int col = threadIdx.x & (kBigCols - 1), j = threadIdx.x / kBigCols;
    const int n2 = tile * kBigCols + col;
    const int stride = M1 >> 3;
    const ColMap m{ j, stride, col, kBigCols };
    double2 v[8];
    if (FRAME) {
        const int c = tr / T, t = tr - c * T;
        const OlsFrame frame(in, chStride, histOld, histNew, P, T, c, t);
#pragma unroll
        for (int q = 0; q < 8; ++q) frame.load((j + q * stride) * 512 + n2, v[q]);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = ir_part_load(in, heffLen, tr, P, (j + q * stride) * 512 + n2);
    }
    col_fft<false>(v, dyn, M1, tw.tw512, m);
    double2* a = A + (int64_t)tr * P;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k1 = j + q * stride;
        a[k1 * 512 + n2] = cmulw<false>(dyn[m.at(k1)], tw.twCol[k1 * 512 + n2]);       // W_M^(n2 k1)
    }
}

// row pass + real-FFT split, forward: workgroup = rows (k1, M1 - k1) of one transform, one wave each
__global__ __launch_bounds__(128) void k_big_rows_fwd(const double2* __restrict__ A, double2* __restrict__ X,
                                                      double2* __restrict__ XDN, FftTables tw, int P, int T, int head,
                                                      int ringMask, int ringRows)
{
    __shared__ double2 lds[2][kLdsPerWave];
    __shared__ double2 rows[2][512];
    const int M1 = P >> 9;
    const int nPairs = (M1 >> 1) + 1;
    const int tr = blockIdx.x / nPairs, k1 = blockIdx.x - tr * nPairs;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int krow = (w == 0) ? k1 : ((M1 - k1) & (M1 - 1));
    const double2* a = A + (int64_t)tr * P + krow * 512;
    double2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = a[lane + 64 * r];
    wave_cfft512<false>(v, lds[w], lane, tw.tw512[lane * M1], tw.tw512[8 * (lane & 7) * M1]);
#pragma unroll
    for (int r = 0; r < 8; ++r) rows[w][lane + 64 * r] = v[r];
    __syncthreads();
    // ringRows > 0: FDL ring of (channel, block); ringRows == 0: IR partition rows (tr = partition)
    int64_t row = tr;
    if (ringRows > 0) {
        const int c = tr / T, t = tr - c * T;
        row = (int64_t)c * ringRows + ((head + t) & ringMask);
    }
    double2* x = X + row * P + krow * 512;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int k2 = lane + 64 * r;
        const double2 zk = v[r];
        const double2 zm = rows[w ^ 1][krow == 0 ? ((512 - k2) & 511) : (511 - k2)];
        double2 xk = rfft_split(zk, zm, [&] { return tw.twSplit[krow * 512 + k2]; });
        if (krow == 0 && k2 == 0) {
            xk = pack_dcnyq(zk);
            XDN[row] = xk;
        }
        x[k2] = xk;
    }
}

// inverse: undo the split, inverse 512-point FFT over k2, conj twiddle -> scratch A'[k1][n2]
__global__ __launch_bounds__(128) void k_big_rows_inv(const double2* __restrict__ Y, double2* __restrict__ A, FftTables tw,
                                                      int P)
{
    __shared__ double2 lds[2][kLdsPerWave];
    __shared__ double2 rows[2][512];
    const int M1 = P >> 9;
    const int nPairs = (M1 >> 1) + 1;
    const int tr = blockIdx.x / nPairs, k1 = blockIdx.x - tr * nPairs;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int krow = (w == 0) ? k1 : ((M1 - k1) & (M1 - 1));
    const double2* y = Y + (int64_t)tr * P + krow * 512;
    const double2 y0 = Y[(int64_t)tr * P];
    // the partner row (M1 - krow) is the other wave's own row (k1 = 0 and M1 / 2: both waves hold the same row): exchanged
    // through LDS like in the forward pass instead of a second read of it from L2
    double2 own[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { own[r] = y[lane + 64 * r]; rows[w][lane + 64 * r] = own[r]; }
    __syncthreads();
    double2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int k2 = lane + 64 * r;
        const double2 yk = own[r];
        const double2 yp = rows[w ^ 1][krow == 0 ? ((512 - k2) & 511) : (511 - k2)];
        double2 z = rfft_unsplit(yk, yp, [&] { return tw.twSplit[krow * 512 + k2]; });
        if (krow == 0 && k2 == 0) z = unpack_dcnyq(y0);
        v[r] = z;
    }
    wave_cfft512<true>(v, lds[w], lane, tw.tw512[lane * M1], tw.tw512[8 * (lane & 7) * M1]);
    double2* a = A + (int64_t)tr * P + krow * 512;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n2 = lane + 64 * r;
        a[n2] = cmulw<true>(v[r], tw.twCol[krow * 512 + n2]);
    }
}

// inverse column pass: M1-point inverse FFT over k1 per column, second half of the frame (n1 >= M1 / 2) to out, 1/M
template <int MODE>
__global__ __launch_bounds__(512) void k_big_cols_inv(const double2* __restrict__ A, double* __restrict__ out,
                                                      int64_t chStride, FftTables tw, int P, int T, OutSpec ro)
{
    extern __shared__ double2 dyn[];
    const int M1 = P >> 9;
    const int kBigCols = bigCols(M1), nTiles = 512 / kBigCols;
    const int tr = blockIdx.x / nTiles, tile = blockIdx.x - tr * nTiles;
    const int col = threadIdx.x & (kBigCols - 1), j = threadIdx.x / kBigCols;
    const int n2 = tile * kBigCols + col;
    const int stride = M1 >> 3;
    const ColMap m{ j, stride, col, kBigCols };
    const double2* a = A + (int64_t)tr * P;
    double2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = a[(j + q * stride) * 512 + n2];
    col_fft<true>(v, dyn, M1, tw.tw512, m);
    const int c = tr / T, t = tr - c * T;
    const double s = 1.0 / (double)P;
    const int halfM = P >> 1;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n1 = j + q * stride;
        if (n1 >= (M1 >> 1)) {
            const double2 z = dyn[m.at(n1)];
            const int n = n1 * 512 + n2;
            store_block2<MODE>(out, chStride, ro, c, t, P, 2 * (n - halfM), make_double2(z.x * s, z.y * s));
        }
    }
}

}  // namespace
void fill_big_twiddles(const double2* tw512, const double2* tw1024, int P, double2* twCol, double2* twSplit)
{
    const int M1 = P >> 9;
    for (int k1 = 0; k1 < M1; ++k1)
        for (int n = 0; n < 512; ++n) {
            twCol[k1 * 512 + n] = tw512[n * k1];
            twSplit[k1 * 512 + n] = tw1024[k1 + M1 * n];
        }
}
namespace {

// H[k][bin] *= gain[bin] for the IR partition spectra of one IR slot (the HC/LC spectral shaping of a non-NULL
// FilterSpec, src/MKLNonUniformConvolver.cpp:433-441); packed bin 0 = (DC * gain[0], Nyquist * gain[P])
// From P = 4096 up the spectra are stored permuted (element k1 * 512 + k2 holds bin k1 + (P / 512) k2, see k_*_p4 / k_big_*).
__global__ __launch_bounds__(256) void k_spectrum_gain(double2* __restrict__ H, double2* __restrict__ HDN,
                                                       const double* __restrict__ gain, int P)
{
    const int k = blockIdx.x;
    double2* row = H + (int64_t)k * P;
    const int M1 = (P >= 4096) ? (P >> 9) : 0;
    for (int e = threadIdx.x; e < P; e += blockDim.x) {
        const int b = M1 ? ((e >> 9) + M1 * (e & 511)) : e;      // bin of element e
        double2 v = row[e];
        if (e == 0) {
            v = make_double2(v.x * gain[0], v.y * gain[P]);
            HDN[k] = v;
        } else {
            v = make_double2(v.x * gain[b], v.y * gain[b]);
        }
        row[e] = v;
    }
}

template <typename K>
void allowLargeLds(K kernel, size_t bytes)
{
    if (bytes > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

// which kernels transform partitions of P samples (the table at the head of this file)
enum class Family { Stockham, Wave512, MixedRadix, P4, FourStep };
static Family fftFamily(int P)
{
    if (P > 4096) return Family::FourStep;
    if (P == kP) return Family::Wave512;
    if (P == kP4) return Family::P4;
    return P >= 1024 ? Family::MixedRadix : Family::Stockham;
}

// launch geometry of the two passes of n four-step transforms (P > 4096); the scratch between them is [n][P]
struct FourStepGeom {
    dim3 colGrid, colBlock, rowGrid, rowBlock;
    size_t colLds;
    FourStepGeom(int P, int n)
    {
        const int M1 = P >> 9, cols = bigCols(M1);
        colGrid = dim3(n * (512 / cols));             // column tiles of every transform
        colBlock = dim3(cols * M1 / 8);
        colLds = (size_t)M1 * cols * sizeof(double2);
        rowGrid = dim3(n * ((M1 >> 1) + 1));          // row pairs (k1, M1 - k1) of every transform
        rowBlock = dim3(128);
    }
};

static size_t p4LdsBytes() { return 8 * kP4Row * sizeof(double2); }      // the exchange buffer: eight rows of kP4Row complex
// frames of one channel are walked by `split` workgroups (contiguous ranges): one per channel when the channels alone
// fill the chip (2 workgroups per CU), more for few channels
static int p4Split(int nCh, int T)
{
    int split = 1;
    while (nCh * split < 2048 && split * 2 <= T) split *= 2;
    return split;
}

// the LDS families: n workgroups, one per transform
template <typename F, bool FRAME, typename... Args>
static void launch_fwd_lds(hipStream_t stream, int n, int P, Args... args)
{
    allowLargeLds(k_rfft_fwd_lds<F, FRAME>, F::ldsBytes(P));
    hipLaunchKernelGGL((k_rfft_fwd_lds<F, FRAME>), dim3(n), dim3(F::threads(P)), F::ldsBytes(P), stream, args...);
}

void launch_rfft_fwd_ols(hipStream_t stream, const double* in, int64_t chStride, const double* histOld,
                         double* histNew, double2* X, double2* XDN, FftTables tw, int P, int nCh, int T, int head,
                         int ringSlots, double2* scratch, int forceSplit)
{
    switch (fftFamily(P)) {
    case Family::FourStep: {      // column pass into scratch [nCh * T][P], then row pass + split into the FDL ring
        const FourStepGeom g(P, nCh * T);
        hipLaunchKernelGGL(k_big_cols_fwd<true>, g.colGrid, g.colBlock, g.colLds, stream, in, chStride, histOld, histNew, 0,
                           scratch, tw, P, T);
        hipLaunchKernelGGL(k_big_rows_fwd, g.rowGrid, g.rowBlock, 0, stream, scratch, X, XDN, tw, P, T, head, ringSlots - 1,
                           ringSlots);
        break;
    }
    case Family::Wave512:
        hipLaunchKernelGGL(k_rfft_fwd_ols<false>, dim3(nCh * T), dim3(64), 0, stream, in, chStride, histOld, histNew, X, XDN,
                           tw, T, head, ringSlots - 1, FwdSide{});
        break;
    case Family::P4: {
        const int split = forceSplit > 0 ? forceSplit : p4Split(nCh, T);
        allowLargeLds(k_rfft_fwd_ols_p4, p4LdsBytes());
        hipLaunchKernelGGL(k_rfft_fwd_ols_p4, dim3(nCh * split), dim3(512), p4LdsBytes(), stream, in, chStride, histOld,
                           histNew, X, XDN, tw, T, split, head, ringSlots - 1);
        break;
    }
    case Family::MixedRadix:
        launch_fwd_lds<MixedRadixFft, true>(stream, nCh * T, P, in, chStride, histOld, histNew, 0, X, XDN, tw, P, T, head, ringSlots - 1);
        break;
    case Family::Stockham:
        launch_fwd_lds<StockhamFft, true>(stream, nCh * T, P, in, chStride, histOld, histNew, 0, X, XDN, tw, P, T, head, ringSlots - 1);
        break;
    }
}

bool rfft_fwd_can_carry_side(int P, int nSide, const int64_t* stride, const int64_t* off, int nTab)
{
    if (P != kP || nSide < 0 || nSide > 2 || nTab < 0 || nTab > kGatherTabMax || nTab > 64) return false;
    for (int a = 0; a < nSide; ++a) if ((off[a] | stride[a]) & 1) return false;      // 16-byte stores into every channel's row
    return true;
}

void launch_rfft_fwd_ols_side(hipStream_t stream, const double* in, int64_t chStride, const double* histOld, double* histNew, double2* X,
                              double2* XDN, FftTables tw, int nCh, int T, int head, int ringSlots, int nSide, double* const* dst,
                              const int64_t* dstStride, const int64_t* dstOff, long long* tabDst, const long long* tab, int nTab,
                              double* tailDst, int64_t tailStride, int tailLen)
{
    FwdSide s{};
    s.tailDst = tailDst; s.tailStride = tailStride; s.tailLen = tailDst ? tailLen : 0;
    s.n = nSide;
    for (int a = 0; a < nSide; ++a) { s.dst[a] = dst[a]; s.stride[a] = dstStride[a]; s.off[a] = dstOff[a]; }
    if (tabDst && tab && nTab > 0) { s.tabDst = tabDst; s.nTab = nTab; for (int i = 0; i < nTab; ++i) s.tab[i] = tab[i]; }
    hipLaunchKernelGGL(k_rfft_fwd_ols<true>, dim3(nCh * T), dim3(64), 0, stream, in, chStride, histOld, histNew, X, XDN, tw, T, head,
                       ringSlots - 1, s);
}

void launch_ir_spectra(hipStream_t stream, const double* heff, int heffLen, double2* H, double2* HDN, FftTables tw,
                       int P, int nParts, double2* scratch)
{
    switch (fftFamily(P)) {
    case Family::FourStep: {      // scratch [nParts][P]
        const FourStepGeom g(P, nParts);
        hipLaunchKernelGGL(k_big_cols_fwd<false>, g.colGrid, g.colBlock, g.colLds, stream, heff, 0, nullptr, nullptr, heffLen,
                           scratch, tw, P, 1);
        hipLaunchKernelGGL(k_big_rows_fwd, g.rowGrid, g.rowBlock, 0, stream, scratch, H, HDN, tw, P, 1, 0, 0, 0);
        break;
    }
    case Family::Wave512:
        hipLaunchKernelGGL(k_ir_spectra, dim3(nParts), dim3(64), 0, stream, heff, heffLen, H, HDN, tw);
        break;
    case Family::P4:
        allowLargeLds(k_ir_spectra_p4, p4LdsBytes());
        hipLaunchKernelGGL(k_ir_spectra_p4, dim3(nParts), dim3(512), p4LdsBytes(), stream, heff, heffLen, H, HDN, tw);
        break;
    case Family::MixedRadix:
        launch_fwd_lds<MixedRadixFft, false>(stream, nParts, P, heff, 0, nullptr, nullptr, heffLen, H, HDN, tw, P, 1, 0, 0);
        break;
    case Family::Stockham:
        launch_fwd_lds<StockhamFft, false>(stream, nParts, P, heff, 0, nullptr, nullptr, heffLen, H, HDN, tw, P, 1, 0, 0);
        break;
    }
}

void launch_spectrum_gain(hipStream_t stream, double2* H, double2* HDN, const double* gain, int P, int nParts)
{
    hipLaunchKernelGGL(k_spectrum_gain, dim3(nParts), dim3(256), 0, stream, H, HDN, gain, P);
}

namespace {
template <int MODE, typename F, typename... Args>
void launch_inv_lds(hipStream_t stream, int n, int P, Args... args)
{
    allowLargeLds(k_rfft_inv_lds<MODE, F>, F::ldsBytes(P));
    hipLaunchKernelGGL((k_rfft_inv_lds<MODE, F>), dim3(n), dim3(F::threads(P)), F::ldsBytes(P), stream, args...);
}

template <int MODE>
void launch_inv(hipStream_t stream, const double2* Y, double* out, int64_t chStride, FftTables tw, int P, int nCh, int T,
                double2* scratch, OutSpec ro, int forceSplit = 0)
{
    switch (fftFamily(P)) {
    case Family::FourStep: {      // scratch [nCh * T][P]
        const FourStepGeom g(P, nCh * T);
        hipLaunchKernelGGL(k_big_rows_inv, g.rowGrid, g.rowBlock, 0, stream, Y, scratch, tw, P);
        hipLaunchKernelGGL(k_big_cols_inv<MODE>, g.colGrid, g.colBlock, g.colLds, stream, scratch, out, chStride, tw, P, T, ro);
        break;
    }
    case Family::Wave512:
        hipLaunchKernelGGL(k_rfft_inv_ols<MODE>, dim3(nCh * T), dim3(64), 0, stream, Y, out, chStride, tw, T, ro);
        break;
    case Family::P4: {
        const int split = forceSplit > 0 ? forceSplit : p4Split(nCh, T);
        allowLargeLds(k_rfft_inv_ols_p4<MODE>, p4LdsBytes());
        hipLaunchKernelGGL(k_rfft_inv_ols_p4<MODE>, dim3(nCh * split), dim3(512), p4LdsBytes(), stream, Y, out, chStride, tw, T,
                           split, ro);
        break;
    }
    case Family::MixedRadix:
        launch_inv_lds<MODE, MixedRadixFft>(stream, nCh * T, P, Y, out, chStride, tw, P, T, ro);
        break;
    case Family::Stockham:
        launch_inv_lds<MODE, StockhamFft>(stream, nCh * T, P, Y, out, chStride, tw, P, T, ro);
        break;
    }
}
}  // namespace

void launch_rfft_inv_ols(hipStream_t stream, const double2* Y, double* out, int64_t chStride, FftTables tw, int P,
                         int nCh, int T, double2* scratch, int forceSplit)
{
    launch_inv<0>(stream, Y, out, chStride, tw, P, nCh, T, scratch, OutSpec{}, forceSplit);
}

void launch_rfft_inv_ols_add(hipStream_t stream, const double2* Y, double* out, int64_t chStride, FftTables tw, int nCh, int T,
                             RingTap a, RingTap b)
{
    OutSpec os{};
    os.ring = const_cast<double*>(a.ring); os.mask = a.ringSize - 1; os.pos = a.sched; os.g1 = a.gain;
    os.ringB = b.ring; os.maskB = b.ringSize - 1; os.schedB = b.sched; os.g2 = b.gain;
    hipLaunchKernelGGL(k_rfft_inv_ols<3>, dim3(nCh * T), dim3(64), 0, stream, Y, out, chStride, tw, T, os);
}

void launch_rfft_inv_ols_ring(hipStream_t stream, const double2* Y, double* ring, int ringSize, const long long* pos,
                              long long pos0, FftTables tw, int P, int nCh, int T, double2* scratch)
{
    OutSpec os{};
    os.ring = ring; os.mask = ringSize - 1; os.pos = pos; os.pos0 = pos0;
    launch_inv<1>(stream, Y, nullptr, 0, tw, P, nCh, T, scratch, os);
}

void launch_rfft_inv_ols_tail(hipStream_t stream, const double2* Y, double* out, int64_t chStride, FftTables tw, int P, int nCh,
                              int T, double2* scratch, const double* layerOut, const double* tailRing, int tailRingSize,
                              const void* tailState, const long long* sched, int nCallbacks, int B, int nTail, double g1, double g2)
{
    OutSpec os{};
    os.layerOut = layerOut; os.tailRing = tailRing; os.tailState = reinterpret_cast<const long long*>(tailState); os.sched = sched;
    os.log2B = 0;
    while ((1 << os.log2B) < B) ++os.log2B;
    os.nCb = nCallbacks; os.B = B; os.tailMask = tailRingSize - 1; os.nTail = nTail; os.nChAll = nCh; os.nSamples = (int)chStride;
    os.g1 = g1; os.g2 = g2;
    launch_inv<2>(stream, Y, out, chStride, tw, P, nCh, T, scratch, os);
}

}  // namespace cpq
