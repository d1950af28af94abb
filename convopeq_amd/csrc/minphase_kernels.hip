// minphase_kernels.hip -- the minimum-phase conversion of cpq_ir_minimum_phase_batch over a batch of rows (a row is one channel
// of one IR): convertToMinimumPhase (src/convolver/ConvolverProcessor.ResampleAndFallback.cpp:333-469) per row,
//   zero-pad to N -> FFT -> ln max(|X|, 1e-300) -> IFFT / N -> fold -> FFT -> clamp +-50, exp(re) (cos im, sin im) -> IFFT / N
//   -> real part of the first n, |v| < 1e-18 -> 0;  a non-finite value after the exponential or in the output marks the row.
//
// One transform core, in LDS: radix-4 butterflies on complex fp64 with a closing (decimation in frequency) or opening (decimation
// in time) radix-2 stage when log2 of the length is odd.  fft_dif takes natural order to bit-reversed order, fft_dit takes
// bit-reversed order to natural order, so a forward transform, a pointwise stage and the inverse behind it need no permutation.
// Stage twiddles are read from one table of the 4096th roots; a value passes at most log4(length) twiddle products.
//
//   k_minphase_small   N <= 4096: one workgroup, the row stays in LDS from the samples in to the samples out
//   k_cfft_cols        N = N1 N2: the N1-point transforms down the columns of the [N1][N2] scratch, a tile of adjacent columns
//                      per workgroup (8 columns = one 128-byte line; 4 at N1 = 2048, where 8 would not fit LDS)
//   k_cfft_rows        the N2-point transforms along its rows
// Forward = columns, twiddle w_N^(k1 n2), rows: X[k1 + N1 k2] is left at [k1][k2].  Inverse = rows, conjugate twiddle, columns,
// from that layout back to natural order.  So the row pass of a forward transform, the pointwise stage on the spectrum and the
// row pass of the inverse are one kernel (kRowsLog, kRowsExp), and the column pass of an inverse, the fold and the column pass
// of the next forward are one kernel (kColsInvFoldFwd): five passes over the scratch for the four transforms.
//
// -ffp-contract=off: no product here is fused; log, exp, hypot and sincos are the device library's full-precision functions.
#include "kernels.hpp"

namespace cpq {

namespace {

constexpr int kThreads = kMinphaseThreads;
constexpr int kRootLog2 = kMinphaseRootLog2;

__device__ inline double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ inline double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ inline double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
template <bool INV> __device__ inline double2 root(const double2* __restrict__ roots, int idx)
{
    double2 w = roots[idx];
    if (INV) w.y = -w.y;
    return w;
}
// times -i (forward) or +i (inverse)
template <bool INV> __device__ inline double2 quarterTurn(double2 a) { return INV ? make_double2(-a.y, a.x) : make_double2(a.y, -a.x); }
__device__ inline int bitrev(int v, int bits) { return bits ? (int)(__brev((unsigned)v) >> (32 - bits)) : 0; }

// nT transforms of 2^lg points, transform t at s + t * stride: natural order in, bit-reversed order out.  Ends on a barrier.
template <bool INV> __device__ void fft_dif(double2* s, int lg, int nT, int stride, const double2* __restrict__ roots, int tid)
{
    int span = lg;      // log2 of the sub-transforms this stage splits
    while (span >= 2) {
        const int lgQ = span - 2, q = 1 << lgQ, step = 1 << (kRootLog2 - span), lgPer = lg - 2;
        for (int b = tid; b < (nT << lgPer); b += kThreads) {
            const int t = b >> lgPer, r = b & ((1 << lgPer) - 1), j = r & (q - 1);
            double2* p = s + t * stride + ((r >> lgQ) << span) + j;
            const double2 x0 = p[0], x1 = p[q], x2 = p[2 * q], x3 = p[3 * q];
            const double2 t0 = cadd(x0, x2), t1 = csub(x0, x2), t2 = cadd(x1, x3), t3 = quarterTurn<INV>(csub(x1, x3));
            p[0] = cadd(t0, t2);
            p[q] = cmul(csub(t0, t2), root<INV>(roots, 2 * j * step));
            p[2 * q] = cmul(cadd(t1, t3), root<INV>(roots, j * step));
            p[3 * q] = cmul(csub(t1, t3), root<INV>(roots, 3 * j * step));
        }
        __syncthreads();
        span -= 2;
    }
    if (span == 1) {
        const int lgPer = lg - 1;
        for (int b = tid; b < (nT << lgPer); b += kThreads) {
            double2* p = s + (b >> lgPer) * stride + 2 * (b & ((1 << lgPer) - 1));
            const double2 a = p[0], c = p[1];
            p[0] = cadd(a, c);
            p[1] = csub(a, c);
        }
        __syncthreads();
    }
}

// the transpose of fft_dif: bit-reversed order in, natural order out.  Ends on a barrier.
template <bool INV> __device__ void fft_dit(double2* s, int lg, int nT, int stride, const double2* __restrict__ roots, int tid)
{
    int span = 0;       // log2 of the sub-transforms that are finished
    if (lg & 1) {
        const int lgPer = lg - 1;
        for (int b = tid; b < (nT << lgPer); b += kThreads) {
            double2* p = s + (b >> lgPer) * stride + 2 * (b & ((1 << lgPer) - 1));
            const double2 a = p[0], c = p[1];
            p[0] = cadd(a, c);
            p[1] = csub(a, c);
        }
        __syncthreads();
        span = 1;
    }
    while (span < lg) {
        const int q = 1 << span, step = 1 << (kRootLog2 - span - 2), lgPer = lg - 2;
        for (int b = tid; b < (nT << lgPer); b += kThreads) {
            const int t = b >> lgPer, r = b & ((1 << lgPer) - 1), j = r & (q - 1);
            double2* p = s + t * stride + ((r >> span) << (span + 2)) + j;
            const double2 a0 = p[0];
            const double2 b1 = cmul(p[q], root<INV>(roots, 2 * j * step));
            const double2 b2 = cmul(p[2 * q], root<INV>(roots, j * step));
            const double2 b3 = cmul(p[3 * q], root<INV>(roots, 3 * j * step));
            const double2 p0 = cadd(a0, b1), p1 = csub(a0, b1), p2 = cadd(b2, b3), p3 = quarterTurn<INV>(csub(b2, b3));
            p[0] = cadd(p0, p2);
            p[q] = cadd(p1, p3);
            p[2 * q] = csub(p0, p2);
            p[3 * q] = csub(p1, p3);
        }
        __syncthreads();
        span += 2;
    }
}

// w_N^m (conjugated for the inverse) from the two-level table
template <bool INV> __device__ inline double2 rootN(MinphaseTables t, int m)
{
    double2 w = cmul(t.hi[m >> 12], t.lo[m & 4095]);
    if (INV) w.y = -w.y;
    return w;
}

__device__ inline double2 logMagnitude(double2 v)
{
    double m = hypot(v.x, v.y);
    m = m < 1.0e-300 ? 1.0e-300 : m;         // a NaN stays a NaN, as in the reference's std::max(mag, 1e-300)
    return make_double2(log(m), 0.0);
}

// jlimit(-50, 50, .) on both parts (a NaN passes), then exp(re) (cos im, sin im); bad: a part is not finite
__device__ inline double2 clampExp(double2 v, int& bad)
{
    const double re = v.x < -50.0 ? -50.0 : (50.0 < v.x ? 50.0 : v.x), im = v.y < -50.0 ? -50.0 : (50.0 < v.y ? 50.0 : v.y);
    const double m = exp(re);
    double sn, cs;
    sincos(im, &sn, &cs);
    const double2 e = make_double2(m * cs, m * sn);
    if (!isfinite(e.x) || !isfinite(e.y)) bad = 1;
    return e;
}

// cepstrum element g of N after the inverse's 1 / N: bin 0 and N / 2 real, below N / 2 real * 2, the rest zero
__device__ inline double2 fold(double2 v, int g, int N, double invN)
{
    const double re = v.x * invN;
    const int half = N >> 1;
    return make_double2(g == 0 || g == half ? re : (g < half ? re * 2.0 : 0.0), 0.0);
}

__device__ inline double extract(double2 v, double invN, int& bad)
{
    double re = v.x * invN;
    if (!isfinite(re)) bad = 1;
    if (fabs(re) < 1.0e-18) re = 0.0;
    return re;
}

__global__ void __launch_bounds__(kThreads) k_minphase_small(const double* __restrict__ x, double* __restrict__ y,
                                                             const MinphaseRow* __restrict__ rows, int* __restrict__ flags,
                                                             MinphaseTables t, int lg)
{
    extern __shared__ double2 s[];
    const int tid = (int)threadIdx.x, N = 1 << lg;
    const MinphaseRow row = rows[blockIdx.x];
    const double invN = 1.0 / (double)N;
    int bad = 0;
    for (int i = tid; i < N; i += kThreads) s[i] = make_double2(i < row.n ? x[row.off + i] : 0.0, 0.0);
    __syncthreads();
    fft_dif<false>(s, lg, 1, 0, t.roots, tid);
    for (int i = tid; i < N; i += kThreads) s[i] = logMagnitude(s[i]);
    __syncthreads();
    fft_dit<true>(s, lg, 1, 0, t.roots, tid);
    for (int i = tid; i < N; i += kThreads) s[i] = fold(s[i], i, N, invN);
    __syncthreads();
    fft_dif<false>(s, lg, 1, 0, t.roots, tid);
    for (int i = tid; i < N; i += kThreads) s[i] = clampExp(s[i], bad);
    __syncthreads();
    fft_dit<true>(s, lg, 1, 0, t.roots, tid);
    for (int i = tid; i < row.n; i += kThreads) y[row.off + i] = extract(s[i], invN, bad);
    if (bad) atomicOr(&flags[blockIdx.x], 1);
}

// workgroup = (row, tile of C adjacent columns); LDS holds column c of the tile at s[c * (N1 + 1) ...], so that the C elements of
// one line go to different banks
template <int OP> __global__ void __launch_bounds__(kThreads) k_cfft_cols(double2* __restrict__ z, const double* __restrict__ x,
                                                                          double* __restrict__ y, const MinphaseRow* __restrict__ rows,
                                                                          int* __restrict__ flags, MinphaseTables t, int lg1, int lg2, int lgC)
{
    extern __shared__ double2 s[];
    const int tid = (int)threadIdx.x, N1 = 1 << lg1, N2 = 1 << lg2, C = 1 << lgC, stride = N1 + 1, count = N1 << lgC;
    const int tilesPerRow = N2 >> lgC;
    const long long r = (long long)blockIdx.x / tilesPerRow;
    const int c0 = (int)((long long)blockIdx.x % tilesPerRow) << lgC;
    double2* __restrict__ zr = z + (r << (lg1 + lg2));
    const double invN = 1.0 / (double)(1LL << (lg1 + lg2));
    constexpr bool kInverse = OP == kColsInvFoldFwd || OP == kColsInvExtract || OP == kColsInvComplex;
    MinphaseRow row = MinphaseRow{ 0, 0, 0 };
    if (OP == kColsFwdPad || OP == kColsInvExtract) row = rows[r];
    int bad = 0;

    for (int idx = tid; idx < count; idx += kThreads) {
        const int c = idx & (C - 1), n1 = idx >> lgC, g = (n1 << lg2) + c0 + c;
        s[c * stride + n1] = OP == kColsFwdPad ? make_double2(g < row.n ? x[row.off + g] : 0.0, 0.0) : zr[g];
    }
    __syncthreads();
    if (kInverse) {
        fft_dif<true>(s, lg1, C, stride, t.roots, tid);         // position p holds n1 = bitrev(p)
        for (int idx = tid; idx < count; idx += kThreads) {
            const int c = idx & (C - 1), p = idx >> lgC, g = (bitrev(p, lg1) << lg2) + c0 + c;
            const double2 v = s[c * stride + p];
            if (OP == kColsInvComplex) zr[g] = make_double2(v.x * invN, v.y * invN);
            else if (OP == kColsInvExtract) { if (g < row.n) y[row.off + g] = extract(v, invN, bad); }
            else s[c * stride + p] = fold(v, g, N1 << lg2, invN);
        }
        if (OP == kColsInvFoldFwd) {
            __syncthreads();
            fft_dit<false>(s, lg1, C, stride, t.roots, tid);    // position p holds k1 = p
        }
    } else {
        fft_dif<false>(s, lg1, C, stride, t.roots, tid);        // position p holds k1 = bitrev(p)
    }
    if (OP == kColsFwdPad || OP == kColsFwdComplex || OP == kColsInvFoldFwd) {
        for (int idx = tid; idx < count; idx += kThreads) {
            const int c = idx & (C - 1), p = idx >> lgC, k1 = OP == kColsInvFoldFwd ? p : bitrev(p, lg1);
            zr[(k1 << lg2) + c0 + c] = cmul(s[c * stride + p], rootN<false>(t, k1 * (c0 + c)));
        }
    }
    if (OP == kColsInvExtract && bad) atomicOr(&flags[r], 1);
}

// workgroup = (row, k1): the N2 contiguous points at [k1][.]
template <int OP> __global__ void __launch_bounds__(kThreads) k_cfft_rows(double2* __restrict__ z, int* __restrict__ flags, MinphaseTables t,
                                                                          int lg1, int lg2, double scale)
{
    extern __shared__ double2 s[];
    const int tid = (int)threadIdx.x, N2 = 1 << lg2;
    const long long r = (long long)blockIdx.x >> lg1;
    const int k1 = (int)((long long)blockIdx.x & ((1 << lg1) - 1));
    double2* __restrict__ zr = z + (r << (lg1 + lg2)) + ((long long)k1 << lg2);
    int bad = 0;

    if (OP == kRowsInv) {
        for (int i = tid; i < N2; i += kThreads) s[bitrev(i, lg2)] = zr[i];
    } else {
        for (int i = tid; i < N2; i += kThreads) s[i] = zr[i];
    }
    __syncthreads();
    if (OP != kRowsInv) fft_dif<false>(s, lg2, 1, 0, t.roots, tid);
    if (OP == kRowsFwd) {
        for (int i = tid; i < N2; i += kThreads) zr[bitrev(i, lg2)] = s[i];
        return;
    }
    if (OP == kRowsLog || OP == kRowsExp) {
        for (int i = tid; i < N2; i += kThreads) s[i] = OP == kRowsLog ? logMagnitude(s[i]) : clampExp(s[i], bad);
        __syncthreads();
    }
    fft_dit<true>(s, lg2, 1, 0, t.roots, tid);
    for (int i = tid; i < N2; i += kThreads) {
        const double2 v = cmul(s[i], rootN<true>(t, k1 * i));
        zr[i] = OP == kRowsInv ? make_double2(v.x * scale, v.y * scale) : v;
    }
    if (OP == kRowsExp && bad) atomicOr(&flags[r], 1);
}

template <typename K> void allowLds(K kernel, size_t bytes)
{
    if (bytes > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <int OP> void launchCols(hipStream_t stream, double2* z, const double* x, double* y, const MinphaseRow* rows, int* flags,
                                  MinphaseTables t, int lg1, int lg2, long long nRows)
{
    const int C = minphaseColTile(lg1), lgC = minphaseLog2(C);
    const size_t lds = minphaseColsLds(lg1);
    allowLds(k_cfft_cols<OP>, lds);
    hipLaunchKernelGGL(k_cfft_cols<OP>, dim3((unsigned)(nRows * ((1LL << lg2) / C))), dim3(kThreads), lds, stream, z, x, y, rows, flags, t,
                       lg1, lg2, lgC);
}

template <int OP> void launchRows(hipStream_t stream, double2* z, int* flags, MinphaseTables t, int lg1, int lg2, long long nRows, double scale)
{
    const size_t lds = (size_t)16 << lg2;
    allowLds(k_cfft_rows<OP>, lds);
    hipLaunchKernelGGL(k_cfft_rows<OP>, dim3((unsigned)(nRows << lg1)), dim3(kThreads), lds, stream, z, flags, t, lg1, lg2, scale);
}

}  // namespace

void launch_minphase_small(hipStream_t stream, const double* x, double* y, const MinphaseRow* rows, int* flags, MinphaseTables t, int log2n,
                           long long nRows)
{
    if (nRows <= 0) return;
    const size_t lds = (size_t)16 << log2n;
    allowLds(k_minphase_small, lds);
    hipLaunchKernelGGL(k_minphase_small, dim3((unsigned)nRows), dim3(kThreads), lds, stream, x, y, rows, flags, t, log2n);
}

void launch_cfft_cols(hipStream_t stream, int op, double2* z, const double* x, double* y, const MinphaseRow* rows, int* flags,
                      MinphaseTables t, int log2n1, int log2n2, long long nRows)
{
    if (nRows <= 0) return;
    switch (op) {
    case kColsFwdPad: launchCols<kColsFwdPad>(stream, z, x, y, rows, flags, t, log2n1, log2n2, nRows); break;
    case kColsFwdComplex: launchCols<kColsFwdComplex>(stream, z, x, y, rows, flags, t, log2n1, log2n2, nRows); break;
    case kColsInvFoldFwd: launchCols<kColsInvFoldFwd>(stream, z, x, y, rows, flags, t, log2n1, log2n2, nRows); break;
    case kColsInvExtract: launchCols<kColsInvExtract>(stream, z, x, y, rows, flags, t, log2n1, log2n2, nRows); break;
    default: launchCols<kColsInvComplex>(stream, z, x, y, rows, flags, t, log2n1, log2n2, nRows); break;
    }
}

void launch_cfft_rows(hipStream_t stream, int op, double2* z, int* flags, MinphaseTables t, int log2n1, int log2n2, long long nRows,
                      double scale)
{
    if (nRows <= 0) return;
    switch (op) {
    case kRowsFwd: launchRows<kRowsFwd>(stream, z, flags, t, log2n1, log2n2, nRows, scale); break;
    case kRowsInv: launchRows<kRowsInv>(stream, z, flags, t, log2n1, log2n2, nRows, scale); break;
    case kRowsLog: launchRows<kRowsLog>(stream, z, flags, t, log2n1, log2n2, nRows, scale); break;
    default: launchRows<kRowsExp>(stream, z, flags, t, log2n1, log2n2, nRows, scale); break;
    }
}

}  // namespace cpq
