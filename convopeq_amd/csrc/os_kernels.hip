// os_kernels.hip -- half-band oversampler stages on gfx950 (CustomInputOversampler, src/CustomInputOversampler.cpp).
//
// After the polyphase split both directions are one contiguous C-tap FIR at the stage's input rate:
//   up   (interpolateStage, :492-568):  out[2n]   = 2 * sum_r c[r] x[n - r]          (convParity 0)
//                                       out[2n+1] = 0.5 * x[n - centerDelayInput]     (centerParity 1)
//   down (decimateStage, :570-723):     y[n] = 0.5 * h[2n - centerTap] + sum_r c[r] h[2n - 2r]
// where x / h run over [history | call input].  A workgroup takes kOsTile consecutive input-rate outputs of one channel:
// the FIR operand (x, or the even phase of h) of the tile plus its C - 1 samples of halo goes to LDS, each lane keeps
// kOsR consecutive outputs in registers and slides a 2 kOsR window over the LDS image, so one LDS read feeds kOsR
// fp64 FMAs; the coefficients are wave-uniform (scalar loads, SGPR operands).  The LDS image has one pad double per
// kOsR, so the lanes' kOsR-strided reads fall on distinct banks.
//
// Histories are per channel and stage, ping-pong: block 0 of a channel writes the next call's history into the other
// buffer while every block reads the current one.  The guards, flushes, silence path, event counters and the per-stream
// auto-clear / hard-fallback state machine run here; the host only flips the ping-pong selectors.
#include "kernels.hpp"

namespace cpq {
namespace {

constexpr int kOsThreads = 256;
constexpr int kOsR = 8;                          // outputs per lane
constexpr int kOsTile = kOsThreads * kOsR;       // outputs per workgroup
constexpr double kOsDenorm = 1.0e-20;            // kDenormThresholdDouble (src/DspNumericPolicy.h:132)

__device__ __forceinline__ bool osBad(double v)
{
    // isBadSample (:24-33): non-finite or |v| > 2^53 -- the magnitude bits above 0x4340000000000000 cover both
    return (static_cast<unsigned long long>(__double_as_longlong(v)) & 0x7FFFFFFFFFFFFFFFull) > 0x4340000000000000ull;
}

__device__ __forceinline__ int osPad(int i) { return i + (i >> 3); }     // one pad double per kOsR = 8

// flags of a stream: [0] corruption pending, [1] consecutive auto-clears, [2] hard fallback, [3] silenced in this down call
// counts of a stream: [0] corruption events, [1] auto-clears

// next history = the last `keep` samples of [old | in(len)]; or the old one unchanged (frozen), or zeros (silence path)
__device__ void osHistoryNext(const double* old, double* nxt, const double* in, int keep, int len, int mode)
{
    for (int i = threadIdx.x; i < keep; i += kOsThreads) {
        double v;
        if (mode == 1) v = old[i];
        else if (mode == 2) v = 0.0;
        else {
            const int j = len + i;
            v = j < keep ? old[j] : in[j - keep];
        }
        nxt[i] = v;
    }
}

// acc[j] += sum_r c[r] * X(base + j - r), X(i) = xs[osPad(i)], r < C
template <int C>
__device__ __forceinline__ void osFir(const double* xs, const double* __restrict__ coef, int base, double acc[kOsR])
{
    double w[2 * kOsR];                          // w[k] = X(base - rb*R - (R-1) + k)
#pragma unroll
    for (int k = kOsR; k < 2 * kOsR - 1; ++k) w[k] = xs[osPad(base - (kOsR - 1) + k)];
    w[2 * kOsR - 1] = 0.0;
#pragma unroll 2
    for (int rb = 0; rb < C / kOsR; ++rb) {
        const int b = base - rb * kOsR - (kOsR - 1);
#pragma unroll
        for (int k = 0; k < kOsR; ++k) w[k] = xs[osPad(b + k)];
#pragma unroll
        for (int q = 0; q < kOsR; ++q) {
            const double c = coef[rb * kOsR + q];
#pragma unroll
            for (int j = 0; j < kOsR; ++j) acc[j] = fma(c, w[j - q + kOsR - 1], acc[j]);
        }
#pragma unroll
        for (int k = 0; k < kOsR - 1; ++k) w[kOsR + k] = w[k];
    }
}

__device__ __forceinline__ void osReportEvents(unsigned* shCount, int stream, int* flags, unsigned long long* counts)
{
    __syncthreads();
    if (threadIdx.x == 0 && *shCount) {
        atomicAdd(&counts[2 * stream], (unsigned long long)*shCount);
        atomicOr(&flags[4 * stream], 1);
    }
}

template <int C>
__global__ void __launch_bounds__(kOsThreads)
k_os_interp(const double* __restrict__ in, int64_t inStride, double* __restrict__ out, int64_t outStride,
            const double* __restrict__ histOld, double* __restrict__ histNew, int keep, const double* __restrict__ coef,
            double centerCoeff, int centerDelay, int n, int* flags, unsigned long long* counts)
{
    __shared__ double xs[(kOsTile + C) * 9 / 8 + 8];
    __shared__ unsigned shCount;
    const int ch = blockIdx.y, stream = ch >> 1;
    const double* x = in + ch * inStride;
    const double* hOld = histOld + (int64_t)ch * keep;
    double* y = out + ch * outStride;
    const bool frozen = flags[4 * stream + 2] != 0;     // hard fallback: silence, the stage does not advance
    if (blockIdx.x == 0) osHistoryNext(hOld, histNew + (int64_t)ch * keep, x, keep, n, frozen ? 1 : 0);
    const int t0 = blockIdx.x * kOsTile;
    if (frozen) {
        for (int i = threadIdx.x; i < kOsTile && t0 + i < n; i += kOsThreads) {
            y[2 * (t0 + i)] = 0.0;
            y[2 * (t0 + i) + 1] = 0.0;
        }
        return;
    }
    if (threadIdx.x == 0) shCount = 0;
    for (int i = threadIdx.x; i < kOsTile + C - 1; i += kOsThreads) {
        const int j = t0 - (C - 1) + i;
        xs[osPad(i)] = j < 0 ? hOld[keep + j] : (j < n ? x[j] : 0.0);
    }
    __syncthreads();
    double acc[kOsR];
#pragma unroll
    for (int j = 0; j < kOsR; ++j) acc[j] = 0.0;
    const int base = threadIdx.x * kOsR + C - 1;        // X(base) = x[t0 + threadIdx.x * R]
    osFir<C>(xs, coef, base, acc);
    unsigned bad = 0;
#pragma unroll
    for (int j = 0; j < kOsR; ++j) {
        const int m = t0 + threadIdx.x * kOsR + j;
        if (m >= n) break;
        // dotProductAvx2 (:159-217): a bad or tiny sum becomes 0 without a flag
        double conv = acc[j];
        if (osBad(conv) || fabs(conv) < kOsDenorm) conv = 0.0;
        double cen = centerCoeff * xs[osPad(base + j - centerDelay)];
        double2 o;
        if (osBad(cen)) {
            ++bad;
            o = make_double2(0.0, 0.0);
        } else {
            conv *= 2.0;
            if (fabs(conv) < kOsDenorm) conv = 0.0;
            if (fabs(cen) < kOsDenorm) cen = 0.0;
            o = make_double2(conv, cen);
        }
        *reinterpret_cast<double2*>(y + 2 * (int64_t)m) = o;
    }
    if (bad) atomicAdd(&shCount, bad);
    osReportEvents(&shCount, stream, flags, counts);
}

template <int C>
__global__ void __launch_bounds__(kOsThreads)
k_os_decim(const double* __restrict__ in, int64_t inStride, double* __restrict__ out, int64_t outStride,
           const double* __restrict__ histOld, double* __restrict__ histNew, int keep, const double* __restrict__ coef,
           double centerCoeff, int centerTap, int n, const int* __restrict__ nonSilent, int* nonSilentNext, int* flags,
           unsigned long long* counts)
{
    __shared__ double xs[(kOsTile + C) * 9 / 8 + 8];
    __shared__ unsigned shCount;
    __shared__ int shNz;
    const int ch = blockIdx.y, stream = ch >> 1;
    const double* h = in + ch * inStride;               // 2n samples
    const double* hOld = histOld + (int64_t)ch * keep;
    double* y = out + ch * outStride;
    // hard fallback or auto-cleared in this call: silence, the history stays (it was cleared by k_os_down_state)
    const bool frozen = flags[4 * stream + 2] != 0 || flags[4 * stream + 3] != 0;
    const bool silent = !frozen && nonSilent[ch] == 0;   // silence path (:583-609): zeros, history zeroed, not shifted
    if (blockIdx.x == 0) osHistoryNext(hOld, histNew + (int64_t)ch * keep, h, keep, 2 * n, frozen ? 1 : silent ? 2 : 0);
    const int t0 = blockIdx.x * kOsTile;
    if (frozen || silent) {
        for (int i = threadIdx.x; i < kOsTile && t0 + i < n; i += kOsThreads) y[t0 + i] = 0.0;
        return;
    }
    if (threadIdx.x == 0) { shCount = 0; shNz = 0; }
    // even phase h[2k] of the tile and its halo
    for (int i = threadIdx.x; i < kOsTile + C - 1; i += kOsThreads) {
        const int k = t0 - (C - 1) + i;
        xs[osPad(i)] = k < 0 ? hOld[keep + 2 * k] : (k < n ? h[2 * k] : 0.0);
    }
    __syncthreads();
    double acc[kOsR];
#pragma unroll
    for (int j = 0; j < kOsR; ++j) acc[j] = 0.0;
    const int base = threadIdx.x * kOsR + C - 1;
    osFir<C>(xs, coef, base, acc);
    unsigned bad = 0;
    bool nz = false;
#pragma unroll
    for (int j = 0; j < kOsR; ++j) {
        const int m = t0 + threadIdx.x * kOsR + j;
        if (m >= n) break;
        const int ci = 2 * m - centerTap;
        const double cen = centerCoeff * (ci < 0 ? hOld[keep + ci] : h[ci]);
        double v = 0.0;
        if (osBad(cen)) ++bad;
        else {
            const double a = cen + acc[j];
            if (osBad(a)) ++bad;
            else v = fabs(a) < kOsDenorm ? 0.0 : a;
        }
        nz = nz || fabs(v) > kOsDenorm;
        y[m] = v;
    }
    if (bad) atomicAdd(&shCount, bad);
    if (nz) shNz = 1;
    osReportEvents(&shCount, stream, flags, counts);
    if (threadIdx.x == 0 && shNz && nonSilentNext) atomicOr(&nonSilentNext[ch], 1);
}

// processDown's prologue (:785-808) per stream, then the history half of the silence test of every stage
__global__ void __launch_bounds__(kOsThreads)
k_os_down_state(OsHistories hs, int nStages, int* flags, unsigned long long* counts, int* nonSilent, int nCh)
{
    __shared__ int shClear;
    const int s = blockIdx.x;
    int* f = flags + 4 * s;
    if (threadIdx.x == 0) {
        int clear = 0;
        if (!f[2]) {
            if (f[0]) {
                f[0] = 0;
                atomicAdd(&counts[2 * s + 1], 1ull);
                f[1] += 1;
                if (f[1] >= 4) f[2] = 1;            // kHardFallbackAutoClearThreshold
                clear = 1;
            } else {
                f[1] = 0;
            }
        }
        f[3] = clear;
        shClear = clear;
    }
    __syncthreads();
    for (int st = 0; st < nStages; ++st) {
        for (int c = 2 * s; c < 2 * s + 2; ++c) {
            double* up = hs.up[st] + (int64_t)c * hs.upKeep[st];
            double* dn = hs.down[st] + (int64_t)c * hs.downKeep[st];
            if (shClear) {                          // clearAllStages
                for (int i = threadIdx.x; i < hs.upKeep[st]; i += kOsThreads) up[i] = 0.0;
                for (int i = threadIdx.x; i < hs.downKeep[st]; i += kOsThreads) dn[i] = 0.0;
            } else {
                bool nz = false;
                for (int i = threadIdx.x; i < hs.downKeep[st]; i += kOsThreads) nz = nz || fabs(dn[i]) > kOsDenorm;
                nz = __syncthreads_or(nz);
                if (threadIdx.x == 0) nonSilent[st * nCh + c] = nz ? 1 : 0;
            }
        }
    }
}

// the input half of the silence test of the top stage: any |v| > 1e-20 in the call's m samples
__global__ void __launch_bounds__(kOsThreads)
k_os_scan(const double* __restrict__ in, int64_t stride, int m, int* nonSilent)
{
    const int ch = blockIdx.y;
    const double* x = in + ch * stride;
    bool nz = false;
    for (int i = blockIdx.x * kOsTile + threadIdx.x; i < m && i < (int)(blockIdx.x + 1) * kOsTile; i += kOsThreads)
        nz = nz || fabs(x[i]) > kOsDenorm;
    nz = __syncthreads_or(nz);
    if (threadIdx.x == 0 && nz) atomicOr(&nonSilent[ch], 1);
}

template <int C>
void interpC(hipStream_t stream, const OsStageArgs& a)
{
    const dim3 grid((a.n + kOsTile - 1) / kOsTile, a.nCh);
    hipLaunchKernelGGL(k_os_interp<C>, grid, dim3(kOsThreads), 0, stream, a.in, a.inStride, a.out, a.outStride, a.histOld,
                       a.histNew, a.keep, a.coef, a.centerCoeff, a.centerOffset, a.n, a.flags, a.counts);
}

template <int C>
void decimC(hipStream_t stream, const OsStageArgs& a, const int* nonSilent, int* nonSilentNext)
{
    const dim3 grid((a.n + kOsTile - 1) / kOsTile, a.nCh);
    hipLaunchKernelGGL(k_os_decim<C>, grid, dim3(kOsThreads), 0, stream, a.in, a.inStride, a.out, a.outStride, a.histOld,
                       a.histNew, a.keep, a.coef, a.centerCoeff, a.centerOffset, a.n, nonSilent, nonSilentNext, a.flags,
                       a.counts);
}

}  // namespace

bool os_conv_count_supported(int c) { return c == 16 || c == 32 || c == 64 || c == 128 || c == 256 || c == 512; }

void launch_os_interp(hipStream_t stream, const OsStageArgs& a)
{
    if (a.n <= 0) return;
    switch (a.convCount) {
        case 16: interpC<16>(stream, a); break;
        case 32: interpC<32>(stream, a); break;
        case 64: interpC<64>(stream, a); break;
        case 128: interpC<128>(stream, a); break;
        case 256: interpC<256>(stream, a); break;
        case 512: interpC<512>(stream, a); break;
        default: break;
    }
}

void launch_os_decim(hipStream_t stream, const OsStageArgs& a, const int* nonSilent, int* nonSilentNext)
{
    if (a.n <= 0) return;
    switch (a.convCount) {
        case 16: decimC<16>(stream, a, nonSilent, nonSilentNext); break;
        case 32: decimC<32>(stream, a, nonSilent, nonSilentNext); break;
        case 64: decimC<64>(stream, a, nonSilent, nonSilentNext); break;
        case 128: decimC<128>(stream, a, nonSilent, nonSilentNext); break;
        case 256: decimC<256>(stream, a, nonSilent, nonSilentNext); break;
        case 512: decimC<512>(stream, a, nonSilent, nonSilentNext); break;
        default: break;
    }
}

void launch_os_down_state(hipStream_t stream, const OsHistories& hs, int nStages, int nStreams, int* flags,
                          unsigned long long* counts, int* nonSilent)
{
    hipLaunchKernelGGL(k_os_down_state, dim3(nStreams), dim3(kOsThreads), 0, stream, hs, nStages, flags, counts, nonSilent,
                       2 * nStreams);
}

void launch_os_scan(hipStream_t stream, const double* in, int64_t stride, int m, int nCh, int* nonSilent)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(k_os_scan, dim3((m + kOsTile - 1) / kOsTile, nCh), dim3(kOsThreads), 0, stream, in, stride, m, nonSilent);
}

}  // namespace cpq
