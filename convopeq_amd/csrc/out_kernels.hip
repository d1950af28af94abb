// out_kernels.hip -- the base-rate steps of DSPCore::processOutputDouble with dither off (DSPCoreDouble.cpp:577-744) on gfx950:
//   k_out_pre       UltraHighRateDCBlocker::process (src/UltraHighRateDCBlocker.h:154-187), then x *= kOutputHeadroom and the scrub
//   k_out_headroom  the multiply and the scrub alone (DC blocker off)
//   k_out_post      SimplePeakLimiter::processBlock (src/audioengine/SimplePeakLimiter.h), then the clamp at +-kOutputHeadroom
//
// DC blocker, time-parallel.  One workgroup walks a channel's call in spans of kOpThreads * kOutChunk samples and carries the
// two one-pole states from span to span.  A lane holds kOutChunk consecutive samples.  Per section (a = 1 - alpha):
//   z = z + alpha (u[i] - z) from z = 0                       the chunk's own end state e_c
//   S_c = a^8 S_(c-1) + e_c                                   Hillis-Steele scan: wave shuffles, then LDS across the four waves;
//                                                             the powers of a from the host (long double)
//   s = s + alpha (u[i] - s), u[i] = u[i] - s                 the reference's two statements from the chunk's true start state
// and section 1 takes section 0's output as its input.  The reference keeps a state at the end of a callback only if it is
// finite and below 1e15.  A state is a convex combination of its inputs and its previous value, so while every input of a span
// and section 0's carried state are below 1e14 and section 1's carried state is below 1e15 (as every kept state is), section 0
// stays below 1e14, section 1's input below 2e14 and section 1 below 1e15: no guard can trip and none is evaluated.  A span
// that fails the test is walked by one lane, sample by sample, in the reference's order with the guards at the callback ends.
//
// Limiter.  The envelope update `if (d < env) env = d; else env = 1 + (env - 1) * release` is a data-dependent branch and not
// monotone in env: no scan reproduces it, so it stays sequential where it has to run.  One workgroup per stream walks batches
// of 2048 samples: every lane forms the desired gain d of its samples (pure).  While the carried envelope is a fixed point of
// the release step (1 + (env - 1) * release == env in fp64) and no d of the batch is below it, every update of the batch
// returns env itself and the batch is a streaming pass with that one gain.  1.0 is such a fixed point -- a stream that has
// never limited -- and so is the value a release ends on: in fp64 the release does not come back to 1.0, it stalls a few
// hundred ulps below it (0.9999999999999556 at 8 kHz, 0.9999999999997335 at 48 kHz) and stays there bit for bit.
// Otherwise wave 0 runs the batch's 64-sample groups in order -- a group at a fixed point with no d below it is skipped the
// same way, any other takes its 64 envelope steps one after the other -- and the lanes apply the gains.
#include "kernels.hpp"

#include <algorithm>

namespace cpq {
namespace {

constexpr int kOpThreads = 256;
constexpr int kOpSpan = kOpThreads * kOutChunk;
constexpr int kOqThreads = 256;
constexpr int kOqPer = 8;                           // samples of a batch per lane
constexpr int kOqBatch = kOqThreads * kOqPer;

__device__ __forceinline__ int opPad(int i) { return i + (i >> 3); }
__device__ __forceinline__ bool opAligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
__device__ __forceinline__ double outScrub(double v) { return fabs(v) < 1.0e300 ? v : 0.0; }

// One section over the lane's chunk: u in, u - lowpass out.  carryIn = the state before the span; li = index in this lane's
// chunk of the span's last sample (outside 0..7: another lane holds it), whose state goes to endState.  shW: [4] wave totals.
__device__ __forceinline__ void outSection(const double* __restrict__ t, double u[kOutChunk], double carryIn, double* shW, int li,
                                           double& endState)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double alpha = t[0];
    const double* pow2 = t + 1;
    const double* lanePow = t + 1 + kOutScanSteps;
    double z = 0.0;
#pragma unroll
    for (int i = 0; i < kOutChunk; ++i) z = z + alpha * (u[i] - z);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int d = 1 << k;
        const double up = __shfl_up(z, d);
        if (lane >= d) z = z + pow2[k] * up;
    }
    __syncthreads();                                // the previous use of shW is over
    if (lane == 63) shW[wave] = z;
    __syncthreads();
    double inc = carryIn;                           // state entering this wave
    for (int w = 0; w < wave; ++w) inc = pow2[6] * inc + shW[w];
    double e = __shfl_up(z, 1);
    if (lane == 0) e = 0.0;
    double s = e + lanePow[lane] * inc;
#pragma unroll
    for (int i = 0; i < kOutChunk; ++i) {
        s = s + alpha * (u[i] - s);
        u[i] = u[i] - s;
        if (i == li) endState = s;
    }
}

// in and out may be the same rows
template <bool HEADROOM>
__global__ void __launch_bounds__(kOpThreads)
k_out_pre(const double* in, int64_t inStride, double* out, int64_t outStride, int n, int cb, const double* __restrict__ tab,
          double* __restrict__ state)
{
    __shared__ double buf[kOpSpan + kOpSpan / 8 + 8];
    __shared__ double shW[4];
    __shared__ double carry[2];
    const int ch = blockIdx.x, tid = threadIdx.x;
    const double* x = in + ch * inStride;
    double* y = out + ch * outStride;
    const double* t0 = tab;
    const double* t1 = tab + kOutSectionDoubles;
    const bool alIn = opAligned(x), alOut = opAligned(y);          // spans start at even samples
    if (tid < 2) carry[tid] = state[2 * ch + tid];
    for (int s0 = 0; s0 < n; s0 += kOpSpan) {
        const int len = min(kOpSpan, n - s0);
        __syncthreads();                            // carry is written, buf is free
        int bad = 0;
        for (int p = tid; p < kOpSpan / 2; p += kOpThreads) {
            const int j = 2 * p;
            double a = 0.0, b = 0.0;
            if (j + 1 < len) {
                if (alIn) { const double2 v = reinterpret_cast<const double2*>(x + s0)[p]; a = v.x; b = v.y; }
                else { a = x[s0 + j]; b = x[s0 + j + 1]; }
            } else if (j < len) {
                a = x[s0 + j];
            }
            bad |= !(fabs(a) < 1.0e14) || !(fabs(b) < 1.0e14);
            buf[opPad(j)] = a;
            buf[opPad(j + 1)] = b;
        }
        if (tid == 0) bad |= !(fabs(carry[0]) < 1.0e14) || !(fabs(carry[1]) < 1.0e15);
        if (__syncthreads_or(bad)) {
            // guarded path: the reference's loop, one lane
            if (tid == 0) {
                const double a0 = t0[0], a1 = t1[0];
                double st0 = carry[0], st1 = carry[1];
                for (int i = 0; i < len; ++i) {
                    double v = buf[opPad(i)];
                    st0 = st0 + a0 * (v - st0);
                    v = v - st0;
                    st1 = st1 + a1 * (v - st1);
                    v = v - st1;
                    buf[opPad(i)] = v;
                    const int g = s0 + i;
                    if ((g + 1) % cb == 0 || g == n - 1) {
                        st0 = fabs(st0) < 1.0e15 ? st0 : 0.0;
                        st1 = fabs(st1) < 1.0e15 ? st1 : 0.0;
                    }
                }
                carry[0] = st0;
                carry[1] = st1;
            }
            __syncthreads();
        } else {
            double u[kOutChunk];
#pragma unroll
            for (int i = 0; i < kOutChunk; ++i) u[i] = buf[opPad(kOutChunk * tid + i)];
            const int li = len - 1 - kOutChunk * tid;
            const double c0 = carry[0], c1 = carry[1];
            double e0 = 0.0, e1 = 0.0;
            outSection(t0, u, c0, shW, li, e0);
            outSection(t1, u, c1, shW, li, e1);
            __syncthreads();                        // every lane has read carry
            if (li >= 0 && li < kOutChunk) { carry[0] = e0; carry[1] = e1; }
#pragma unroll
            for (int i = 0; i < kOutChunk; ++i) buf[opPad(kOutChunk * tid + i)] = u[i];
            __syncthreads();
        }
        for (int p = tid; p < kOpSpan / 2; p += kOpThreads) {
            const int j = 2 * p;
            if (j >= len) break;
            double a = buf[opPad(j)], b = buf[opPad(j + 1)];
            if (HEADROOM) { a = outScrub(a * kOutHeadroom); b = outScrub(b * kOutHeadroom); }
            if (j + 1 < len) {
                if (alOut) reinterpret_cast<double2*>(y + s0)[p] = make_double2(a, b);
                else { y[s0 + j] = a; y[s0 + j + 1] = b; }
            } else {
                y[s0 + j] = a;
            }
        }
    }
    __syncthreads();
    if (tid < 2) state[2 * ch + tid] = carry[tid];
}

__global__ void __launch_bounds__(256)
k_out_headroom(const double* in, int64_t inStride, double* out, int64_t outStride, int n)
{
    const double* x = in + blockIdx.y * inStride;
    double* y = out + blockIdx.y * outStride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) y[i] = outScrub(x[i] * kOutHeadroom);
}

// juce::jmax: a NaN in the first place stays, one in the second is dropped
__device__ __forceinline__ double oqMax(double a, double b) { return a < b ? b : a; }

__device__ __forceinline__ double oqDesiredGain(double l, double r)
{
    const double clipStart = kOutLimiterThreshold - kOutLimiterKnee * 0.5;
    const double peak = oqMax(fabs(l), fabs(r));
    const double safePeak = oqMax(peak, 1.0e-12);
    double d = 1.0;
    if (safePeak > clipStart) {
        if (safePeak <= kOutLimiterThreshold) {
            const double t = (safePeak - clipStart) / kOutLimiterKnee;
            const double kneeShape = t * t * (3.0 - 2.0 * t);
            d = 1.0 - (1.0 - kOutLimiterThreshold / safePeak) * kneeShape;
        } else {
            d = kOutLimiterThreshold / safePeak;
        }
    }
    return d;
}

__device__ __forceinline__ double oqClamp(double v)
{
    const double t = v > -kOutHeadroom ? v : -kOutHeadroom;
    return t < kOutHeadroom ? t : kOutHeadroom;
}

__device__ __forceinline__ double oqReadLane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// LIMIT: one workgroup per stream (gridDim.y == 1), the batches in order; without it the batches are dealt over gridDim.y
template <bool LIMIT, bool CLAMP>
__global__ void __launch_bounds__(kOqThreads)
k_out_post(const double* in, int64_t inStride, double* out, int64_t outStride, int n, double release, double* __restrict__ envState)
{
    __shared__ double sd[kOqBatch];
    __shared__ double envSh;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* xl = in + 2 * s * inStride;
    const double* xr = xl + inStride;
    double* yl = out + 2 * s * outStride;
    double* yr = yl + outStride;
    double env = LIMIT ? envState[s] : 1.0;
    for (int base = blockIdx.y * kOqBatch; base < n; base += gridDim.y * kOqBatch) {
        double l[kOqPer], r[kOqPer];
#pragma unroll
        for (int k = 0; k < kOqPer; ++k) {
            const int i = base + k * kOqThreads + tid;
            l[k] = i < n ? xl[i] : 0.0;
            r[k] = i < n ? xr[i] : 0.0;
        }
        if (LIMIT) {
            double d[kOqPer];
            int lim = 0;
#pragma unroll
            for (int k = 0; k < kOqPer; ++k) {
                d[k] = oqDesiredGain(l[k], r[k]);       // 1.0 past the end of the call
                lim |= d[k] < env;
            }
            const int any = __syncthreads_or(lim);      // also: every lane has read sd and envSh of the batch before
            if (any || 1.0 + (env - 1.0) * release != env) {
#pragma unroll
                for (int k = 0; k < kOqPer; ++k) sd[k * kOqThreads + tid] = d[k];
                __syncthreads();
                if (wave == 0) {
                    const int len = min(kOqBatch, n - base);
                    for (int g0 = 0; g0 < len; g0 += 64) {
                        const int cnt = min(64, len - g0);
                        const double dl = sd[g0 + lane];
                        double mine = env;
                        if (1.0 + (env - 1.0) * release != env || __ballot(lane < cnt && dl < env) != 0ull) {
                            for (int i = 0; i < cnt; ++i) {
                                const double di = oqReadLane(dl, i);
                                if (di < env) env = di;
                                else env = 1.0 + (env - 1.0) * release;
                                if (lane == i) mine = env;
                            }
                        }
                        sd[g0 + lane] = mine;
                    }
                    if (lane == 0) envSh = env;
                }
                __syncthreads();
                env = envSh;
#pragma unroll
                for (int k = 0; k < kOqPer; ++k) {
                    const double g = sd[k * kOqThreads + tid];
                    l[k] = l[k] * g;
                    r[k] = r[k] * g;
                }
            } else {
#pragma unroll
                for (int k = 0; k < kOqPer; ++k) {
                    l[k] = l[k] * env;
                    r[k] = r[k] * env;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kOqPer; ++k) {
            const int i = base + k * kOqThreads + tid;
            if (i < n) {
                yl[i] = CLAMP ? oqClamp(l[k]) : l[k];
                yr[i] = CLAMP ? oqClamp(r[k]) : r[k];
            }
        }
    }
    if (LIMIT && tid == 0) envState[s] = env;
}

}  // namespace

void launch_out_pre(hipStream_t stream, const double* in, int64_t inStride, double* out, int64_t outStride, int n, int cb, int nCh,
                    bool dcBlock, bool headroom, const double* tab, double* dcState)
{
    if (dcBlock) {
        if (headroom) hipLaunchKernelGGL(k_out_pre<true>, dim3(nCh), dim3(kOpThreads), 0, stream, in, inStride, out, outStride, n, cb, tab, dcState);
        else hipLaunchKernelGGL(k_out_pre<false>, dim3(nCh), dim3(kOpThreads), 0, stream, in, inStride, out, outStride, n, cb, tab, dcState);
    } else if (headroom) {
        hipLaunchKernelGGL(k_out_headroom, dim3(std::min((n + 255) / 256, 1024), nCh), dim3(256), 0, stream, in, inStride, out, outStride, n);
    }
}

void launch_out_post(hipStream_t stream, const double* in, int64_t inStride, double* out, int64_t outStride, int n, int nStreams,
                     bool limiter, bool clamp, double release, double* env)
{
    const dim3 block(kOqThreads);
    if (limiter) {
        if (clamp) hipLaunchKernelGGL((k_out_post<true, true>), dim3(nStreams), block, 0, stream, in, inStride, out, outStride, n, release, env);
        else hipLaunchKernelGGL((k_out_post<true, false>), dim3(nStreams), block, 0, stream, in, inStride, out, outStride, n, release, env);
    } else if (clamp) {
        const int tiles = std::min((n + kOqBatch - 1) / kOqBatch, 256);
        hipLaunchKernelGGL((k_out_post<false, true>), dim3(nStreams, tiles), block, 0, stream, in, inStride, out, outStride, n, release, env);
    }
}

}  // namespace cpq
