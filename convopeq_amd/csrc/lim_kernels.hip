// lim_kernels.hip -- the device object of cpq_limiter (engine_lim.cpp): the look-ahead true-peak limiter of lim_plan.hpp, which has
// the definition.  Every index, count, offset and stride is lim_plan.hpp's arithmetic on LimLaunch, which arrives by value: there is
// no table in device memory.  The kernels read hist, gains and the caller's in, and write out, part, hist and tel.
//
//   k_lim_apply  grid (tilesPerRow, streams), kLimThreads lanes.  A workgroup takes kLimTile consecutive outputs of one stream.
//                It stages both channels of u for the tile and its halo in LDS (limVirt: history, the caller's rows with pre-gain
//                and scrub, 0.0 outside; 16-byte loads where a pair of a wide row lies whole inside the call).  From there on no
//                loop checks a bound against the call.  A lane first takes the delayed samples of its outputs into registers,
//                since both stages are written over: r goes over channel 1's stage in rounds of kLimThreads (r[q] reads slots
//                q ... q + 11, a round writes only slots it has read itself: one barrier a round), the sliding minimum runs by
//                doubling steps that swing between the two stages (windows 1, 2, 4, ... 2^k <= M, then one step of M - 2^k), a
//                lane sums the W minima of its pairs of outputs (limEnvelopePair) and stores 16 bytes a pair on a wide row.
//                The tile's smallest a and its count of a < 1.0 go to part[stream][tile].
//   k_lim_keep   one workgroup per stream: the kept tail of u to the front of hist (both rows, ascending chunks, each loaded
//                whole before it is stored), then the tile partials folded into tel[stream] (a minimum and an integer sum: exact
//                in any order).
#include "kernels.hpp"

namespace cpq {

namespace {

__global__ void __launch_bounds__(kLimThreads)
k_lim_apply(const double* __restrict__ hist, const double* __restrict__ gains, const double* __restrict__ in, double* __restrict__ out,
            LimPartial* __restrict__ part, LimLaunch a)
{
    extern __shared__ double lds[];
    __shared__ double shMin[kLimThreads / 64];
    __shared__ int shCnt[kLimThreads / 64];
    const int tid = (int)threadIdx.x, tileIndex = (int)blockIdx.x, st = (int)blockIdx.y;
    const int W = a.W, pitch = limStagePitch(W, kLimTile), len = limStageLen(W, kLimTile);
    double* A = lds;
    double* B = lds + pitch;
    const double g = gains[st];
    const int lo = limStageLo(a, tileIndex);

    // stage: slot s of channel ch is u[ch] at v = lo + s
    {
        const int eLo = lo - a.hLen, e0 = limPairFirst(lo, a.hLen), nIn = a.nVirt - a.hLen;
        for (int j = tid; j < limPairCount(W); j += kLimThreads) {
            const int e = e0 + 2 * j, s = e - eLo;
            const bool whole = a.wide && e >= 0 && e + 1 < nIn && s >= 0 && s + 1 < len;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                double* S = ch ? B : A;
                if (whole) {
                    const double2 v = *reinterpret_cast<const double2*>(in + (long long)(2 * st + ch) * a.inStride + e);
                    S[s] = limPre(v.x, g);
                    S[s + 1] = limPre(v.y, g);
                } else {
                    if (s >= 0 && s < len) S[s] = limVirt(a, hist, in, g, 2 * st + ch, lo + s);
                    if (s + 1 >= 0 && s + 1 < len) S[s + 1] = limVirt(a, hist, in, g, 2 * st + ch, lo + s + 1);
                }
            }
        }
    }
    __syncthreads();

    // the delayed samples of this lane's outputs: pair k of the lane is outputs 2 (tid + k kLimThreads) and the next
    double d0[kLimPairs][2], d1[kLimPairs][2];
#pragma unroll
    for (int k = 0; k < kLimPairs; ++k) {
        const int s = limDelaySlot(W, 2 * (tid + k * kLimThreads));
        d0[k][0] = A[s]; d0[k][1] = A[s + 1];
        d1[k][0] = B[s]; d1[k][1] = B[s + 1];
    }

    // r over B: idle lanes of the last round follow its last position and store nothing
    const int nR = limRCount(W, kLimTile);
    for (int q0 = 0; q0 < nR; q0 += kLimThreads) {
        const int q = q0 + tid, qq = q < nR ? q : nR - 1;
        const double rq = limRequired(A + qq + kPeakHist, B + qq + kPeakHist, a.mask, a.c);
        __syncthreads();                            // every window of the round has been read
        if (q < nR) B[q] = rq;
    }
    __syncthreads();

    // the sliding minimum over M: X holds windows of `have`, Y takes windows of have + step
    double* X = B;
    double* Y = A;
    const int M = limM(W);
    for (int have = 1; have < M;) {
        const int step = 2 * have <= M ? have : M - have;
        for (int q = tid; q < nR; q += kLimThreads) {
            const double x0 = X[q], x1 = X[q >= step ? q - step : q];
            Y[q] = x1 < x0 ? x1 : x0;
        }
        __syncthreads();
        double* t = X; X = Y; Y = t;
        have += step;
    }

    // the envelope, the product, the partial
    double mn = 1.0;
    int cnt = 0;
    const int tile0 = tileIndex * kLimTile;
    double* y0 = out + (long long)(2 * st) * a.outStride;
    double* y1 = y0 + a.outStride;
#pragma unroll
    for (int k = 0; k < kLimPairs; ++k) {
        const int ot = 2 * (tid + k * kLimThreads), o = tile0 + ot;
        double e0, e1;
        limEnvelopePair(X + ot + limReach(W), W, e0, e1);
        if (o + 1 < a.nOut) {
            mn = e0 < mn ? e0 : mn; mn = e1 < mn ? e1 : mn;
            cnt += (e0 < 1.0) + (e1 < 1.0);
            if (a.wide) {
                *reinterpret_cast<double2*>(y0 + o) = double2{ d0[k][0] * e0, d0[k][1] * e1 };
                *reinterpret_cast<double2*>(y1 + o) = double2{ d1[k][0] * e0, d1[k][1] * e1 };
            } else {
                y0[o] = d0[k][0] * e0; y0[o + 1] = d0[k][1] * e1;
                y1[o] = d1[k][0] * e0; y1[o + 1] = d1[k][1] * e1;
            }
        } else if (o < a.nOut) {
            mn = e0 < mn ? e0 : mn;
            cnt += e0 < 1.0;
            y0[o] = d0[k][0] * e0;
            y1[o] = d1[k][0] * e0;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double v = __shfl_xor(mn, d);
        mn = v < mn ? v : mn;
        cnt += __shfl_xor(cnt, d);
    }
    if ((tid & 63) == 0) { shMin[tid >> 6] = mn; shCnt[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        LimPartial p{ 1.0, 0 };
        for (int w = 0; w < kLimThreads / 64; ++w) limFold(p, shMin[w], shCnt[w]);
        part[(long long)st * a.partStride + tileIndex] = p;
    }
}

__global__ void __launch_bounds__(kLimKeepBlock)
k_lim_keep(double* hist, const double* __restrict__ gains, const double* __restrict__ in, const LimPartial* __restrict__ part,
           LimPartial* __restrict__ tel, LimLaunch a)
{
    __shared__ double shMin[kLimKeepBlock];
    __shared__ long long shCnt[kLimKeepBlock];
    const int tid = (int)threadIdx.x, st = (int)blockIdx.x;
    const double g = gains[st];
    for (int chunk = 0; chunk < limKeepChunks(a); ++chunk) {
        const int i = chunk * kLimKeepBlock + tid;
        const bool live = i < a.keepLen;
        const double v0 = live ? limVirt(a, hist, in, g, 2 * st, a.keepShift + i) : 0.0;
        const double v1 = live ? limVirt(a, hist, in, g, 2 * st + 1, a.keepShift + i) : 0.0;
        __syncthreads();
        if (live) {
            hist[(long long)(2 * st) * a.hBound + i] = v0;
            hist[(long long)(2 * st + 1) * a.hBound + i] = v1;
        }
        __syncthreads();
    }
    LimPartial p{ 1.0, 0 };
    for (int t = tid; t < a.tilesPerRow; t += kLimKeepBlock) {
        const LimPartial q = part[(long long)st * a.partStride + t];
        limFold(p, q.minGain, q.limited);
    }
    shMin[tid] = p.minGain; shCnt[tid] = p.limited;
    __syncthreads();
    for (int s = kLimKeepBlock / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            shMin[tid] = shMin[tid + s] < shMin[tid] ? shMin[tid + s] : shMin[tid];
            shCnt[tid] = shCnt[tid] + shCnt[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        LimPartial t = a.first ? LimPartial{ 1.0, 0 } : tel[st];
        limFold(t, shMin[0], shCnt[0]);
        tel[st] = t;
    }
}

}  // namespace

void launch_lim_apply(hipStream_t stream, const double* hist, const double* gains, const double* in, double* out, LimPartial* part, const LimLaunch& a)
{
    hipLaunchKernelGGL(k_lim_apply, dim3((unsigned)a.tilesPerRow, (unsigned)a.streams), dim3(kLimThreads), (size_t)limLdsBytes(a.W), stream,
                       hist, gains, in, out, part, a);
}

void launch_lim_keep(hipStream_t stream, double* hist, const double* gains, const double* in, const LimPartial* part, LimPartial* tel, const LimLaunch& a)
{
    hipLaunchKernelGGL(k_lim_keep, dim3((unsigned)a.streams), dim3(kLimKeepBlock), 0, stream, hist, gains, in, part, tel, a);
}

}  // namespace cpq
