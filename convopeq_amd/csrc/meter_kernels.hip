// meter_kernels.hip -- the two meters DSPCore runs on its final block (DSPCoreDouble.cpp:695-701) on gfx950:
//   k_meter_kweight    LoudnessMeter::processBlock (src/LoudnessMeter.cpp): two Direct-Form-I biquads in series per channel,
//                      then sum of squares and peak per callback
//   k_meter_true_peak  TruePeakDetector::processBlock (src/TruePeakDetector.cpp): two half-band interpolator stages, max |.|
//   k_meter_finish     the records: mean square and peak of a stream's two channels, the peak-hold replay, the ring
// Both meters read a sample as 0 when it is not finite or |v| >= 1e300 (the scrub at DSPCoreDouble.cpp:665-693).
//
// K-weighting, time-parallel.  One workgroup walks a channel's call in spans of kMwThreads * kMeterChunk samples and carries
// (x1, x2, y1, y2 of both sections) from span to span.  A lane holds kMeterChunk consecutive samples.  Per section:
//   f[i] = b0 u[i] + b1 u[i-1] + b2 u[i-2]                                  the FIR half, no recurrence
//   d[i] = f[i] - c y[i-1] + a2 d[i-1], y[i] = y[i-1] + d[i], c = 1 + a1 + a2   the recursive half on the state (y, d = y - y1);
//                                                                            from a zero state -> e_c, the chunk's own end state
//   S_c = M^8 S_(c-1) + e_c, M = [[1 - c, a2], [-c, a2]]                    Hillis-Steele scan: wave shuffles, then LDS across
//                                                                            the four waves; c and the powers of M from the host
//                                                                            (long double)
//   the same recurrence from the chunk's true start state                   one more pass; section 2 takes y as its u
// The state is (y1, y1 - y2), not (y1, y2): the RLB poles sit at 0.995 (c = 2.5e-5), where the powers of the companion matrix
// grow like k and act on two nearly equal numbers -- measured on the host, the (y1, y2) scan lies 600 - 1450 x further from
// a long-double run than the sequential Direct Form I does, the (y, d) scan 0.8 - 2.7 x.
// The K-weighted span goes to LDS; the callbacks that overlap the span are dealt to the waves, each sums its segment in a
// fixed order (lane-strided, then a butterfly), and a callback that straddles spans is carried in LDS.
//
// True peak.  interpolateStage reads [history | callback | 16 zeros]: a callback sees no sample of the next one, and the
// stage-1 history is the tail of the previous callback's stage-0 output, which itself saw zeros after its last sample.
// Every (callback, 512-sample tile, channel) is one workgroup: the scrubbed input tile with its halo goes to LDS
// (conflict-free padding as in os_kernels.hip), stage 0 slides kMtR outputs per lane through registers and leaves its 2x
// signal in LDS, stage 1 does the same from there and only its max |.| leaves the workgroup (one atomic max on the bit
// pattern of a non-negative double).  Both polyphase branches of a stage are the same dot product one sample apart
// (convParity 0), so each is computed once.  The previous callback's last 8 stage-0 outputs (what stage 1 reaches of its
// history) are recomputed from the 24 samples before the callback with zeros after them, so the only carried state is the
// last 32 scrubbed inputs of a channel.
#include "kernels.hpp"

namespace cpq {
namespace {

constexpr int kMwThreads = 256;
constexpr int kMwSpan = kMwThreads * kMeterChunk;
constexpr int kMtThreads = 128;
constexpr int kMtR = 8;                          // outputs per lane
constexpr int kMtTile = 512;                     // base-rate samples per workgroup
constexpr int kMtLead = 24;                      // input samples before the tile held in LDS
constexpr int kMtIn = kMtTile + 64;              // LDS image of the input: j in [t0 - 24, t0 + 552)
constexpr int kMtMid = 2 * kMtTile + 16;         // stage-0 signal: o in [2 t0 - 8, 2 t0 + 1032)

__device__ __forceinline__ double meterScrub(double v) { return fabs(v) < 1.0e300 ? v : 0.0; }
__device__ __forceinline__ int mtPad(int i) { return i + (i >> 3); }

struct Sec {
    double b0, b1, b2, a2, c;
    const double* pow2;     // [kMeterScanSteps][4]
    const double* lane;     // [64][4]
};

__device__ __forceinline__ Sec meterSection(const double* __restrict__ t)
{
    return Sec{ t[0], t[1], t[2], t[4], t[5], t + 8, t + 8 + 4 * kMeterScanSteps };
}

// One section over the lane's chunk: u (in), um1 / um2 = the two samples before it; returns y in u and y[i] - y[i-1] in dv.
// carryY = state before the span (y1, d1); on return start = the chunk's true start state.  shW: [4][2] wave totals.
__device__ __forceinline__ void meterSectionRun(const Sec& s, double u[kMeterChunk], double um1, double um2, const double carryY[2],
                                                double (*shW)[2], double start[2], double dv[kMeterChunk])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double f[kMeterChunk];
#pragma unroll
    for (int i = 0; i < kMeterChunk; ++i) {
        f[i] = s.b0 * u[i] + s.b1 * um1 + s.b2 * um2;
        um2 = um1;
        um1 = u[i];
    }
    double z1 = 0.0, z2 = 0.0;
#pragma unroll
    for (int i = 0; i < kMeterChunk; ++i) {
        z2 = f[i] - s.c * z1 + s.a2 * z2;
        z1 = z1 + z2;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int d = 1 << k;
        const double t1 = __shfl_up(z1, d), t2 = __shfl_up(z2, d);
        const double* m = s.pow2 + 4 * k;
        if (lane >= d) {
            z1 = z1 + (m[0] * t1 + m[1] * t2);
            z2 = z2 + (m[2] * t1 + m[3] * t2);
        }
    }
    __syncthreads();                                // the previous use of shW is over
    if (lane == 63) { shW[wave][0] = z1; shW[wave][1] = z2; }
    __syncthreads();
    double i1 = carryY[0], i2 = carryY[1];          // state entering this wave
    const double* mw = s.pow2 + 4 * 6;              // M^(chunk * 64)
    for (int w = 0; w < wave; ++w) {
        const double n1 = mw[0] * i1 + mw[1] * i2 + shW[w][0];
        const double n2 = mw[2] * i1 + mw[3] * i2 + shW[w][1];
        i1 = n1;
        i2 = n2;
    }
    double e1 = __shfl_up(z1, 1), e2 = __shfl_up(z2, 1);
    if (lane == 0) { e1 = 0.0; e2 = 0.0; }
    const double* ml = s.lane + 4 * lane;
    double y1 = e1 + (ml[0] * i1 + ml[1] * i2);
    double y2 = e2 + (ml[2] * i1 + ml[3] * i2);
    start[0] = y1;
    start[1] = y2;
#pragma unroll
    for (int i = 0; i < kMeterChunk; ++i) {
        y2 = f[i] - s.c * y1 + s.a2 * y2;
        y1 = y1 + y2;
        u[i] = y1;
        dv[i] = y2;
    }
}

__global__ void __launch_bounds__(kMwThreads)
k_meter_kweight(const double* __restrict__ in, int64_t stride, int n, int cb, const double* __restrict__ tab,
                double* __restrict__ state, double* __restrict__ chSum, double* __restrict__ chPeak, int cbCap)
{
    __shared__ double buf[kMwSpan + kMwSpan / 8 + 8];
    __shared__ double shW[4][2];
    __shared__ double carry[6];                     // x1 x2 | pre y1 d1 | rlb y1 d1 (d1 = y1 - y2)
    __shared__ double pend[2][2];                   // sum, peak of a callback that straddles spans, by span parity
    const int ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* x = in + ch * stride;
    const Sec pre = meterSection(tab), rlb = meterSection(tab + kMeterSectionDoubles);
    if (tid < 6) carry[tid] = state[8 * ch + tid];
    for (int s0 = 0, par = 0; s0 < n; s0 += kMwSpan, par ^= 1) {
        const int len = min(kMwSpan, n - s0);
        __syncthreads();                            // carry is written, buf is free
        for (int i = tid; i < kMwSpan; i += kMwThreads) buf[mtPad(i)] = i < len ? meterScrub(x[s0 + i]) : 0.0;
        __syncthreads();
        double u[kMeterChunk];
#pragma unroll
        for (int i = 0; i < kMeterChunk; ++i) u[i] = buf[mtPad(kMeterChunk * tid + i)];
        const double xm1 = tid ? buf[mtPad(kMeterChunk * tid - 1)] : carry[0];
        const double xm2 = tid ? buf[mtPad(kMeterChunk * tid - 2)] : carry[1];
        const double cPre[2] = { carry[2], carry[3] }, cRlb[2] = { carry[4], carry[5] };
        // the state after the span's last sample: the lane that holds it keeps (v[i], v[i - 1]) of the three signals
        const int li = len - 1 - kMeterChunk * tid;                 // index of that sample in this lane's chunk
        const bool holds = li >= 0 && li < kMeterChunk;
        double nc[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        // (x[i], x[i - 1]) for the input, (y[i], y[i] - y[i - 1]) for the sections
        auto keep = [&](const double v[kMeterChunk], const double w[kMeterChunk], int at) {
#pragma unroll
            for (int i = 0; i < kMeterChunk; ++i)
                if (i == li) { nc[at] = v[i]; nc[at + 1] = w[i]; }
        };
        double dv[kMeterChunk];
        dv[0] = xm1;
#pragma unroll
        for (int i = 1; i < kMeterChunk; ++i) dv[i] = u[i - 1];
        if (holds) keep(u, dv, 0);
        double stPre[2], stRlb[2];
        meterSectionRun(pre, u, xm1, xm2, cPre, shW, stPre, dv);
        if (holds) keep(u, dv, 2);
        meterSectionRun(rlb, u, stPre[0], stPre[0] - stPre[1], cRlb, shW, stRlb, dv);
        if (holds) keep(u, dv, 4);
        __syncthreads();                            // every lane has read buf and carry
        if (holds) {
#pragma unroll
            for (int i = 0; i < 6; ++i) carry[i] = nc[i];
        }
#pragma unroll
        for (int i = 0; i < kMeterChunk; ++i) buf[mtPad(kMeterChunk * tid + i)] = u[i];
        __syncthreads();
        // callbacks that overlap [s0, s0 + len): one wave per segment
        const int k0 = s0 / cb, k1 = (s0 + len - 1) / cb;
        for (int k = k0 + wave; k <= k1; k += 4) {
            const int a = max(k * cb, s0), cbEnd = min((k + 1) * cb, n), b = min(cbEnd, s0 + len);
            double sum = 0.0, pk = 0.0;
            for (int i = a + lane; i < b; i += 64) {
                const double y = buf[mtPad(i - s0)];
                sum = sum + y * y;
                pk = fmax(pk, fabs(y));
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                sum = sum + __shfl_xor(sum, d);
                pk = fmax(pk, __shfl_xor(pk, d));
            }
            if (lane == 0) {
                if (a > k * cb) { sum = pend[par ^ 1][0] + sum; pk = fmax(pend[par ^ 1][1], pk); }
                if (b < cbEnd) { pend[par][0] = sum; pend[par][1] = pk; }
                else { chSum[(int64_t)ch * cbCap + k] = sum; chPeak[(int64_t)ch * cbCap + k] = pk; }
            }
        }
    }
    __syncthreads();
    if (tid < 6) state[8 * ch + tid] = carry[tid];
}

// acc[j] += sum_r c[r] * X(base + j - r), X(i) = xs[mtPad(i)], r < C: kMtR outputs slide over one LDS window (os_kernels.hip, osFir)
template <int C>
__device__ __forceinline__ void mtFir(const double* xs, const double* __restrict__ coef, int base, double acc[kMtR])
{
    double w[2 * kMtR];
#pragma unroll
    for (int k = kMtR; k < 2 * kMtR - 1; ++k) w[k] = xs[mtPad(base - (kMtR - 1) + k)];
    w[2 * kMtR - 1] = 0.0;
#pragma unroll 2
    for (int rb = 0; rb < C / kMtR; ++rb) {
        const int b = base - rb * kMtR - (kMtR - 1);
#pragma unroll
        for (int k = 0; k < kMtR; ++k) w[k] = xs[mtPad(b + k)];
#pragma unroll
        for (int q = 0; q < kMtR; ++q) {
            const double c = coef[rb * kMtR + q];
#pragma unroll
            for (int j = 0; j < kMtR; ++j) acc[j] = fma(c, w[j - q + kMtR - 1], acc[j]);
        }
#pragma unroll
        for (int k = 0; k < kMtR - 1; ++k) w[kMtR + k] = w[k];
    }
}

// the same sum for one output, in the same order: sum_r c[r] * X(at - r)
template <int C>
__device__ __forceinline__ double mtDot(const double* xs, const double* __restrict__ coef, int at)
{
    double acc = 0.0;
    for (int r = 0; r < C; ++r) acc = fma(coef[r], xs[mtPad(at - r)], acc);
    return acc;
}

__global__ void __launch_bounds__(kMtThreads)
k_meter_true_peak(const double* __restrict__ in, int64_t stride, int n, int cb, int tilesPerCb, const double* __restrict__ histOld,
                  double* __restrict__ histNew, const double* __restrict__ coef0, const double* __restrict__ coef1,
                  unsigned long long* __restrict__ tp, int cbCap)
{
    __shared__ double es[kMtIn + kMtIn / 8 + 8];
    __shared__ double fs[kMtMid + kMtMid / 8 + 8];
    __shared__ double shMax[kMtThreads / 64];
    const int ch = blockIdx.y, tid = threadIdx.x;
    const int k = blockIdx.x / tilesPerCb, t0 = (blockIdx.x % tilesPerCb) * kMtTile;
    const double* x = in + ch * stride;
    const double* hOld = histOld + 32 * ch;
    if (blockIdx.x == 0 && tid < 32) {              // the next call's history: the last 32 of [old | call]
        const int j = n + tid;
        histNew[32 * ch + tid] = j < 32 ? hOld[j] : meterScrub(x[j - 32]);
    }
    // e[j], j in [t0 - 24, t0 + 552): before the call from the history, beyond the callback zero
    for (int i = tid; i < kMtIn; i += kMtThreads) {
        const int j = t0 - kMtLead + i, g = k * cb + j;
        es[mtPad(i)] = j >= cb ? 0.0 : (g < 0 ? hOld[32 + g] : meterScrub(x[g]));
    }
    __syncthreads();
    // stage 0: C(m) = sum_r c0[r] e[m + 16 - r]; out[2m] = 0.5 e[m - 15] + C(m), out[2m + 1] = 0.5 e[m - 14] + C(m - 1)
    {
        const int l = min(tid, 65);                 // 66 lanes cover m in [t0 - 8, t0 + 520)
        const int base = kMtR * l + 32;             // X(base + j) = e[m0 + j + 16], m0 = t0 - 8 + 8 l
        double acc[kMtR];
#pragma unroll
        for (int j = 0; j < kMtR; ++j) acc[j] = 0.0;
        mtFir<32>(es, coef0, base, acc);
        double prev = __shfl_up(acc[kMtR - 1], 1);
        if ((tid & 63) == 0) prev = mtDot<32>(es, coef0, base - 1);
        if (tid < 66) {
#pragma unroll
            for (int j = 0; j < kMtR; ++j) {
                const int d = kMtR * l + j - 8;     // m - t0
                const int m = t0 + d;
                if (d >= -4 && d < kMtTile + 4 && m >= 0) {
                    double2 o = make_double2(0.0, 0.0);
                    if (m < cb) {
                        o.x = 0.5 * es[mtPad(d + 9)] + acc[j];
                        o.y = 0.5 * es[mtPad(d + 10)] + (j ? acc[j ? j - 1 : 0] : prev);
                    }
                    fs[mtPad(2 * d + 8)] = o.x;
                    fs[mtPad(2 * d + 9)] = o.y;
                }
            }
        } else if (t0 == 0 && tid < 74) {
            // the previous callback's last 8 stage-0 outputs, o in [-8, 0): the same formulas with zeros from sample 0 on
            const int o = tid - 74, m = o >> 1, q = o & 1;
            double a = 0.0;
            for (int r = 0; r < 32; ++r) {
                const int j = m + 16 - q - r;
                a = fma(coef0[r], j < 0 ? es[mtPad(j + kMtLead)] : 0.0, a);
            }
            fs[mtPad(o + 8)] = 0.5 * es[mtPad(m - 15 + q + kMtLead)] + a;
        }
    }
    __syncthreads();
    // stage 1: D(m) = sum_r c1[r] f[m + 8 - r]; out[2m] = 0.5 f[m - 7] + D(m), out[2m + 1] = 0.5 f[m - 6] + D(m - 1)
    double mx = 0.0;
    {
        const int base = kMtR * tid + 16;           // X(base + j) = f[m0 + j + 8], m0 = 2 t0 + 8 tid
        double acc[kMtR];
#pragma unroll
        for (int j = 0; j < kMtR; ++j) acc[j] = 0.0;
        mtFir<16>(fs, coef1, base, acc);
        double prev = __shfl_up(acc[kMtR - 1], 1);
        if ((tid & 63) == 0) prev = mtDot<16>(fs, coef1, base - 1);
#pragma unroll
        for (int j = 0; j < kMtR; ++j) {
            const int m = 2 * t0 + kMtR * tid + j;
            if (m < 2 * cb) {
                const double p0 = 0.5 * fs[mtPad(kMtR * tid + j + 1)] + acc[j];
                const double p1 = 0.5 * fs[mtPad(kMtR * tid + j + 2)] + (j ? acc[j ? j - 1 : 0] : prev);
                mx = fmax(mx, fmax(fabs(p0), fabs(p1)));
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d));
    if ((tid & 63) == 0) shMax[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kMtThreads / 64; ++w) mx = fmax(mx, shMax[w]);
        atomicMax(&tp[(int64_t)(ch >> 1) * cbCap + k], (unsigned long long)__double_as_longlong(mx));
    }
}

constexpr int kMfThreads = 64;
constexpr int kMfChunk = 1024;

// one workgroup per stream: the records of the call's callbacks; the hold chain is one lane walking LDS
__global__ void __launch_bounds__(kMfThreads)
k_meter_finish(MeterFinishArgs a)
{
    __shared__ double shTp[kMfChunk];
    const int s = blockIdx.x, tid = threadIdx.x;
    const bool loud = (a.flags & CPQ_METER_LOUDNESS) != 0, peak = (a.flags & CPQ_METER_TRUE_PEAK) != 0;
    double hold = peak ? a.hold[s] : 0.0;
    for (int c0 = 0; c0 < a.nCb; c0 += kMfChunk) {
        const int cnt = min(kMfChunk, a.nCb - c0);
        __syncthreads();
        for (int i = tid; i < cnt; i += kMfThreads)
            shTp[i] = peak ? __longlong_as_double((long long)a.tp[(int64_t)s * a.cbCap + c0 + i]) : 0.0;
        __syncthreads();
        if (tid == 0 && peak) {
            // processBlock: peak > peakHold ? peakHold = peak : peakHold *= 0.999; the hold takes the slot, the peak moves on
            for (int i = 0; i < cnt; ++i) {
                const double t = shTp[i];
                hold = t > hold ? t : hold * 0.999;
                shTp[i] = hold;
            }
        }
        __syncthreads();
        for (int i = tid; i < cnt; i += kMfThreads) {
            const int k = c0 + i;
            if (k >= a.nStore) continue;
            cpq_meter_block r;
            r.mean_square = 0.0;
            r.peak_linear = 0.0;
            if (loud) {
                const int len = min(a.cb, a.n - k * a.cb);
                const int64_t l = (int64_t)(2 * s) * a.cbCap + k, rr = l + a.cbCap;
                r.mean_square = (a.chSum[l] + a.chSum[rr]) / (double)len;
                r.peak_linear = fmax(a.chPeak[l], a.chPeak[rr]);
            }
            r.true_peak = peak ? __longlong_as_double((long long)a.tp[(int64_t)s * a.cbCap + k]) : 0.0;
            r.true_peak_hold = shTp[i];
            r.block_index = a.index0 + (unsigned long long)k;
            a.ring[(int64_t)s * a.ringSize + (int64_t)((a.write0 + (unsigned long long)k) % (unsigned long long)a.ringSize)] = r;
        }
    }
    if (tid == 0 && peak) a.hold[s] = hold;
}

}  // namespace

void launch_meter_kweight(hipStream_t stream, const double* in, int64_t stride, int n, int cb, int nCh, const double* tab,
                          double* state, double* chSum, double* chPeak, int cbCap)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_meter_kweight, dim3(nCh), dim3(kMwThreads), 0, stream, in, stride, n, cb, tab, state, chSum, chPeak, cbCap);
}

void launch_meter_true_peak(hipStream_t stream, const double* in, int64_t stride, int n, int cb, int nCh, const double* histOld,
                            double* histNew, const double* coef0, const double* coef1, unsigned long long* tp, int cbCap)
{
    if (n <= 0) return;
    const int tiles = (cb + kMtTile - 1) / kMtTile;
    hipLaunchKernelGGL(k_meter_true_peak, dim3((n / cb) * tiles, nCh), dim3(kMtThreads), 0, stream, in, stride, n, cb, tiles,
                       histOld, histNew, coef0, coef1, tp, cbCap);
}

void launch_meter_finish(hipStream_t stream, const MeterFinishArgs& a, int nStreams)
{
    if (a.nCb <= 0) return;
    hipLaunchKernelGGL(k_meter_finish, dim3(nStreams), dim3(kMfThreads), 0, stream, a);
}

}  // namespace cpq
