// prog_kernels.hip -- gated programme loudness (EBU R 128) per stream on gfx950; the definition and all integer arithmetic of a
// call are prog_plan.hpp's.
//   k_prog_hops    K-weights a call's rows and adds them up on the stream's 100 ms hop grid: hops[stream][h]
//   k_prog_finish  gating, means, maxima and the sort for the loudness range over a stream's hop sums: one ProgRecord per stream
//   k_prog_peak    true peak (BS.1770-4 Annex 2) and sample peak per row, carried over calls; described where it stands
//   k_prog_apply   out = in * gain[stream]
//
// k_prog_hops.  A workgroup is a stream: waves 0-3 take its left row, waves 4-7 its right row, both through the time-parallel
// K-weighting of k_meter_kweight (meter_kernels.hip: the (y, d) scan over spans of 2048 samples, 8 per lane, with the host's
// long-double matrix powers; the section tables are the meters').  The scan is restated here with the wave counted inside its
// channel; meter_kernels.hip is left as it is.  The weighted span stays in LDS.  A span overlaps at most four hops (H >= 800):
// wave w of a channel sums hop k0 + w's samples inside the span, lane-strided, then by a butterfly.  After a barrier one lane per
// hop adds what the hop had before the span (LDS, by span parity; in a call's first span the channel's slot of `part`), and
// either stores L + R -- the hop is complete -- or carries the two sums on.  No atomics: every hop sum has one writer and a fixed
// order for a given call geometry.  At the end of the call the channel's filter state and its partial hop sum go back to memory.
#include "kernels.hpp"
#include "prog_plan.hpp"

namespace cpq {
namespace {

static_assert(kProgChunk == kMeterChunk, "the section tables are the meters'");

__device__ __forceinline__ double progScrub(double v) { return fabs(v) < 1.0e300 ? v : 0.0; }

struct PSec {
    double b0, b1, b2, a2, c;
    const double* pow2;     // [kMeterScanSteps][4]
    const double* lane;     // [64][4]
};

__device__ __forceinline__ PSec progSection(const double* __restrict__ t)
{
    return PSec{ t[0], t[1], t[2], t[4], t[5], t + 8, t + 8 + 4 * kMeterScanSteps };
}

// meterSectionRun for one channel of the workgroup: lane and wave (0 ... 3) inside the channel, shW [4][2] the channel's wave totals
__device__ __forceinline__ void progSectionRun(const PSec& s, double u[kProgChunk], double um1, double um2, const double carryY[2],
                                               double (*shW)[2], double start[2], double dv[kProgChunk], int lane, int wave)
{
    double f[kProgChunk];
#pragma unroll
    for (int i = 0; i < kProgChunk; ++i) {
        f[i] = s.b0 * u[i] + s.b1 * um1 + s.b2 * um2;
        um2 = um1;
        um1 = u[i];
    }
    double z1 = 0.0, z2 = 0.0;
#pragma unroll
    for (int i = 0; i < kProgChunk; ++i) {
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
    for (int i = 0; i < kProgChunk; ++i) {
        y2 = f[i] - s.c * y1 + s.a2 * y2;
        y1 = y1 + y2;
        u[i] = y1;
        dv[i] = y2;
    }
}

__global__ void __launch_bounds__(kProgThreads)
k_prog_hops(const double* __restrict__ in, ProgCall c, const double* __restrict__ tab, double* __restrict__ state,
            double* __restrict__ part, double* __restrict__ hops)
{
    __shared__ double bufs[2][kProgBufDoubles];
    __shared__ double shWs[2][4][2];
    __shared__ double carries[2][6];                // x1 x2 | pre y1 d1 | rlb y1 d1 (d1 = y1 - y2), as k_meter_kweight keeps them
    __shared__ double seg[2][kProgSegs];            // [channel][wave]: the wave's hop inside this span
    __shared__ double pend[2][2];                   // [span parity][channel]: the hop that straddles spans
    const int s = blockIdx.x, tid = threadIdx.x, chn = tid / kProgLanes, t = tid % kProgLanes, lane = tid & 63, wave = (tid >> 6) & 3;
    const int ch = 2 * s + chn;
    const double* x = in + (long long)ch * c.stride;
    double* buf = bufs[chn];
    double* carry = carries[chn];
    const PSec pre = progSection(tab), rlb = progSection(tab + kMeterSectionDoubles);
    if (t < 6) carry[t] = state[8 * ch + t];
    if (t == 6) pend[1][chn] = part[ch];            // read by the first span (parity 0) where the call begins inside a hop
    int par = 0;
    for (int s0 = 0; s0 < c.n; s0 += kProgSpan, par ^= 1) {
        const int len = progSpanLen(c, s0);
        __syncthreads();                            // carry and pend are written, buf and seg are free
        for (int i = t; i < kProgSpan; i += kProgLanes) buf[progPad(i)] = i < len ? progScrub(x[s0 + i]) : 0.0;
        __syncthreads();
        double u[kProgChunk];
#pragma unroll
        for (int i = 0; i < kProgChunk; ++i) u[i] = buf[progPad(kProgChunk * t + i)];
        const double xm1 = t ? buf[progPad(kProgChunk * t - 1)] : carry[0];
        const double xm2 = t ? buf[progPad(kProgChunk * t - 2)] : carry[1];
        const double cPre[2] = { carry[2], carry[3] }, cRlb[2] = { carry[4], carry[5] };
        // the state after the span's last sample: the lane that holds it keeps (v[i], v[i - 1]) of the three signals
        const int li = len - 1 - kProgChunk * t;
        const bool holds = li >= 0 && li < kProgChunk;
        double nc[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        auto keep = [&](const double v[kProgChunk], const double w[kProgChunk], int at) {
#pragma unroll
            for (int i = 0; i < kProgChunk; ++i)
                if (i == li) { nc[at] = v[i]; nc[at + 1] = w[i]; }
        };
        double dv[kProgChunk];
        dv[0] = xm1;
#pragma unroll
        for (int i = 1; i < kProgChunk; ++i) dv[i] = u[i - 1];
        if (holds) keep(u, dv, 0);
        double stPre[2], stRlb[2];
        progSectionRun(pre, u, xm1, xm2, cPre, shWs[chn], stPre, dv, lane, wave);
        if (holds) keep(u, dv, 2);
        progSectionRun(rlb, u, stPre[0], stPre[0] - stPre[1], cRlb, shWs[chn], stRlb, dv, lane, wave);
        if (holds) keep(u, dv, 4);
        __syncthreads();                            // every lane has read buf and carry
        if (holds) {
#pragma unroll
            for (int i = 0; i < 6; ++i) carry[i] = nc[i];
        }
#pragma unroll
        for (int i = 0; i < kProgChunk; ++i) buf[progPad(kProgChunk * t + i)] = u[i];
        __syncthreads();
        // the hops that overlap [s0, s0 + len): one to a wave of each channel
        const int k0 = progHopAt(c, s0), k1 = progHopAt(c, s0 + len - 1);
        if (k0 + wave <= k1) {
            const ProgSeg g = progSeg(c, k0 + wave, s0, len);
            double sum = 0.0;
            for (int i = g.a + lane; i < g.b; i += 64) {
                const double y = buf[progPad(i - s0)];
                sum = sum + y * y;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) sum = sum + __shfl_xor(sum, d);
            if (lane == 0) seg[chn][wave] = sum;
        }
        __syncthreads();
        if (tid <= k1 - k0) {                       // lane j: hop k0 + j, left then right
            const ProgSeg g = progSeg(c, k0 + tid, s0, len);
            double l = seg[0][tid], r = seg[1][tid];
            if (g.carried) { l = pend[par ^ 1][0] + l; r = pend[par ^ 1][1] + r; }
            if (g.complete) hops[(long long)s * c.maxHops + k0 + tid] = l + r;
            else { pend[par][0] = l; pend[par][1] = r; }
        }
    }
    __syncthreads();
    if (t < 6) state[8 * ch + t] = carry[t];
    if (t == 6 && c.fillOut) part[ch] = pend[par ^ 1][chn];     // par has moved on: the last span's parity
}

// one workgroup per stream over its nHops hop sums
__global__ void __launch_bounds__(kProgFinishLanes)
k_prog_finish(const double* __restrict__ hops, ProgFinish f, ProgRecord* __restrict__ out)
{
    __shared__ double srt[kProgSortMax];
    __shared__ double shSum[kProgFinishLanes], shMx[kProgFinishLanes];
    __shared__ int shCnt[kProgFinishLanes];
    const int tid = threadIdx.x;
    const double* E = hops + (long long)blockIdx.x * f.maxHops;
    auto reduce = [&](const ProgAcc& a) {
        __syncthreads();                            // the previous result has been read
        shSum[tid] = a.sum; shCnt[tid] = a.cnt; shMx[tid] = a.mx;
        __syncthreads();
        for (int st = kProgFinishLanes / 2; st >= 1; st >>= 1) {
            if (tid < st) progTreeStep(shSum, shCnt, shMx, tid, st);
            __syncthreads();
        }
        return ProgAcc{ shSum[0], shCnt[0], shMx[0] };
    };
    const ProgAcc abs = reduce(progLaneGate(E, f, 4, 3, 1, tid, f.zAbs, -HUGE_VAL));
    const ProgAcc rel = reduce(progLaneGate(E, f, 4, 3, 1, tid, f.zAbs, 0.1 * progMean(abs)));
    const ProgAcc sMax = reduce(progLaneGate(E, f, 30, 29, 1, tid, HUGE_VAL, HUGE_VAL));
    const ProgAcc sAbs = reduce(progLaneGate(E, f, 30, 29, 10, tid, f.zAbs, -HUGE_VAL));
    const int nCand = progShortCount(f.nHops), P = progSortSize(nCand);      // nCand <= kProgSortMax: refused at create otherwise
    const double meanShort = progMean(sAbs);
    ProgAcc k{ 0.0, 0, 0.0 };
    for (int j = tid; j < P; j += kProgFinishLanes) {
        const double v = j < nCand ? progShortKept(E, f, j, meanShort) : HUGE_VAL;
        srt[j] = v;
        k.cnt += v < HUGE_VAL;
    }
    const int kept = reduce(k).cnt;                 // its barriers also publish srt
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < P; i += kProgFinishLanes) progSortStep(srt, i, j, kk);
            __syncthreads();
        }
    if (tid == 0) {
        ProgRecord r;
        r.zInt = progMean(rel); r.zGate = progMean(abs); r.zMomMax = abs.mx; r.zShortMax = sMax.mx;
        r.zLo = kept ? srt[progPick10(kept)] : 0.0;
        r.zHi = kept ? srt[progPick95(kept)] : 0.0;
        r.nAbs = abs.cnt; r.nRel = rel.cnt; r.nShortAbs = sAbs.cnt; r.nShortKept = kept;
        out[blockIdx.x] = r;
    }
}

// k_prog_peak.  A workgroup of kPeakThreads lanes is a row.  It walks the row in tiles of kPeakTile samples, scrubbed into LDS
// behind a halo of kPeakHist samples: the row's history in the call's first tile, the previous tile's tail afterwards.  A lane holds
// kPeakPer outputs and their kPeakWindow inputs in registers (progPeakLane), all phases of c.mask.  The lane maxima meet in a wave
// butterfly and then in LDS; lane 0 folds them into the row's running maxima, lanes 0 ... 10 write the new history, which is the
// last tile's buffer at [len, len + 11): [old history | call] where the call is shorter than the history.  One writer per row.
__global__ void __launch_bounds__(kPeakThreads)
k_prog_peak(const double* __restrict__ in, PeakCall c, double* __restrict__ pk)
{
    __shared__ double buf[kPeakBufDoubles];
    __shared__ double shMax[kPeakThreads / 64][2];
    const int row = blockIdx.x, t = threadIdx.x;
    const double* x = in + (long long)row * c.stride;
    double* st = pk + (long long)row * kPeakState;
    if (t < kPeakHist) buf[progPeakPad(t)] = st[t];
    double tp = 0.0, sp = 0.0;
    int len = 0;
    for (int s0 = 0; s0 < c.n; s0 += kPeakTile) {
        len = progPeakTileLen(c, s0);
        __syncthreads();                            // the halo is written, the tile before it has been read
        for (int i = t; i < kPeakTile; i += kPeakThreads) buf[progPeakPad(kPeakHist + i)] = i < len ? progPeakScrub(x[s0 + i]) : 0.0;
        __syncthreads();
        double w[kPeakWindow];
#pragma unroll
        for (int m = 0; m < kPeakWindow; ++m) w[m] = buf[progPeakPad(kPeakPer * t + m)];
        progPeakLane(w, len - kPeakPer * t, c.mask, tp, sp);
        if (s0 + kPeakTile < c.n) {                 // a full tile with another behind it: its tail is that one's halo
            const double h = t < kPeakHist ? buf[progPeakPad(kPeakTile + t)] : 0.0;
            __syncthreads();                        // every window has been read
            if (t < kPeakHist) buf[progPeakPad(t)] = h;
        }
    }
    if (!c.mask) tp = sp;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double a = __shfl_xor(tp, d), b = __shfl_xor(sp, d);
        tp = a > tp ? a : tp;
        sp = b > sp ? b : sp;
    }
    if ((t & 63) == 0) { shMax[t >> 6][0] = tp; shMax[t >> 6][1] = sp; }
    __syncthreads();
    if (t < kPeakHist) st[t] = buf[progPeakPad(len + t)];
    if (t == 0) {
        double a = st[kPeakTp], b = st[kPeakSp];
        for (int wv = 0; wv < kPeakThreads / 64; ++wv) {
            a = shMax[wv][0] > a ? shMax[wv][0] : a;
            b = shMax[wv][1] > b ? shMax[wv][1] : b;
        }
        st[kPeakTp] = a;
        st[kPeakSp] = b;
    }
}

// out = in * gain[row / 2]: one rounding, nothing scrubbed.  in and out may be the same rows, so neither is __restrict__: every
// element is read and written by the same lane.  c.wide: two samples per access, the odd last one alone
__global__ void __launch_bounds__(kApplyThreads)
k_prog_apply(const double* in, ApplyCall c, const double* __restrict__ gain, double* out)
{
    const int row = blockIdx.y;
    const double g = gain[row >> 1];
    const double* x = in + (long long)row * c.inStride;
    double* y = out + (long long)row * c.outStride;
    const int step = gridDim.x * kApplyThreads, first = blockIdx.x * kApplyThreads + threadIdx.x;
    if (c.wide) {
        const int pairs = c.n >> 1;
        for (int i = first; i < pairs; i += step) {
            const double2 v = reinterpret_cast<const double2*>(x)[i];
            reinterpret_cast<double2*>(y)[i] = double2{ v.x * g, v.y * g };
        }
        if ((c.n & 1) && first == 0) y[c.n - 1] = x[c.n - 1] * g;
    } else {
        for (int i = first; i < c.n; i += step) y[i] = x[i] * g;
    }
}

}  // namespace

void launch_prog_peak(hipStream_t stream, const double* in, const PeakCall& c, double* pk)
{
    hipLaunchKernelGGL(k_prog_peak, dim3(c.rows), dim3(kPeakThreads), 0, stream, in, c, pk);
}

void launch_prog_apply(hipStream_t stream, const double* in, const ApplyCall& c, const double* gain, double* out)
{
    hipLaunchKernelGGL(k_prog_apply, dim3(progApplyBlocks(c), c.rows), dim3(kApplyThreads), 0, stream, in, c, gain, out);
}

void launch_prog_hops(hipStream_t stream, const double* in, const ProgCall& c, const double* tab, double* state, double* part, double* hops)
{
    hipLaunchKernelGGL(k_prog_hops, dim3(c.streams), dim3(kProgThreads), 0, stream, in, c, tab, state, part, hops);
}

void launch_prog_finish(hipStream_t stream, const double* hops, const ProgFinish& f, int nStreams, ProgRecord* out)
{
    hipLaunchKernelGGL(k_prog_finish, dim3(nStreams), dim3(kProgFinishLanes), 0, stream, hops, f, out);
}

}  // namespace cpq
