// softclip_kernels.hip -- DSPCore's soft clipper on gfx950 (softClipBlockAVX2, DSPCoreDouble.cpp:133-224): memoryless, in place,
// streaming.  The arithmetic of a sample is softclip_design.hpp's, the same text the host walk compiles.
//
// One lane takes two consecutive samples, an even one and its neighbour, as one 16-byte load and one 16-byte store where the
// row starts on a 16-byte boundary (k_out_pre's rule: rows of an odd length put every other row on an odd double, which is
// then moved 8 bytes at a time; the last sample of an odd row always is).  The reference clips callback by callback and takes
// the last len % 4 samples of a callback of len samples through its scalar loop, so a lane finds its samples' place in their
// callback (the last callback of a call may be shorter) and picks the path per sample.  Both paths return x itself while
// |x| <= threshold - knee, before any arithmetic: a wave whose samples all rest there only moves them, and the tail's three
// divisions are executed by waves that hold a tail sample above it and by no other.  The divisions are plain fp64 `/`, which
// this build (no fast-math) expands to the correctly rounded sequence.  16 bytes of traffic per sample and one table row per
// workgroup; no LDS, no state.
#include "kernels.hpp"
#include "softclip_design.hpp"

#include <algorithm>

namespace cpq {
namespace {

constexpr int kScThreads = 256;
constexpr int kScGridTarget = 8192;         // workgroups of a launch: 32 per CU, the rest of a long row by grid stride

__global__ void __launch_bounds__(kScThreads)
k_soft_clip(double* data, int64_t stride, int n, int cb, const double* __restrict__ tab)
{
    const int ch = blockIdx.y;
    double p[kSoftClipTabDoubles];
#pragma unroll
    for (int k = 0; k < kSoftClipTabDoubles; ++k) p[k] = tab[(ch >> 1) * kSoftClipTabDoubles + k];
    if (p[kScOn] == 0.0) return;                                // the stream rests
    double* x = data + ch * stride;
    const bool al = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
    const int pairs = (n + 1) / 2;
    for (int q = blockIdx.x * kScThreads + threadIdx.x; q < pairs; q += gridDim.x * kScThreads) {
        const int j = 2 * q;
        const bool two = j + 1 < n;
        double a, b = 0.0;
        if (two && al) { const double2 v = *reinterpret_cast<const double2*>(x + j); a = v.x; b = v.y; }
        else { a = x[j]; if (two) b = x[j + 1]; }
        const int i0 = j % cb;
        const int len0 = min(cb, n - (j - i0));
        a = softClipSample(a, i0, len0, p);
        if (two) {
            const bool next = i0 + 1 == cb;                     // the neighbour opens the next callback
            b = softClipSample(b, next ? 0 : i0 + 1, next ? min(cb, n - (j + 1)) : len0, p);
        }
        if (two && al) *reinterpret_cast<double2*>(x + j) = make_double2(a, b);
        else { x[j] = a; if (two) x[j + 1] = b; }
    }
}

}  // namespace

void launch_soft_clip(hipStream_t stream, double* data, int64_t stride, int n, int cb, int nCh, const double* tab)
{
    if (n <= 0 || nCh <= 0) return;
    const int tiles = ((n + 1) / 2 + kScThreads - 1) / kScThreads;
    const int gx = std::min(tiles, std::max(1, kScGridTarget / nCh));
    hipLaunchKernelGGL(k_soft_clip, dim3(gx, nCh), dim3(kScThreads), 0, stream, data, stride, n, cb, tab);
}

}  // namespace cpq
