// pcm_kernels.hip -- packed PCM <-> the engine's fp64 rows on gfx950 (include/convopeq_mi355x.h, "packed PCM in and out").
//
// Pure streaming passes, 3 to 24 bytes per sample.  A workgroup of 256 lanes takes one tile: kPcmTile samples of one row
// (planar) or kPcmTile / 2 stereo frames of one stream (interleaved) -- either way ONE contiguous byte range of the packed side.
// That range goes through the workgroup's LDS as a byte image that keeps the global address modulo 16:
//   unpack  global -> LDS with 16-byte loads on 16-byte-aligned addresses, LDS -> registers per sample (any width, any phase),
//           fp64 rows stored as double2
//   pack    fp64 rows loaded as double2, converted, written to the LDS image per sample, LDS -> global with 16-byte stores
// so an S24 row that starts on an odd byte, or the L/R split of a frame, costs LDS accesses and not narrow global ones.
// The ends of a tile's range that do not fill an aligned 16-byte slot are moved byte by byte (at most 15 + 15 bytes), an fp64 row
// that starts or ends on an odd sample gets one 8-byte access there: no load and no store touches a byte outside the tile's own
// range, hence none outside [base, base + bytes) of either buffer.
//
// CPQ_PCM_SANITIZE: the callback phase of sample i of a row of n is computed here from n and the callback length cb --
// callback i / cb, of min(cb, n - start) samples, scalar tail = its last len % 4 samples.  No table.
#include "kernels.hpp"
#include "pcm_device.hpp"

namespace cpq {
namespace {

constexpr int kPcmThreads = 256;

template <int FMT> struct PcmFmt;
template <> struct PcmFmt<CPQ_PCM_F64> { static constexpr int bps = 8; };
template <> struct PcmFmt<CPQ_PCM_F32> { static constexpr int bps = 4; };
template <> struct PcmFmt<CPQ_PCM_S16> { static constexpr int bps = 2; };
template <> struct PcmFmt<CPQ_PCM_S24> { static constexpr int bps = 3; };
template <> struct PcmFmt<CPQ_PCM_S32> { static constexpr int bps = 4; };

// the LDS image of a tile: byte b of the tile's range lives at img[skew + b], skew = global address & 15; 16 bytes of slack at
// the end for the dword pair an S24 sample is cut from
template <int BPS> constexpr int pcmImageBytes() { return 16 + kPcmTile * BPS + 16; }

struct PcmSpan { int head, body16, tail; };      // bytes before the first aligned slot, whole slots, bytes after the last
__device__ __forceinline__ PcmSpan pcmSpan(int skew, int bytes)
{
    PcmSpan s;
    s.head = min(bytes, (16 - skew) & 15);
    s.body16 = (bytes - s.head) >> 4;
    s.tail = bytes - s.head - (s.body16 << 4);
    return s;
}

// applyHighQuality64BitTransform(gain = 1) on one sample (ir_ingest.cpp sanitizeAndLimit)
__device__ __forceinline__ double pcmSanitize(double v, int i, int n, int cb)
{
    const int start = i / cb * cb;
    const int len = min(cb, n - start);
    const bool scalarTail = i - start >= (len & ~3);
    const bool inf = fabs(v) == __builtin_huge_val();
    if (v != v || fabs(v) < 1.0e-20 || (inf && scalarTail)) v = 0.0;
    v = (-1.0 < v) ? v : -1.0;
    return (v < 1.0) ? v : 1.0;
}

__device__ __forceinline__ double pcmFixedToDouble(int fixed)
{
    constexpr float kFixedToFloat = 1.0f / static_cast<float>(0x7fffffff);
    return (double)(static_cast<float>(fixed) * kFixedToFloat);
}

// the sample at byte `off` of the image (off = skew + index * bps: aligned to the element, S24 at any phase)
template <int FMT>
__device__ __forceinline__ double pcmDecode(const unsigned char* image, int off)
{
    if constexpr (FMT == CPQ_PCM_F64) return *reinterpret_cast<const double*>(image + off);
    else if constexpr (FMT == CPQ_PCM_F32) return (double)*reinterpret_cast<const float*>(image + off);
    else if constexpr (FMT == CPQ_PCM_S32) return pcmFixedToDouble(*reinterpret_cast<const int*>(image + off));
    else if constexpr (FMT == CPQ_PCM_S16) return pcmFixedToDouble((int)((unsigned)*reinterpret_cast<const unsigned short*>(image + off) << 16));
    else {
        // three bytes at any phase: the aligned dword pair around them, shifted
        const unsigned* w = reinterpret_cast<const unsigned*>(image + (off & ~3));
        const unsigned long long pair = ((unsigned long long)w[1] << 32) | w[0];
        return pcmFixedToDouble((int)((unsigned)(pair >> (8 * (off & 3))) << 8));
    }
}

template <int FMT>
__device__ __forceinline__ void pcmEncode(unsigned char* img, int k, double x)
{
    if constexpr (FMT == CPQ_PCM_F64) *reinterpret_cast<double*>(img + 8 * k) = x;
    else if constexpr (FMT == CPQ_PCM_F32) *reinterpret_cast<float*>(img + 4 * k) = (float)x;
    else if constexpr (FMT == CPQ_PCM_S32) *reinterpret_cast<int*>(img + 4 * k) = pcmQuantize<32>(x);
    else if constexpr (FMT == CPQ_PCM_S16) *reinterpret_cast<short*>(img + 2 * k) = (short)pcmQuantize<16>(x);
    else {
        static_assert(FMT == CPQ_PCM_S24, "unknown format");
        const unsigned q = (unsigned)pcmQuantize<24>(x);
        img[3 * k] = (unsigned char)q;
        img[3 * k + 1] = (unsigned char)(q >> 8);
        img[3 * k + 2] = (unsigned char)(q >> 16);
    }
}

// LAYOUT planar: grid (tiles of kPcmTile samples, 2 S rows); interleaved: grid (tiles of kPcmTile / 2 frames, S streams)
template <int FMT, int LAYOUT>
__global__ __launch_bounds__(kPcmThreads) void k_pcm_unpack(const unsigned char* __restrict__ pcm, double* __restrict__ rows, int n, int cb)
{
    constexpr int BPS = PcmFmt<FMT>::bps;
    constexpr int CH = LAYOUT == CPQ_PCM_INTERLEAVED ? 2 : 1;
    constexpr int FR = kPcmTile / CH;
    __shared__ __attribute__((aligned(16))) unsigned char image[pcmImageBytes<BPS>()];
    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * FR;
    const int cnt = min(FR, n - t0);                                 // samples per row in this tile, >= 1
    const size_t unit = blockIdx.y;
    const unsigned char* src = pcm + (unit * (size_t)n + (size_t)t0) * (CH * BPS);
    const int bytes = cnt * CH * BPS;
    const int skew = (int)(reinterpret_cast<uintptr_t>(src) & 15);
    unsigned char* img = image + skew;
    const PcmSpan sp = pcmSpan(skew, bytes);
    {
        const uint4* s16 = reinterpret_cast<const uint4*>(src + sp.head);        // 16-byte aligned (or body16 == 0)
        uint4* d16 = reinterpret_cast<uint4*>(img + sp.head);
        for (int i = tid; i < sp.body16; i += kPcmThreads) d16[i] = s16[i];
        if (tid < sp.head) img[tid] = src[tid];
        const int tb = sp.head + (sp.body16 << 4);
        if (tid >= 64 && tid - 64 < sp.tail) img[tb + tid - 64] = src[tb + tid - 64];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        double* dst = rows + (unit * CH + c) * (size_t)n + t0;
        auto value = [&](int k) {
            const double v = pcmDecode<FMT>(image, skew + (k * CH + c) * BPS);
            return cb > 0 ? pcmSanitize(v, t0 + k, n, cb) : v;
        };
        const int h = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);        // a row that starts on an odd double
        const int pairs = (cnt - h) >> 1;
        if (tid == 0 && h) dst[0] = value(0);
        for (int p = tid; p < pairs; p += kPcmThreads) {
            const int k = h + 2 * p;
            *reinterpret_cast<double2*>(dst + k) = make_double2(value(k), value(k + 1));
        }
        if (tid == kPcmThreads - 1 && ((cnt - h) & 1)) dst[cnt - 1] = value(cnt - 1);
    }
}

template <int FMT, int LAYOUT>
__global__ __launch_bounds__(kPcmThreads) void k_pcm_pack(const double* __restrict__ rows, unsigned char* __restrict__ pcm, int n)
{
    constexpr int BPS = PcmFmt<FMT>::bps;
    constexpr int CH = LAYOUT == CPQ_PCM_INTERLEAVED ? 2 : 1;
    constexpr int FR = kPcmTile / CH;
    __shared__ __attribute__((aligned(16))) unsigned char image[pcmImageBytes<BPS>()];
    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * FR;
    const int cnt = min(FR, n - t0);
    const size_t unit = blockIdx.y;
    unsigned char* dstB = pcm + (unit * (size_t)n + (size_t)t0) * (CH * BPS);
    const int bytes = cnt * CH * BPS;
    const int skew = (int)(reinterpret_cast<uintptr_t>(dstB) & 15);
    unsigned char* img = image + skew;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const double* src = rows + (unit * CH + c) * (size_t)n + t0;
        const int h = (int)((reinterpret_cast<uintptr_t>(src) >> 3) & 1);
        const int pairs = (cnt - h) >> 1;
        if (tid == 0 && h) pcmEncode<FMT>(img, c, src[0]);
        for (int p = tid; p < pairs; p += kPcmThreads) {
            const int k = h + 2 * p;
            const double2 v = *reinterpret_cast<const double2*>(src + k);
            pcmEncode<FMT>(img, k * CH + c, v.x);
            pcmEncode<FMT>(img, (k + 1) * CH + c, v.y);
        }
        if (tid == kPcmThreads - 1 && ((cnt - h) & 1)) pcmEncode<FMT>(img, (cnt - 1) * CH + c, src[cnt - 1]);
    }
    __syncthreads();
    const PcmSpan sp = pcmSpan(skew, bytes);
    const uint4* s16 = reinterpret_cast<const uint4*>(img + sp.head);
    uint4* d16 = reinterpret_cast<uint4*>(dstB + sp.head);                       // 16-byte aligned (or body16 == 0)
    for (int i = tid; i < sp.body16; i += kPcmThreads) d16[i] = s16[i];
    if (tid < sp.head) dstB[tid] = img[tid];
    const int tb = sp.head + (sp.body16 << 4);
    if (tid >= 64 && tid - 64 < sp.tail) dstB[tb + tid - 64] = img[tb + tid - 64];
}

template <int LAYOUT>
dim3 pcmGrid(int n, int nStreams)
{
    constexpr int CH = LAYOUT == CPQ_PCM_INTERLEAVED ? 2 : 1;
    constexpr int FR = kPcmTile / CH;
    return dim3((unsigned)((n + FR - 1) / FR), (unsigned)(nStreams * (2 / CH)));
}

template <int FMT>
void unpackLayout(hipStream_t stream, const void* pcm, int layout, double* rows, int n, int nStreams, int cb)
{
    const unsigned char* p = static_cast<const unsigned char*>(pcm);
    if (layout == CPQ_PCM_INTERLEAVED)
        hipLaunchKernelGGL((k_pcm_unpack<FMT, CPQ_PCM_INTERLEAVED>), pcmGrid<CPQ_PCM_INTERLEAVED>(n, nStreams), dim3(kPcmThreads), 0, stream, p, rows, n, cb);
    else
        hipLaunchKernelGGL((k_pcm_unpack<FMT, CPQ_PCM_PLANAR>), pcmGrid<CPQ_PCM_PLANAR>(n, nStreams), dim3(kPcmThreads), 0, stream, p, rows, n, cb);
}

template <int FMT>
void packLayout(hipStream_t stream, const double* rows, void* pcm, int layout, int n, int nStreams)
{
    unsigned char* p = static_cast<unsigned char*>(pcm);
    if (layout == CPQ_PCM_INTERLEAVED)
        hipLaunchKernelGGL((k_pcm_pack<FMT, CPQ_PCM_INTERLEAVED>), pcmGrid<CPQ_PCM_INTERLEAVED>(n, nStreams), dim3(kPcmThreads), 0, stream, rows, p, n);
    else
        hipLaunchKernelGGL((k_pcm_pack<FMT, CPQ_PCM_PLANAR>), pcmGrid<CPQ_PCM_PLANAR>(n, nStreams), dim3(kPcmThreads), 0, stream, rows, p, n);
}

}  // namespace

bool launch_pcm_unpack(hipStream_t stream, const void* pcm, int format, int layout, double* rows, int n, int nStreams, int sanitizeCb)
{
    switch (format) {
    case CPQ_PCM_F64: unpackLayout<CPQ_PCM_F64>(stream, pcm, layout, rows, n, nStreams, sanitizeCb); return true;
    case CPQ_PCM_F32: unpackLayout<CPQ_PCM_F32>(stream, pcm, layout, rows, n, nStreams, sanitizeCb); return true;
    case CPQ_PCM_S16: unpackLayout<CPQ_PCM_S16>(stream, pcm, layout, rows, n, nStreams, sanitizeCb); return true;
    case CPQ_PCM_S24: unpackLayout<CPQ_PCM_S24>(stream, pcm, layout, rows, n, nStreams, sanitizeCb); return true;
    case CPQ_PCM_S32: unpackLayout<CPQ_PCM_S32>(stream, pcm, layout, rows, n, nStreams, sanitizeCb); return true;
    default: return false;
    }
}

bool launch_pcm_pack(hipStream_t stream, const double* rows, void* pcm, int format, int layout, int n, int nStreams)
{
    switch (format) {
    case CPQ_PCM_F64: packLayout<CPQ_PCM_F64>(stream, rows, pcm, layout, n, nStreams); return true;
    case CPQ_PCM_F32: packLayout<CPQ_PCM_F32>(stream, rows, pcm, layout, n, nStreams); return true;
    case CPQ_PCM_S16: packLayout<CPQ_PCM_S16>(stream, rows, pcm, layout, n, nStreams); return true;     // the callers refuse it without dither
    case CPQ_PCM_S24: packLayout<CPQ_PCM_S24>(stream, rows, pcm, layout, n, nStreams); return true;
    case CPQ_PCM_S32: packLayout<CPQ_PCM_S32>(stream, rows, pcm, layout, n, nStreams); return true;
    default: return false;
    }
}

}  // namespace cpq
