// quant_kernels.hip -- cpq_quantizer on gfx950: the stream's gain, the noise shaper and the PCM pack of rows [channel][sample] in
// one launch (include/convopeq_mi355x.h, "word-length reduction").
//
// The skeleton is k_dither's (dither_kernels.hip): one wave per workgroup, a lane owns kDitherCpl consecutive channels and keeps
// their error taps or lattice states and the generator words in registers for the whole call, and a tile of kDitherStep samples x
// the wave's rows goes through LDS at a row pitch of kDitherStep + 1 doubles.  The shapers' arithmetic, the generator and the
// tile load are dither_device.hpp's and lattice_device.hpp's, the integer code is pcm_device.hpp's: nothing of them is restated.
// What is fused around the chain:
//   in    the tile load multiplies row r by the gain of its stream, one rounding; the chain runs at headroom 1.0 without scrub
//   out   the lane that walks a row converts each yq to its code and writes it into an LDS byte image; the tile does not go
//         back out as fp64
//
// The byte image.  A tile's output is one contiguous byte range per channel (planar: len * bps bytes of the channel's packed
// row) or per stream (interleaved: len * 2 * bps bytes, L and R of a frame side by side).  Range g lives at img[g * P + skew + b],
// skew = the range's global address & 15, so a byte's LDS address and its global address agree modulo 16.  The store pass walks
// the image in 16-byte slots, lane = slot: slot k of range g is img[16 (g * P / 16 + k)], consecutive lanes read consecutive
// slots (a linear 16-byte read, conflict-free), and a slot that lies whole inside its range leaves as one aligned 16-byte store.
// The slots a range only partly covers, its first and its last, move byte by byte: at most 15 + 15 single bytes a range, and no
// byte outside a row's [base, base + width) is read or written, so a pitch gap stays as it was.
//
// The slot arithmetic is quant_host.hpp's (quantSlot), where a host program checks it (tests/sanitize/quant_host_check.cpp).
// P = quantImagePitch = kDitherStep * bps * (1 or 2) + 16: room for any skew, and P / 16 is odd.  The chain's writes are one
// element per lane and sample, all lanes at the same sample.  A store's bank is (address / 4) mod 32, and rows that are aligned alike put all those
// addresses on one residue modulo 16, so a write can spread over the 8 sixteen-byte slots of the 128-byte bank row and no
// further: 32 lanes, 8 slots, 4-way at best, whatever the pitch.  An odd P / 16 reaches that best (consecutive ranges rotate
// through all 8 slots; an even one would fold them onto 4 or fewer).  It costs about a dozen LDS cycles per sample of a chain
// that takes several hundred, and it saves the fp64 tile's second trip through LDS.  Interleaved, the two lanes
// of a stream write neighbouring elements of one range.
//
// The file is built with -ffp-contract=off; the only fused multiply-adds are the lattice's four, inside dLatticeSample.
#include "kernels.hpp"
#include "dither_device.hpp"
#include "pcm_device.hpp"
#include "quant_host.hpp"

namespace cpq {
namespace {

template <int FMT> struct QuantFmt;
template <> struct QuantFmt<CPQ_PCM_S16> { static constexpr int bps = 2; };
template <> struct QuantFmt<CPQ_PCM_S24> { static constexpr int bps = 3; };
template <> struct QuantFmt<CPQ_PCM_S32> { static constexpr int bps = 4; };

// the code of yq at the container's width, little-endian at `at` (aligned to the element; S24 on any byte)
template <int FMT>
__device__ __forceinline__ void qEncode(unsigned char* at, double yq)
{
    if constexpr (FMT == CPQ_PCM_S16) *reinterpret_cast<short*>(at) = (short)pcmQuantize<16>(yq);
    else if constexpr (FMT == CPQ_PCM_S32) *reinterpret_cast<int*>(at) = pcmQuantize<32>(yq);
    else {
        static_assert(FMT == CPQ_PCM_S24, "unknown container");
        const unsigned q = (unsigned)pcmQuantize<24>(yq);
        at[0] = (unsigned char)q;
        at[1] = (unsigned char)(q >> 8);
        at[2] = (unsigned char)(q >> 16);
    }
}

// a channel's shaper in registers.  kGroup: samples per unrolled group (the fixed shapers' shift register turns once in ORDER)
template <int ORDER>
struct QuantFixed {
    static constexpr int kGroup = ORDER;
    double e[ORDER];
    __device__ __forceinline__ void load(const double* err, const double* coef, int nCh, int ch, bool live)
    {
#pragma unroll
        for (int k = 0; k < ORDER; ++k) e[k] = live ? err[(size_t)k * nCh + ch] : 0.0;
    }
    __device__ __forceinline__ double step(double u, unsigned long long (&s)[4], const DitherParams& p) { return dSample<ORDER>(u, e, s, p); }
    __device__ __forceinline__ void save(double* err, int nCh, int ch) const
    {
#pragma unroll
        for (int k = 0; k < ORDER; ++k) err[(size_t)k * nCh + ch] = e[k];
    }
};

struct QuantLattice {
    static constexpr int kGroup = 1;
    double st[kLatticeOrder], c[kLatticeOrder];
    __device__ __forceinline__ void load(const double* err, const double* coef, int nCh, int ch, bool live)
    {
#pragma unroll
        for (int k = 0; k < kLatticeOrder; ++k) {
            st[k] = live ? err[(size_t)k * nCh + ch] : 0.0;
            c[k] = live ? coef[(size_t)k * nCh + ch] : 0.0;
        }
    }
    __device__ __forceinline__ double step(double u, unsigned long long (&s)[4], const DitherParams& p) { return dLatticeSample(u, st, c, s, p); }
    __device__ __forceinline__ void save(double* err, int nCh, int ch) const
    {
#pragma unroll
        for (int k = 0; k < kLatticeOrder; ++k) err[(size_t)k * nCh + ch] = st[k];
    }
};

// grid: ceil(nCh / kDitherRows) workgroups of one wave.  err [kDitherMaxOrder][nCh], rng [4][nCh], coef [kLatticeOrder][nCh],
// gain [nCh / 2].  pcm: planar, channel r's packed row at r * pitch; interleaved, stream s's at s * pitch (bytes)
template <class CHAIN, int FMT, int LAYOUT>
__device__ __forceinline__ void quantizeBody(const double* in, int64_t inStride, unsigned char* pcm, int64_t pitch, int n, int nCh, const DitherParams& p,
                                             const double* __restrict__ gain, const double* __restrict__ coef, double* __restrict__ err,
                                             unsigned long long* __restrict__ rng)
{
    constexpr int BPS = QuantFmt<FMT>::bps;
    constexpr int CH = LAYOUT == CPQ_PCM_INTERLEAVED ? 2 : 1;           // channels of a range
    constexpr int P = quantImagePitch(kDitherStep, BPS, CH);            // image bytes of a range
    constexpr int SLOTS = P / 16;
    static_assert(P % 16 == 0 && SLOTS % 2 == 1, "the ranges rotate through the bank row");
    static_assert(kDitherRows % 2 == 0, "a stream's two channels belong to one wave");
    __shared__ double tile[kDitherRows * kDitherPitch];
    __shared__ __attribute__((aligned(16))) unsigned char image[kDitherRows / CH * P];
    const int lane = threadIdx.x;
    const int row0 = blockIdx.x * kDitherRows;
    const int rows = min(kDitherRows, nCh - row0);                      // >= 2 and even: nCh is
    const int ranges = rows / CH;
    unsigned char* const out0 = pcm + (size_t)(row0 / CH) * (size_t)pitch;      // the wave's first range, sample 0
    CHAIN chain[kDitherCpl];
    unsigned long long s[kDitherCpl][4];
#pragma unroll
    for (int c = 0; c < kDitherCpl; ++c) {
        const int r = lane * kDitherCpl + c;
        const bool live = r < rows;
        chain[c].load(err, coef, nCh, row0 + (live ? r : 0), live);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[c][k] = live ? rng[(size_t)k * nCh + row0 + r] : 1ull;
    }
    for (int t0 = 0; t0 < n; t0 += kDitherStep) {
        const int len = min(kDitherStep, n - t0);
        dTileLoad<true>(tile, in, inStride, row0, rows, t0, len, lane, gain);
        __syncthreads();                                                // the tile is whole, and the last tile's image has left
        if (lane * kDitherCpl < rows) {
            const double* mine = tile + lane * kDitherCpl * kDitherPitch;
            unsigned char* at[kDitherCpl];                              // element 0 of channel c in its range's image
#pragma unroll
            for (int c = 0; c < kDitherCpl; ++c) {
                const int r = lane * kDitherCpl + c;
                const int g = r / CH;
                const int skew = (int)(reinterpret_cast<uintptr_t>(out0 + (size_t)g * (size_t)pitch + (size_t)t0 * (CH * BPS)) & 15);
                at[c] = image + g * P + skew + (r % CH) * BPS;
            }
            int t = 0;
            for (; t + CHAIN::kGroup <= len; t += CHAIN::kGroup) {
#pragma unroll
                for (int k = 0; k < CHAIN::kGroup; ++k) {
#pragma unroll
                    for (int c = 0; c < kDitherCpl; ++c)
                        qEncode<FMT>(at[c] + (t + k) * (CH * BPS), chain[c].step(mine[c * kDitherPitch + t + k], s[c], p));
                }
            }
            if constexpr (CHAIN::kGroup > 1) {
                for (; t < len; ++t) {
#pragma unroll
                    for (int c = 0; c < kDitherCpl; ++c) qEncode<FMT>(at[c] + t * (CH * BPS), chain[c].step(mine[c * kDitherPitch + t], s[c], p));
                }
            }
        }
        __syncthreads();                                                // the image is whole
        const int bytes = len * CH * BPS;
        for (int i = lane; i < ranges * SLOTS; i += 64) {
            const int g = i / SLOTS, k = i - g * SLOTS;
            unsigned char* dst = out0 + (size_t)g * (size_t)pitch + (size_t)t0 * (CH * BPS);       // byte 0 of the range
            const int skew = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
            const QuantSlot sl = quantSlot(skew, k, bytes);                                         // the slot's bytes of the range
            if (sl.hi - sl.lo == 16) {
                *reinterpret_cast<uint4*>(dst + sl.lo) = *reinterpret_cast<const uint4*>(image + 16 * i);
            } else {
                for (int b = sl.lo; b < sl.hi; ++b) dst[b] = image[g * P + skew + b];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kDitherCpl; ++c) {
        const int r = lane * kDitherCpl + c;
        if (r < rows) {
            chain[c].save(err, nCh, row0 + r);
#pragma unroll
            for (int k = 0; k < 4; ++k) rng[(size_t)k * nCh + row0 + r] = s[c][k];
        }
    }
}

template <int ORDER, int FMT, int LAYOUT>
__global__ void __launch_bounds__(64)
k_quantize(const double* in, int64_t inStride, unsigned char* pcm, int64_t pitch, int n, int nCh, DitherParams p, const double* __restrict__ gain,
           double* __restrict__ err, unsigned long long* __restrict__ rng)
{
    quantizeBody<QuantFixed<ORDER>, FMT, LAYOUT>(in, inStride, pcm, pitch, n, nCh, p, gain, nullptr, err, rng);
}

template <int FMT, int LAYOUT>
__global__ void __launch_bounds__(64)
k_quantize_lattice(const double* in, int64_t inStride, unsigned char* pcm, int64_t pitch, int n, int nCh, DitherParams p,
                   const double* __restrict__ gain, const double* __restrict__ coef, double* __restrict__ err, unsigned long long* __restrict__ rng)
{
    quantizeBody<QuantLattice, FMT, LAYOUT>(in, inStride, pcm, pitch, n, nCh, p, gain, coef, err, rng);
}

template <int FMT, int LAYOUT>
bool quantOrder(hipStream_t stream, const double* in, unsigned char* pcm, const QuantLaunch& a, const DitherParams& p, const double* gain,
                const double* coef, double* err, unsigned long long* rng)
{
    const dim3 grid((unsigned)((a.nCh + kDitherRows - 1) / kDitherRows)), block(64);
    if (a.order == 4)
        hipLaunchKernelGGL((k_quantize<4, FMT, LAYOUT>), grid, block, 0, stream, in, a.inStride, pcm, a.pitch, a.n, a.nCh, p, gain, err, rng);
    else if (a.order == 16)
        hipLaunchKernelGGL((k_quantize<16, FMT, LAYOUT>), grid, block, 0, stream, in, a.inStride, pcm, a.pitch, a.n, a.nCh, p, gain, err, rng);
    else if (a.order == kLatticeOrder && coef)
        hipLaunchKernelGGL((k_quantize_lattice<FMT, LAYOUT>), grid, block, 0, stream, in, a.inStride, pcm, a.pitch, a.n, a.nCh, p, gain, coef, err, rng);
    else return false;
    return true;
}

template <int FMT>
bool quantLayout(hipStream_t stream, const double* in, unsigned char* pcm, const QuantLaunch& a, const DitherParams& p, const double* gain,
                 const double* coef, double* err, unsigned long long* rng)
{
    if (a.layout == CPQ_PCM_INTERLEAVED) return quantOrder<FMT, CPQ_PCM_INTERLEAVED>(stream, in, pcm, a, p, gain, coef, err, rng);
    if (a.layout == CPQ_PCM_PLANAR) return quantOrder<FMT, CPQ_PCM_PLANAR>(stream, in, pcm, a, p, gain, coef, err, rng);
    return false;
}

}  // namespace

bool launch_quantize(hipStream_t stream, const double* in, void* pcm, const QuantLaunch& a, const DitherParams& p, const double* gain,
                     const double* coef, double* err, unsigned long long* rng)
{
    unsigned char* out = static_cast<unsigned char*>(pcm);
    switch (a.format) {
    case CPQ_PCM_S16: return quantLayout<CPQ_PCM_S16>(stream, in, out, a, p, gain, coef, err, rng);
    case CPQ_PCM_S24: return quantLayout<CPQ_PCM_S24>(stream, in, out, a, p, gain, coef, err, rng);
    case CPQ_PCM_S32: return quantLayout<CPQ_PCM_S32>(stream, in, out, a, p, gain, coef, err, rng);
    default: return false;
    }
}

}  // namespace cpq
