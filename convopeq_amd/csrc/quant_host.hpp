// quant_host.hpp -- cpq_quantizer without HIP: the definition of a call (gain, shaper, pack), the byte layout of its packed side,
// the refusals of a call in their documented order, and QuantHost, the object that computes on the host.  A host program can
// include this header and link dither_design.cpp alone (tests/sanitize/quant_host_check.cpp).
//
//   u  = x * gain[s]                          one rounding, nothing scrubbed
//   yq = DitherHost::process(u, headroom 1.0) the shaper's processSample, a DitherHost per stream
//   b  = rint(yq * 2^(w - 1)), ties to even, saturated to [-2^(w-1), 2^(w-1) - 1], NaN -> 0; w = the container's width
// b leaves as w / 8 little-endian bytes: planar, sample i of channel c at c * pitch + i * bps; interleaved, sample i of channel
// ch of stream s at s * pitch + (2 i + ch) * bps.  The layout arithmetic is pcm_layout.hpp's, with the caller's pitch in place
// of the width.
#pragma once

#include "host_design.hpp"
#include "pcm_layout.hpp"

#include <cmath>
#include <cstdint>
#include <vector>

namespace cpq {

constexpr int kQuantMaxCall = 1 << 30;
constexpr int kQuantChunk = 4096;       // samples QuantHost runs through a shaper at a time

constexpr bool quantContainer(int format) { return format == CPQ_PCM_S16 || format == CPQ_PCM_S24 || format == CPQ_PCM_S32; }
constexpr int quantWidth(int format) { return 8 * pcm::bytesPerSample(format); }

// "out, S24/S32" at `width` bits
inline int32_t quantCode(double yq, int width)
{
    const double k = std::ldexp(1.0, width - 1);
    double v = std::nearbyint(yq * k);          // round to nearest even: the default rounding mode
    if (v != v) v = 0.0;
    v = (-k < v) ? v : -k;
    v = (v < k - 1.0) ? v : k - 1.0;
    return (int32_t)v;
}

inline void quantStore(unsigned char* at, int32_t code, int bps)
{
    for (int b = 0; b < bps; ++b) at[b] = (unsigned char)((uint32_t)code >> (8 * b));
}

// byte offset of sample i of channel ch (0, 1) of stream s
constexpr int64_t quantOffset(int format, int layout, int64_t pitch, int64_t s, int ch, int64_t i)
{
    return layout == CPQ_PCM_INTERLEAVED ? s * pitch + (2 * i + ch) * pcm::bytesPerSample(format)
                                         : (2 * s + ch) * pitch + i * pcm::bytesPerSample(format);
}
// bytes from the first byte a call writes to the one after the last: the gap after the last row is not part of it
constexpr int64_t quantPcmBytes(int format, int layout, int streams, int64_t pitch, int64_t n)
{
    return (pcm::rowsOf(layout, streams) - 1) * pitch + pcm::widthBytes(format, layout, n);
}
constexpr int64_t quantInBytes(int streams, int64_t stride, int64_t n) { return ((2 * (int64_t)streams - 1) * stride + n) * 8; }

// The byte image of the device kernel (quant_kernels.hip): a tile's range of `bytes` bytes whose first byte has the global
// address A lives at image[skew + b], skew = A & 15, in an image of quantImagePitch bytes that starts on 16 bytes.  Slot k is
// image[16 k, 16 k + 16); quantSlot gives the bytes [lo, hi) of the range that lie in it: hi - lo == 16 is a whole slot, which
// leaves as one aligned 16-byte store to A + lo; a shorter one moves byte by byte; hi <= lo is a slot outside the range.
constexpr int quantImagePitch(int tileSamples, int bps, int channels) { return tileSamples * bps * channels + 16; }
struct QuantSlot { int lo, hi; };
constexpr QuantSlot quantSlot(int skew, int k, int bytes)
{
    const int first = 16 * k - skew;
    return QuantSlot{ first > 0 ? first : 0, first + 16 < bytes ? first + 16 : bytes };
}

// The refusals of a call on rows in and bytes out, in the header's order; null where the call may run.  deviceRows: d_in on
// 16 bytes
inline const char* quantCallFault(const void* in, int64_t inStride, const void* pcmOut, int64_t pitch, int format, int layout, int streams,
                                  int64_t n, bool deviceRows)
{
    if (!in || !pcmOut) return "null buffer";
    if (n < 1 || n > kQuantMaxCall) return "n_samples outside 1..2^30";
    if (!pcm::validLayout(layout)) return "unknown layout";
    if (inStride < n) return "in_stride below n_samples";
    if (pitch < pcm::widthBytes(format, layout, n)) return "pcm_pitch_bytes below the width of a packed row";
    const uint64_t a = (uint64_t)reinterpret_cast<uintptr_t>(in), b = (uint64_t)reinterpret_cast<uintptr_t>(pcmOut);
    if (a & (deviceRows ? 15u : 7u)) return deviceRows ? "d_in must be 16-byte aligned" : "in must be 8-byte aligned";
    const uint64_t el = (uint64_t)pcm::alignmentOf(format);
    if (b % el || (uint64_t)pitch % el) return "the packed buffer and its pitch must be aligned to the element";
    if (pcm::overlaps(pcm::ByteRange{ a, a + (uint64_t)quantInBytes(streams, inStride, n) },
                      pcm::ByteRange{ b, b + (uint64_t)quantPcmBytes(format, layout, streams, pitch, n) }))
        return "the rows and the packed buffer overlap";
    return nullptr;
}

struct QuantHost {
    int streams = 0, shaper = CPQ_DITHER_OFF, bits = 0, format = CPQ_PCM_S16;
    double rate = 0.0;
    std::vector<DitherHost> d;          // one per stream: all streams draw the same two sequences (L, R)
    std::vector<double> gains;
    std::vector<double> l, r;           // a chunk of u, then of yq
    int64_t pos = 0;                    // samples taken since create / reset

    // arguments checked by the caller (cpq_quantizer_create)
    bool init(int nStreams, double sampleRate, int shaperId, int bitDepth, int containerFormat)
    {
        streams = nStreams; rate = sampleRate; shaper = shaperId; bits = bitDepth; format = containerFormat;
        d.assign((size_t)nStreams, DitherHost());
        for (DitherHost& h : d)
            if (!h.configure(sampleRate, shaperId, bitDepth)) return false;
        gains.assign((size_t)nStreams, 1.0);
        l.assign(kQuantChunk, 0.0);
        r.assign(kQuantChunk, 0.0);
        pos = 0;
        return true;
    }
    // as new: errors cleared, generators reseeded; gains and coefficients stay
    void reset()
    {
        for (DitherHost& h : d) {
            h.reset();
            for (int ch = 0; ch < 2; ++ch) ditherSeed(shaper, rate, bits, ch, h.rng[ch]);
        }
        pos = 0;
    }
    // applyMatchedCoefficients of streams [s0, s1): clamped, their states cleared.  Arguments checked by the caller
    void setAdaptive(int s0, int s1, const double* k, int n)
    {
        for (int s = s0; s < s1; ++s) d[(size_t)s].setAdaptiveCoeffs(k, n);
    }
    // a checked call (quantCallFault) on host rows
    void process(const double* in, int64_t inStride, int n, unsigned char* out, int64_t pitch, int layout)
    {
        const int bps = pcm::bytesPerSample(format), width = quantWidth(format);
        for (int s = 0; s < streams; ++s) {
            const double g = gains[(size_t)s];
            const double* rows[2] = { in + (2 * (int64_t)s) * inStride, in + (2 * (int64_t)s + 1) * inStride };
            double* u[2] = { l.data(), r.data() };
            for (int t0 = 0; t0 < n; t0 += kQuantChunk) {
                const int len = n - t0 < kQuantChunk ? n - t0 : kQuantChunk;
                for (int ch = 0; ch < 2; ++ch)
                    for (int i = 0; i < len; ++i) u[ch][i] = rows[ch][t0 + i] * g;
                d[(size_t)s].process(u[0], u[1], len, 1.0);
                for (int ch = 0; ch < 2; ++ch)
                    for (int i = 0; i < len; ++i)
                        quantStore(out + quantOffset(format, layout, pitch, s, ch, (int64_t)t0 + i), quantCode(u[ch][i], width), bps);
            }
        }
        pos += n;
    }
};

}  // namespace cpq
