// pcm_layout.hpp -- the layout arithmetic of the packed PCM entry points (engine_pcm.cpp, pcm_kernels.hip): bytes per sample,
// pitches and widths of a call and of its time chunks, the byte ranges a call touches, the overlap test.  The only place that
// knows them.  HIP-free, 64-bit throughout: a host program can include this header alone (tests/sanitize/pcm_layout_check.cpp).
//
//   planar       [2 S][n]     one row per channel, the engine's own row order
//   interleaved  [S][n][2]    stereo frames per stream, as in a file
// A copy of the packed side moves `rows` lines of `width` bytes: 2 S lines of len * bps (planar), S lines of len * 2 * bps
// (interleaved); the pitch of a buffer is the width of its whole length.
#pragma once

#include "convopeq_mi355x.h"

#include <cstdint>

namespace cpq {
namespace pcm {

constexpr int bytesPerSample(int format)
{
    return format == CPQ_PCM_F64 ? 8 : format == CPQ_PCM_F32 ? 4 : format == CPQ_PCM_S16 ? 2 : format == CPQ_PCM_S24 ? 3
         : format == CPQ_PCM_S32 ? 4 : -1;
}
// the alignment a packed buffer needs: that of its element (packed 24-bit samples start on any byte)
constexpr int alignmentOf(int format) { return format == CPQ_PCM_S24 ? 1 : bytesPerSample(format); }
constexpr bool validLayout(int layout) { return layout == CPQ_PCM_PLANAR || layout == CPQ_PCM_INTERLEAVED; }

constexpr int64_t samplesPerFrame(int layout) { return layout == CPQ_PCM_INTERLEAVED ? 2 : 1; }
constexpr int64_t rowsOf(int layout, int streams) { return layout == CPQ_PCM_INTERLEAVED ? (int64_t)streams : 2 * (int64_t)streams; }
// bytes of `len` samples per channel in one line of the packed side
constexpr int64_t widthBytes(int format, int layout, int64_t len) { return len * samplesPerFrame(layout) * bytesPerSample(format); }
constexpr int64_t pitchBytes(int format, int layout, int64_t n) { return widthBytes(format, layout, n); }
constexpr int64_t totalBytes(int format, int layout, int streams, int64_t n) { return rowsOf(layout, streams) * pitchBytes(format, layout, n); }

struct ByteRange { uint64_t begin, end; };      // [begin, end)

inline ByteRange callRange(const void* p, int format, int layout, int streams, int64_t n)
{
    const uint64_t b = (uint64_t)reinterpret_cast<uintptr_t>(p);
    return ByteRange{ b, b + (uint64_t)totalBytes(format, layout, streams, n) };
}
// ranges that only touch do not overlap; an empty range overlaps nothing
constexpr bool overlaps(ByteRange a, ByteRange b) { return a.begin < b.end && b.begin < a.end && a.begin < a.end && b.begin < b.end; }

// in and out of one call: the same buffer when format (and the call's one layout) agree, otherwise disjoint
inline bool buffersAllowed(const void* in, int inFormat, const void* out, int outFormat, int layout, int streams, int64_t n)
{
    if (in == out) return inFormat == outFormat;
    return !overlaps(callRange(in, inFormat, layout, streams, n), callRange(out, outFormat, layout, streams, n));
}

// Time chunk `index` of `chunkLen` samples per channel out of a call of n: one 2-D copy between the caller's buffer (pitch of
// n) and a device buffer that holds the chunks one after the other, each with the pitch of its own length.
struct ChunkCopy { int64_t hostOffset, hostPitch, devOffset, devPitch, width, rows; };

constexpr ChunkCopy chunkCopy(int format, int layout, int streams, int64_t n, int64_t chunkLen, int index)
{
    const int64_t w = widthBytes(format, layout, chunkLen);
    return ChunkCopy{ index * w, pitchBytes(format, layout, n), index * rowsOf(layout, streams) * w, w, w, rowsOf(layout, streams) };
}

}  // namespace pcm
}  // namespace cpq
