// Host program over convopeq_amd/csrc/pcm_layout.hpp alone (no HIP, not the library), built with the address and
// undefined-behaviour sanitizers by tests/test_pcm_layout_cpu.py.  Every check is exact.
#include "pcm_layout.hpp"

#include <cstdio>
#include <vector>

namespace pcm = cpq::pcm;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

int main()
{
    const int formats[5] = { CPQ_PCM_F64, CPQ_PCM_F32, CPQ_PCM_S16, CPQ_PCM_S24, CPQ_PCM_S32 };
    const int64_t bps[5] = { 8, 4, 2, 3, 4 };
    for (int f = 0; f < 5; ++f) CHECK(pcm::bytesPerSample(formats[f]) == bps[f]);
    CHECK(pcm::bytesPerSample(-1) == -1 && pcm::bytesPerSample(5) == -1 && pcm::bytesPerSample(1 << 30) == -1);
    CHECK(pcm::alignmentOf(CPQ_PCM_S24) == 1 && pcm::alignmentOf(CPQ_PCM_F32) == 4 && pcm::alignmentOf(CPQ_PCM_S16) == 2 && pcm::alignmentOf(CPQ_PCM_F64) == 8);
    CHECK(pcm::validLayout(CPQ_PCM_PLANAR) && pcm::validLayout(CPQ_PCM_INTERLEAVED) && !pcm::validLayout(2) && !pcm::validLayout(-1));

    // pitches and widths of every format x layout
    const int64_t ns[3] = { 1, 3, 4097 };
    const int S = 3;
    for (int f = 0; f < 5; ++f)
        for (int64_t n : ns) {
            CHECK(pcm::pitchBytes(formats[f], CPQ_PCM_PLANAR, n) == n * bps[f]);
            CHECK(pcm::pitchBytes(formats[f], CPQ_PCM_INTERLEAVED, n) == n * 2 * bps[f]);
            CHECK(pcm::widthBytes(formats[f], CPQ_PCM_PLANAR, n) == n * bps[f]);
            CHECK(pcm::widthBytes(formats[f], CPQ_PCM_INTERLEAVED, n) == n * 2 * bps[f]);
            CHECK(pcm::rowsOf(CPQ_PCM_PLANAR, S) == 2 * S && pcm::rowsOf(CPQ_PCM_INTERLEAVED, S) == S);
            CHECK(pcm::totalBytes(formats[f], CPQ_PCM_PLANAR, S, n) == 2 * S * n * bps[f]);
            CHECK(pcm::totalBytes(formats[f], CPQ_PCM_INTERLEAVED, S, n) == 2 * S * n * bps[f]);
        }

    // the four time chunks of a call tile the caller's buffer and the device buffer: every byte once
    for (int f = 0; f < 5; ++f)
        for (int layout = 0; layout < 2; ++layout)
            for (int64_t chunkLen : { (int64_t)1, (int64_t)3, (int64_t)512 }) {
                const int64_t n = 4 * chunkLen;
                const int64_t total = pcm::totalBytes(formats[f], layout, S, n);
                std::vector<unsigned char> host((size_t)total, 0), dev((size_t)total, 0);
                for (int i = 0; i < 4; ++i) {
                    const pcm::ChunkCopy c = pcm::chunkCopy(formats[f], layout, S, n, chunkLen, i);
                    CHECK(c.hostPitch == pcm::pitchBytes(formats[f], layout, n) && c.width == pcm::widthBytes(formats[f], layout, chunkLen));
                    CHECK(c.devPitch == c.width && c.rows == pcm::rowsOf(layout, S));
                    CHECK(c.devOffset % bps[f] == 0 && c.hostOffset % bps[f] == 0);
                    for (int64_t r = 0; r < c.rows; ++r)
                        for (int64_t b = 0; b < c.width; ++b) {
                            host[(size_t)(c.hostOffset + r * c.hostPitch + b)]++;      // out of range: the address sanitizer stops here
                            dev[(size_t)(c.devOffset + r * c.devPitch + b)]++;
                        }
                }
                bool once = true;
                for (int64_t b = 0; b < total; ++b) once = once && host[(size_t)b] == 1 && dev[(size_t)b] == 1;
                CHECK(once);
            }
    {   // one chunk of the whole call is the call
        const pcm::ChunkCopy c = pcm::chunkCopy(CPQ_PCM_S24, CPQ_PCM_INTERLEAVED, S, 4097, 4097, 0);
        CHECK(c.hostOffset == 0 && c.devOffset == 0 && c.width == c.hostPitch && c.rows * c.width == pcm::totalBytes(CPQ_PCM_S24, CPQ_PCM_INTERLEAVED, S, 4097));
    }

    // the overlap test
    using R = pcm::ByteRange;
    CHECK(!pcm::overlaps(R{ 100, 200 }, R{ 200, 300 }) && !pcm::overlaps(R{ 200, 300 }, R{ 100, 200 }));        // touching
    CHECK(pcm::overlaps(R{ 100, 200 }, R{ 199, 300 }) && pcm::overlaps(R{ 199, 300 }, R{ 100, 200 }));
    CHECK(pcm::overlaps(R{ 100, 400 }, R{ 200, 300 }) && pcm::overlaps(R{ 200, 300 }, R{ 100, 400 }));          // nested
    CHECK(pcm::overlaps(R{ 100, 200 }, R{ 100, 200 }));                                                         // equal
    CHECK(!pcm::overlaps(R{ 100, 100 }, R{ 50, 150 }) && !pcm::overlaps(R{ 50, 150 }, R{ 100, 100 }));          // empty
    {
        alignas(16) static unsigned char buf[4096];
        const int n = 64;       // one stream: F32 = 512 bytes, S32 = 512, S24 = 384, F64 = 1024
        CHECK(pcm::buffersAllowed(buf, CPQ_PCM_F32, buf, CPQ_PCM_F32, CPQ_PCM_PLANAR, 1, n));                   // in place, same format
        CHECK(!pcm::buffersAllowed(buf, CPQ_PCM_F32, buf, CPQ_PCM_S32, CPQ_PCM_PLANAR, 1, n));                  // same pointer, other format
        CHECK(!pcm::buffersAllowed(buf, CPQ_PCM_F32, buf, CPQ_PCM_F64, CPQ_PCM_INTERLEAVED, 1, n));
        CHECK(pcm::buffersAllowed(buf, CPQ_PCM_F32, buf + 512, CPQ_PCM_F32, CPQ_PCM_PLANAR, 1, n));             // touching
        CHECK(!pcm::buffersAllowed(buf, CPQ_PCM_F32, buf + 496, CPQ_PCM_F32, CPQ_PCM_PLANAR, 1, n));            // 16 bytes shared
        CHECK(!pcm::buffersAllowed(buf + 496, CPQ_PCM_F32, buf, CPQ_PCM_F32, CPQ_PCM_PLANAR, 1, n));
        CHECK(pcm::buffersAllowed(buf, CPQ_PCM_S24, buf + 384, CPQ_PCM_F64, CPQ_PCM_INTERLEAVED, 1, n));
        CHECK(!pcm::buffersAllowed(buf + 16, CPQ_PCM_S24, buf, CPQ_PCM_F64, CPQ_PCM_INTERLEAVED, 1, n));        // nested
        const R r = pcm::callRange(buf, CPQ_PCM_S24, CPQ_PCM_INTERLEAVED, 1, n);
        CHECK(r.end - r.begin == 384);
    }

    // no 32-bit overflow at the largest shape: 1024 streams x 524288 samples
    {
        const int bigS = 1024;
        const int64_t bigN = 524288;
        CHECK(pcm::totalBytes(CPQ_PCM_F64, CPQ_PCM_PLANAR, bigS, bigN) == 8589934592ll);
        CHECK(pcm::totalBytes(CPQ_PCM_S24, CPQ_PCM_INTERLEAVED, bigS, bigN) == 3221225472ll);
        CHECK(pcm::totalBytes(CPQ_PCM_F32, CPQ_PCM_INTERLEAVED, bigS, bigN) == 4294967296ll);
        const pcm::ChunkCopy c = pcm::chunkCopy(CPQ_PCM_F64, CPQ_PCM_PLANAR, bigS, bigN, bigN / 4, 3);
        CHECK(c.devOffset == 3ll * 2048 * 131072 * 8 && c.hostOffset == 3ll * 131072 * 8 && c.hostPitch == 4194304 && c.width == 1048576);
        CHECK(c.devOffset + c.rows * c.devPitch == 8589934592ll);
        CHECK(c.hostOffset + (c.rows - 1) * c.hostPitch + c.width == 8589934592ll);
        const R a = pcm::callRange(reinterpret_cast<const void*>((uintptr_t)0x100000000ull), CPQ_PCM_F64, CPQ_PCM_PLANAR, bigS, bigN);
        CHECK(a.end - a.begin == 8589934592ull);
        CHECK(pcm::buffersAllowed(reinterpret_cast<const void*>((uintptr_t)0x100000000ull), CPQ_PCM_F64,
                                  reinterpret_cast<const void*>((uintptr_t)0x300000000ull), CPQ_PCM_F32, CPQ_PCM_PLANAR, bigS, bigN));
        CHECK(!pcm::buffersAllowed(reinterpret_cast<const void*>((uintptr_t)0x100000000ull), CPQ_PCM_F64,
                                   reinterpret_cast<const void*>((uintptr_t)0x2fffffff0ull), CPQ_PCM_F32, CPQ_PCM_PLANAR, bigS, bigN));
    }

    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
