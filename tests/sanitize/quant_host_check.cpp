// quant_host_check.cpp -- csrc/quant_host.hpp as a program of its own, for the address and undefined-behaviour sanitizers: the host
// object of cpq_quantizer (cpq::QuantHost, linked with csrc/dither_design.cpp) on heap blocks of exactly the sizes a caller
// passes -- rows [2 S][stride], bytes from the first one written to the last -- at every container, both layouts, packed rows that
// start on any byte phase, pitch gaps and n = 1.  An index outside them is a sanitizer report.  Three things are held to the
// object's bytes:
//   the definition restated sample by sample: a DitherHost per stream on x * gain, quantCode, quantOffset
//   the same programme split into calls
//   the store pass of k_quantize (csrc/quant_kernels.hip) as host loops: per wave and tile the chain's element writes into an
//   image block of exactly ranges * quantImagePitch bytes, then slot after slot through quantSlot, whole slots as 16-byte
//   copies whose two addresses must be 16-byte aligned, the rest byte by byte
// and the gaps between the rows must come out as they went in.  Then quantCallFault's refusals in their documented order.
// Built and run by tests/test_quant_plan_cpu.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "quant_host.hpp"

static int g_failed = 0;
static long long g_cases = 0, g_bytes = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++g_failed;                                   \
            std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

using namespace cpq;

constexpr int kTile = CPQ_DITHER_TILE, kWaveRows = 64;
constexpr unsigned char kGuard = 0xA5;

struct Case {
    int shaper, bits, format, layout, streams, n, gap, phase;
    int64_t stride;
};

// the packed buffer of a case, ending at the end of its allocation, its first byte at address = phase (mod 16)
struct Packed {
    std::unique_ptr<unsigned char[]> raw;
    unsigned char* p = nullptr;
    size_t bytes = 0;
    Packed(size_t n, int phase) : bytes(n)
    {
        // 16 spare bytes in front let the first byte land on the wanted phase; the end is the allocation's end
        for (int extra = 0; extra < 16; ++extra) {
            raw.reset(new unsigned char[n + (size_t)extra]);
            p = raw.get() + extra;
            if ((int)(reinterpret_cast<uintptr_t>(p) & 15) == phase) break;
        }
        std::memset(raw.get(), kGuard, (size_t)(p - raw.get()) + n);
    }
};

static std::vector<double> makeRows(const Case& c, unsigned seed)
{
    std::mt19937_64 gen(seed);
    std::uniform_real_distribution<double> u(-1.2, 1.2);
    std::vector<double> x((size_t)(2 * c.streams - 1) * (size_t)c.stride + (size_t)c.n);     // exactly what a call may read
    for (double& v : x) v = u(gen);
    if (c.n > 3) {
        x[1] = std::numeric_limits<double>::quiet_NaN();
        x[2] = std::numeric_limits<double>::infinity();
        x[(size_t)c.stride + 3 < x.size() ? (size_t)c.stride + 3 : 3] = -std::numeric_limits<double>::infinity();
    }
    return x;
}

static void setUp(QuantHost& q, const Case& c)
{
    CHECK(q.init(c.streams, 48000.0, c.shaper, c.bits, c.format), "init");
    for (int s = 0; s < c.streams; ++s) q.gains[(size_t)s] = 0.5 + 0.25 * (s % 5);
}

static bool gapsIntact(const Case& c, const Packed& out, int64_t pitch)
{
    const int64_t width = pcm::widthBytes(c.format, c.layout, c.n), rows = pcm::rowsOf(c.layout, c.streams);
    for (unsigned char* b = out.raw.get(); b < out.p; ++b)
        if (*b != kGuard) return false;
    for (int64_t r = 0; r + 1 < rows; ++r)
        for (int64_t b = width; b < pitch; ++b)
            if (out.p[r * pitch + b] != kGuard) return false;
    return true;
}

// the definition, sample by sample
static void byDefinition(const Case& c, const std::vector<double>& x, unsigned char* out, int64_t pitch)
{
    QuantHost q;
    setUp(q, c);
    const int bps = pcm::bytesPerSample(c.format);
    for (int s = 0; s < c.streams; ++s) {
        std::vector<double> l((size_t)c.n), r((size_t)c.n);
        for (int i = 0; i < c.n; ++i) {
            l[(size_t)i] = x[(size_t)(2 * s) * (size_t)c.stride + (size_t)i] * q.gains[(size_t)s];
            r[(size_t)i] = x[(size_t)(2 * s + 1) * (size_t)c.stride + (size_t)i] * q.gains[(size_t)s];
        }
        q.d[(size_t)s].process(l.data(), r.data(), c.n, 1.0);
        for (int i = 0; i < c.n; ++i) {
            quantStore(out + quantOffset(c.format, c.layout, pitch, s, 0, i), quantCode(l[(size_t)i], quantWidth(c.format)), bps);
            quantStore(out + quantOffset(c.format, c.layout, pitch, s, 1, i), quantCode(r[(size_t)i], quantWidth(c.format)), bps);
        }
    }
}

// k_quantize's image and store pass over yq rows [2 S][n] (the shaper's outputs, computed by the caller)
static void kernelStorePass(const Case& c, const std::vector<double>& yq, unsigned char* pcmOut, int64_t pitch)
{
    const int bps = pcm::bytesPerSample(c.format), CH = c.layout == CPQ_PCM_INTERLEAVED ? 2 : 1;
    const int P = quantImagePitch(kTile, bps, CH), SLOTS = P / 16, nCh = 2 * c.streams;
    CHECK(P % 16 == 0 && SLOTS % 2 == 1, "P=%d", P);
    for (int row0 = 0; row0 < nCh; row0 += kWaveRows) {
        const int rows = nCh - row0 < kWaveRows ? nCh - row0 : kWaveRows, ranges = rows / CH;
        unsigned char* out0 = pcmOut + (int64_t)(row0 / CH) * pitch;
        for (int t0 = 0; t0 < c.n; t0 += kTile) {
            const int len = c.n - t0 < kTile ? c.n - t0 : kTile, bytes = len * CH * bps;
            // aligned to 16 bytes as the kernel's image is: over-allocate in front, end exactly at the image's end
            std::unique_ptr<unsigned char[]> raw(new unsigned char[(size_t)ranges * (size_t)P + 15]);
            const size_t lead = (16 - (reinterpret_cast<uintptr_t>(raw.get()) & 15)) & 15;
            unsigned char* image = raw.get() + lead;
            const size_t imageBytes = (size_t)ranges * (size_t)P;
            std::vector<char> written(imageBytes, 0);
            for (int r = 0; r < rows; ++r) {                    // the chain: lane r / kDitherCpl, element writes
                const int g = r / CH;
                unsigned char* dst = out0 + (int64_t)g * pitch + (int64_t)t0 * (CH * bps);
                const int skew = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
                for (int t = 0; t < len; ++t) {
                    const size_t at = (size_t)g * (size_t)P + (size_t)skew + (size_t)((t * CH + r % CH) * bps);
                    CHECK(at + (size_t)bps <= imageBytes, "image write at %zu of %zu", at, imageBytes);
                    CHECK(bps == 3 || at % (size_t)bps == 0, "element at %zu not aligned to %d", at, bps);
                    quantStore(image + at, quantCode(yq[(size_t)(row0 + r) * (size_t)c.n + (size_t)(t0 + t)], quantWidth(c.format)), bps);
                    for (int b = 0; b < bps; ++b) written[at + (size_t)b] = 1;
                }
            }
            int singles = 0, lastRange = -1;
            for (int i = 0; i < ranges * SLOTS; ++i) {          // the store pass: lane i % 64
                const int g = i / SLOTS, k = i - g * SLOTS;
                if (g != lastRange) { singles = 0; lastRange = g; }
                unsigned char* dst = out0 + (int64_t)g * pitch + (int64_t)t0 * (CH * bps);
                const int skew = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
                const QuantSlot sl = quantSlot(skew, k, bytes);
                if (sl.hi - sl.lo == 16) {
                    CHECK((reinterpret_cast<uintptr_t>(dst + sl.lo) & 15) == 0 && (reinterpret_cast<uintptr_t>(image + 16 * (size_t)i) & 15) == 0, "slot %d", i);
                    CHECK(16 * (size_t)i == (size_t)g * (size_t)P + (size_t)skew + (size_t)sl.lo, "slot %d is not its range's bytes from %d", i, sl.lo);
                    for (int b = 0; b < 16; ++b) CHECK(written[16 * (size_t)i + (size_t)b], "slot %d byte %d never written", i, b);
                    std::memcpy(dst + sl.lo, image + 16 * (size_t)i, 16);
                } else {
                    for (int b = sl.lo; b < sl.hi; ++b) {
                        const size_t at = (size_t)g * (size_t)P + (size_t)skew + (size_t)b;
                        CHECK(written[at], "byte %zu never written", at);
                        dst[b] = image[at];
                        ++singles;
                    }
                }
                CHECK(singles <= 30, "%d single bytes in range %d", singles, g);
            }
        }
    }
}

static void runCase(const Case& c)
{
    ++g_cases;
    const int64_t width = pcm::widthBytes(c.format, c.layout, c.n), pitch = width + c.gap;
    const size_t bytes = (size_t)quantPcmBytes(c.format, c.layout, c.streams, pitch, c.n);
    const std::vector<double> x = makeRows(c, 17u * (unsigned)c.n + (unsigned)c.format);
    auto tag = [&] {
        std::printf("  [shaper %d bits %d format %d layout %d S %d n %d gap %d phase %d]\n", c.shaper, c.bits, c.format, c.layout, c.streams, c.n, c.gap, c.phase);
    };
    const int before = g_failed;

    Packed one(bytes, c.phase);
    CHECK((int)(reinterpret_cast<uintptr_t>(one.p) & 15) == c.phase, "phase");
    CHECK(quantCallFault(x.data(), c.stride, one.p, pitch, c.format, c.layout, c.streams, c.n, false) == nullptr, "%s",
          quantCallFault(x.data(), c.stride, one.p, pitch, c.format, c.layout, c.streams, c.n, false));
    QuantHost q;
    setUp(q, c);
    q.process(x.data(), c.stride, c.n, one.p, pitch, c.layout);
    CHECK(gapsIntact(c, one, pitch), "a gap byte changed");
    CHECK(q.pos == c.n, "pos");
    g_bytes += (long long)bytes;

    Packed def(bytes, c.phase);
    byDefinition(c, x, def.p, pitch);
    CHECK(std::memcmp(one.p, def.p, bytes) == 0, "the object differs from the definition");

    // the programme in pieces: each piece its own exactly sized buffers
    {
        QuantHost s;
        setUp(s, c);
        const int cuts[] = { 1, 63, 64, 65, 7 };
        int at = 0, k = 0;
        bool same = true;
        while (at < c.n) {
            int len = cuts[k++ % 5];
            if (len > c.n - at) len = c.n - at;
            Case pc = c;
            pc.n = len;
            const int64_t pw = pcm::widthBytes(c.format, c.layout, len), pp = pw + c.gap;
            Packed piece((size_t)quantPcmBytes(c.format, c.layout, c.streams, pp, len), c.phase);
            std::vector<double> rows((size_t)(2 * c.streams - 1) * (size_t)len + (size_t)len);
            for (int r = 0; r < 2 * c.streams; ++r)
                for (int i = 0; i < len; ++i) rows[(size_t)r * (size_t)len + (size_t)i] = x[(size_t)r * (size_t)c.stride + (size_t)(at + i)];
            s.process(rows.data(), len, len, piece.p, pp, c.layout);
            CHECK(gapsIntact(pc, piece, pp), "a gap byte of a piece changed");
            const int bps = pcm::bytesPerSample(c.format);
            for (int st = 0; st < c.streams && same; ++st)
                for (int ch = 0; ch < 2 && same; ++ch)
                    for (int i = 0; i < len && same; ++i)
                        same = std::memcmp(piece.p + quantOffset(c.format, c.layout, pp, st, ch, i),
                                           one.p + quantOffset(c.format, c.layout, pitch, st, ch, at + i), (size_t)bps) == 0;
            at += len;
        }
        CHECK(same, "a split of the programme changed its bytes");
    }

    // the kernel's store pass on the shaper's rows
    {
        QuantHost s;
        setUp(s, c);
        std::vector<double> yq((size_t)(2 * c.streams) * (size_t)c.n);
        for (int st = 0; st < c.streams; ++st) {
            double* l = yq.data() + (size_t)(2 * st) * (size_t)c.n;
            double* r = l + c.n;
            for (int i = 0; i < c.n; ++i) {
                l[i] = x[(size_t)(2 * st) * (size_t)c.stride + (size_t)i] * s.gains[(size_t)st];
                r[i] = x[(size_t)(2 * st + 1) * (size_t)c.stride + (size_t)i] * s.gains[(size_t)st];
            }
            s.d[(size_t)st].process(l, r, c.n, 1.0);
        }
        Packed dev(bytes, c.phase);
        kernelStorePass(c, yq, dev.p, pitch);
        CHECK(gapsIntact(c, dev, pitch), "the store pass changed a gap byte");
        CHECK(std::memcmp(one.p, dev.p, bytes) == 0, "the store pass differs from the object");
    }
    if (g_failed != before) tag();
}

static void refusals()
{
    std::vector<double> x(4 * 40);
    std::vector<unsigned char> out(4 * 200);
    const double* in = x.data();
    unsigned char* o = out.data();
    auto is = [](const char* got, const char* word) { return got && std::strstr(got, word); };
    const int F = CPQ_PCM_S16, L = CPQ_PCM_PLANAR;
    // each call is wrong in its own rule and in every later one: the earlier rule answers
    CHECK(is(quantCallFault(nullptr, 0, o + 1, 0, F, 7, 2, 0, true), "null"), "null in");
    CHECK(is(quantCallFault(in, 0, nullptr, 0, F, 7, 2, 0, true), "null"), "null out");
    CHECK(is(quantCallFault(in, 0, o + 1, 0, F, 7, 2, 0, true), "n_samples"), "n 0");
    CHECK(is(quantCallFault(in, 0, o + 1, 0, F, 7, 2, ((int64_t)1 << 30) + 1, true), "n_samples"), "n 2^30 + 1");
    CHECK(is(quantCallFault(in, 0, o + 1, 0, F, 7, 2, 32, true), "layout"), "layout");
    CHECK(is(quantCallFault(in, 31, o + 1, 0, F, L, 2, 32, true), "in_stride"), "stride");
    CHECK(is(quantCallFault(in + 1, 32, o + 1, 63, F, L, 2, 32, true), "pcm_pitch_bytes"), "pitch");
    CHECK(is(quantCallFault(in + 1, 32, o + 1, 127, F, CPQ_PCM_INTERLEAVED, 2, 32, true), "pcm_pitch_bytes"), "pitch, interleaved");
    CHECK(is(quantCallFault(in + 1, 32, o + 1, 64, F, L, 2, 32, true), "16-byte") || (reinterpret_cast<uintptr_t>(in + 1) & 15) == 0, "d_in alignment");
    CHECK(is(quantCallFault(reinterpret_cast<const double*>(reinterpret_cast<const char*>(in) + 4), 32, o + 1, 64, F, L, 2, 32, false), "8-byte"), "in alignment");
    CHECK(is(quantCallFault(in, 32, o + 1, 64, F, L, 2, 32, false), "element"), "pcm alignment");
    CHECK(is(quantCallFault(in, 32, o, 65, F, L, 2, 32, false), "element"), "pitch alignment");
    CHECK(quantCallFault(in, 32, o + 1, 97, CPQ_PCM_S24, L, 2, 32, false) == nullptr, "S24 on any byte, any pitch");
    CHECK(is(quantCallFault(in, 32, reinterpret_cast<const unsigned char*>(in) + 8, 64, F, L, 2, 32, false), "overlap"), "overlap");
    CHECK(is(quantCallFault(in, 32, reinterpret_cast<const unsigned char*>(in + 4 * 32) - 2, 64, F, L, 2, 32, false), "overlap"), "overlap at the end");
    CHECK(quantCallFault(in, 32, reinterpret_cast<const unsigned char*>(in + 4 * 32), 64, F, L, 2, 32, false) == nullptr, "touching is not overlapping");
    // the bytes a call touches end with its last row, not with the last pitch
    CHECK(quantPcmBytes(F, L, 2, 100, 32) == 3 * 100 + 64 && quantPcmBytes(F, CPQ_PCM_INTERLEAVED, 2, 200, 32) == 200 + 128, "range");
    // slots: whole, partial, outside
    for (int skew = 0; skew < 16; ++skew)
        for (int bytes = 1; bytes <= 80; ++bytes) {
            int covered = 0;
            for (int k = 0; k < 7; ++k) {
                const QuantSlot sl = quantSlot(skew, k, bytes);
                if (sl.hi > sl.lo) covered += sl.hi - sl.lo;
                CHECK(sl.hi <= sl.lo || (sl.lo >= 0 && sl.hi <= bytes && sl.hi - sl.lo <= 16), "slot");
            }
            CHECK(covered == bytes, "skew %d bytes %d: %d covered", skew, bytes, covered);
        }
}

int main()
{
    const int shapers[] = { CPQ_DITHER_FIXED4, CPQ_DITHER_FIXED15, CPQ_DITHER_ADAPTIVE9 };
    const int formats[] = { CPQ_PCM_S16, CPQ_PCM_S24, CPQ_PCM_S32 };
    for (int shaper : shapers)
        for (int format : formats)
            for (int layout = 0; layout < 2; ++layout) {
                const int el = pcm::alignmentOf(format), bits = format == CPQ_PCM_S16 ? 16 : shaper == CPQ_DITHER_FIXED4 ? 24 : 20;
                const int ns[] = { 1, 2, 63, 64, 65, 129, 4099 };
                for (int n : ns) {
                    // tight rows on an aligned buffer; a gap and an off-boundary start; S24: every odd phase class
                    runCase(Case{ shaper, bits, format, layout, 1, n, 0, 0, n });
                    runCase(Case{ shaper, bits, format, layout, 3, n, 5 * el, el, n + 3 });
                    if (format == CPQ_PCM_S24 && n <= 129)
                        for (int phase : { 1, 3, 7, 13, 15 }) runCase(Case{ shaper, bits, format, layout, 2, n, phase, phase, n + 1 });
                }
                runCase(Case{ shaper, bits, format, layout, 33, 65, 2 * el, 16 - el, 70 });      // a second wave, not full
            }
    refusals();
    std::printf("%lld cases, %lld bytes\n%d failed checks\n", g_cases, g_bytes, g_failed);
    return g_failed ? 1 : 0;
}
