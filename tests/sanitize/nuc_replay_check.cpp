// Host-only driver for convopeq_amd/csrc/nuc_replay.hpp (tests/test_nuc_replay_cpu.py): the plan of a plan group's call, with no
// HIP and no engine.  Integers only, every check is exact.
//   1. split invariance: a stretch of input played as one call, as two calls cut at an odd chunk, as one call per chunk, and
//      ragged stretches (1-sample calls, calls that are no multiple of B) against one call per chunk of the same chunks, give
//      the same per-chunk entries and leave the same layer state
//   2. the reference's invariants per chunk: layer 0 reads min(len, wPos - rPos); a tail reads only if start + len <= wPos with
//      start = max(rPos, wPos - outputDelay); lastGot is the sum of layer 0's counts
//   3. every decision on the smallest input that flips it
//   4. the table never outgrows nucTabEntries for a call of up to maxCall samples
// The layer plans are hand-written cpq_nuc_plan-shaped data (the planner cpq_nuc_plan_compute is not this header's).
//
// Put positions and the cut into calls.  A tail block is stored at the delay line's write position when its partition fills,
// and the write position moves on only when the block's distributed MAC completes.  A block that is abandoned (the next
// partition fills first) is therefore overwritten by its successor at the SAME position.  Inside one call the plan says so with
// a put position of -1; when the successor fills in a later call the earlier table has gone out with the position itself.  Both
// leave the same delay line, so put positions are compared after this normalisation: an entry whose position a later block is stored at is -1.
#include "nuc_replay.hpp"

#include <cstdint>
#include <cstdio>

using namespace cpqi;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

struct Rng {        // seeded, the same everywhere
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

// ---------------------------------------------------------------------------------------------------- plans and layers
struct Layer : LayerState { int P = 0, K = 0, ppc = 1, outputDelay = 0, nbMax = 0; };
struct Plan { const char* name; int B, L, P[3], K[3], ppc[3], delay[3]; };

static std::vector<Layer> makeLayers(const Plan& pl, int maxCall)
{
    std::vector<Layer> v((size_t)pl.L);
    for (int l = 0; l < pl.L; ++l) {
        v[(size_t)l].P = pl.P[l]; v[(size_t)l].K = pl.K[l]; v[(size_t)l].ppc = pl.ppc[l]; v[(size_t)l].outputDelay = pl.delay[l];
        v[(size_t)l].nbMax = (pl.P[l] - 1 + maxCall) / pl.P[l];         // layerGeometry
    }
    return v;
}

static NucCallFacts factsFor(int B) { return NucCallFacts{ B, 4, 4, true, false, 512 }; }

static bool sameState(const LayerState& a, const LayerState& b)
{
    return a.fill == b.fill && a.distributing == b.distributing && a.nextPart == b.nextPart && a.wPos == b.wPos && a.rPos == b.rPos;
}

// ---------------------------------------------------------------------------------------------------- playing calls
struct Chunk { int len; long long pos0, cnt0, sched[2]; bool operator==(const Chunk&) const = default; };
struct Record {
    std::vector<Chunk> chunks;
    std::vector<long long> puts[2];         // per tail layer: the put position of every filled block, in order
    std::vector<Layer> end;
};
struct Saw {
    bool shortRead = false, tailRead[2] = {}, tailSkip[2] = {}, completed[2] = {}, abandonedInCall[2] = {}, abandonedAcross[2] = {},
         timeVaryingSkip = false;
};

// one call through planNucCall and what the engine does behind it to the input fill (runLayerBlocks: fill = rem)
static void call(const Plan& pl, std::vector<Layer>& layers, NucCallPlan& p, int n, int maxCall, const NucCallFacts& f, Record& rec, Saw& saw)
{
    const std::vector<Layer> before = layers;
    planNucCall(p, layers.data(), layers.size(), n, f);
    const size_t L = layers.size();
    CHECK(p.n == n && p.chunks == (n + pl.B - 1) / pl.B && p.L == L);
    CHECK((int)p.tab.size() <= nucTabEntries(layers.data(), L, maxCall, pl.B));
    CHECK(p.offs[2 * L] == p.tab.size() && p.offs[0] == 0 && p.offs[1] == (size_t)p.chunks);
    CHECK(p.w0 == before[0].wPos && p.r0 == before[0].rPos);
    long long got = 0;
    for (int c = 0; c < p.chunks; ++c) {
        Chunk ch{ std::min(pl.B, n - c * pl.B), p.pos0()[c], p.cnt0()[c], { -2, -2 } };
        for (size_t l = 1; l < L; ++l) {
            ch.sched[l - 1] = p.sched(l)[c];
            (ch.sched[l - 1] >= 0 ? saw.tailRead : saw.tailSkip)[l - 1] = true;
        }
        got += ch.cnt0;
        CHECK(ch.cnt0 >= 0 && ch.cnt0 <= ch.len);
        saw.shortRead = saw.shortRead || ch.cnt0 < ch.len;
        rec.chunks.push_back(ch);
    }
    CHECK(p.lastGot == (int)got);
    int nAcc = 0;
    for (size_t l = 0; l < L; ++l) {
        const Layer& b = before[l];
        const NucCallPlan::Layer& pll = p.layer[l];
        CHECK(pll.nb >= 0 && pll.rem >= 0 && pll.rem < b.P && pll.nb * b.P + pll.rem == b.fill + n);
        CHECK(pll.straight == (f.identityMap && f.usedCh == f.nCh && b.fill == 0 && n % b.P == 0 && n / b.P <= b.nbMax));
        if (!pll.straight) { CHECK(nAcc < p.nAcc && p.accLayer[nAcc] == (int)l); ++nAcc; }
        CHECK(layers[l].fill == b.fill && layers[l].head == b.head && layers[l].histSel == b.histSel && layers[l].accSel == b.accSel);
        if (l > 0) {
            CHECK(p.offs[2 * l + 2] - p.offs[2 * l + 1] == (size_t)pll.nb && p.offs[2 * l + 1] - p.offs[2 * l] == (size_t)p.chunks);
            for (int k = 0; k < pll.nb; ++k) {
                rec.puts[l - 1].push_back(p.put(l)[k]);
                if (p.put(l)[k] < 0) { saw.abandonedInCall[l - 1] = true; CHECK(k + 1 < pll.nb); }   // only a successor in the call abandons
            }
            if (layers[l].wPos > b.wPos) saw.completed[l - 1] = true;
        }
        layers[l].fill = pll.rem;
    }
    CHECK(nAcc == p.nAcc);
    if (p.chunks != 1) return;
    // a call of one chunk is one Add + Get pair: the reference's invariants, on the state before and after it
    const int len = n;
    CHECK(p.pos0()[0] == before[0].rPos && p.cnt0()[0] == std::min<long long>(len, layers[0].wPos - before[0].rPos));
    CHECK(layers[0].rPos == before[0].rPos + p.cnt0()[0]);
    CHECK(layers[0].wPos == before[0].wPos + (long long)p.layer[0].nb * layers[0].P);
    for (size_t l = 1; l < L; ++l) {
        const Layer& a = layers[l];
        const long long start = std::max(before[l].rPos, a.wPos - a.outputDelay);
        const bool reads = start + len <= a.wPos;
        CHECK(p.sched(l)[0] == (reads ? start : -1));
        CHECK(a.rPos == (reads ? start + len : before[l].rPos));
        if (reads && start > before[l].rPos && before[l].rPos > 0) saw.timeVaryingSkip = true;     // the reader jumped ahead (:1658-1666)
        CHECK(a.wPos == before[l].wPos || a.wPos == before[l].wPos + a.P);     // at most one block completes per Add
    }
}

static Record play(const Plan& pl, const std::vector<int>& calls, int maxCall, Saw& saw)
{
    Record rec;
    std::vector<Layer> layers = makeLayers(pl, maxCall);
    NucCallPlan p;              // one plan refilled in place, as the PlanGroup's
    for (int n : calls) call(pl, layers, p, n, maxCall, factsFor(pl.B), rec, saw);
    rec.end = layers;
    return rec;
}

static std::vector<long long> normalised(const std::vector<long long>& puts, bool& sawAcross)
{
    std::vector<long long> v = puts;
    long long later = -1;       // the next position further on that a block is stored at (the -1 entries between sat at the same one)
    for (size_t i = v.size(); i-- > 0;) {
        if (v[i] >= 0 && v[i] == later) { v[i] = -1; sawAcross = true; }
        else if (v[i] >= 0) later = v[i];
    }
    return v;
}

static void checkSame(const Record& a, const Record& b, Saw& saw)
{
    CHECK(a.chunks == b.chunks);
    for (int t = 0; t < 2; ++t) CHECK(normalised(a.puts[t], saw.abandonedAcross[t]) == normalised(b.puts[t], saw.abandonedAcross[t]));
    CHECK(a.end.size() == b.end.size());
    for (size_t l = 0; l < a.end.size() && l < b.end.size(); ++l) CHECK(sameState(a.end[l], b.end[l]));
}

// ---------------------------------------------------------------------------------------------------- 1, 2, 4
static void splitInvariance(const Plan& pl, int N, Saw& saw)
{
    const int B = pl.B, maxCall = N * B;
    const Record perChunk = play(pl, std::vector<int>((size_t)N, B), maxCall, saw);
    checkSame(play(pl, { N * B }, maxCall, saw), perChunk, saw);
    for (int cut = 1; cut < N; cut += 2) checkSame(play(pl, { cut * B, (N - cut) * B }, maxCall, saw), perChunk, saw);
    // ragged stretches: the chunks a call of n samples has are B, B, ..., n mod B, so a ragged sequence is compared with the
    // same chunks played one call each
    Rng rng{ 0x5eedull + (uint64_t)pl.P[pl.L - 1] * 31u + (uint64_t)pl.K[pl.L - 1] };
    const int maxRagged = 5 * B + 3;
    for (int round = 0; round < 6; ++round) {
        std::vector<int> calls = { 1, B - 1, B + 1, 2 * B, 3 * B + B / 2, 1, 1 }, chunks;
        int total = 0;
        for (int n : calls) total += n;
        while (total < N * B) {
            const int r = rng.below(10);
            const int n = r == 0 ? 1 : r < 3 ? 1 + rng.below(B) : r < 5 ? B * (1 + rng.below(5)) : 1 + rng.below(maxRagged);
            calls.push_back(n);
            total += n;
        }
        for (int n : calls)
            for (int o = 0; o < n; o += B) chunks.push_back(std::min(B, n - o));
        checkSame(play(pl, calls, maxRagged, saw), play(pl, chunks, maxRagged, saw), saw);
    }
}

static void capacity(const Plan& pl)
{
    const int maxCall = 4 * pl.B + 1;
    std::vector<Layer> layers = makeLayers(pl, maxCall);
    NucCallPlan p, probe;
    Record rec;
    Saw saw;
    const int bound = nucTabEntries(layers.data(), layers.size(), maxCall, pl.B);
    for (int step = 0; step < 2 * pl.P[pl.L - 1]; step += 37) {
        for (int n = 1; n <= maxCall; ++n) {
            std::vector<Layer> copy = layers;
            planNucCall(probe, copy.data(), copy.size(), n, factsFor(pl.B));
            CHECK((int)probe.tab.size() <= bound);
        }
        call(pl, layers, p, 37, maxCall, factsFor(pl.B), rec, saw);
    }
}

// ---------------------------------------------------------------------------------------------------- 3
struct Decided { bool direct, hold0, addTails, getDeferred, straight0; long long w, r, w0; };
// `before`: calls that set the state up; then the call of n samples whose decisions are returned
static Decided decide(const Plan& pl, const std::vector<int>& before, int n, NucCallFacts f)
{
    const int maxCall = 8 * pl.B;
    std::vector<Layer> layers = makeLayers(pl, maxCall);
    NucCallPlan p;
    Record rec;
    Saw saw;
    for (int m : before) call(pl, layers, p, m, maxCall, f, rec, saw);
    call(pl, layers, p, n, maxCall, f, rec, saw);
    CHECK(!p.tabOnDevice);                  // a launch outcome: the planner leaves it off
    return Decided{ p.direct, p.hold0, p.addTails, p.getDeferred, p.layer[0].straight, layers[0].wPos, layers[0].rPos, p.w0 };
}

static void decisions()
{
    const Plan one{ "512", 512, 1, { 512 }, { 4 }, { 1 }, { 0 } };
    const Plan two{ "512/4096", 512, 2, { 512, 4096 }, { 4, 5 }, { 1, 1 }, { 0, 2048 } };
    const Plan three{ "512/4096/32768", 512, 3, { 512, 4096, 32768 }, { 4, 8, 3 }, { 1, 1, 1 }, { 0, 2048, 34816 } };
    const Plan wide{ "1024/8192", 1024, 2, { 1024, 8192 }, { 4, 3 }, { 1, 1 }, { 0, 4096 } };
    const Plan half{ "B 256 under P0 512", 256, 2, { 512, 4096 }, { 4, 3 }, { 1, 1 }, { 0, 2048 } };
    const NucCallFacts f = factsFor(512);
    NucCallFacts hole = f, fewer = f, head = f;
    hole.identityMap = false;
    fewer.usedCh = 2;
    head.anyDirect = true;

    // direct: a whole-partition call on an empty ring with an identity map ...
    Decided d = decide(one, {}, 512, f);
    CHECK(d.direct && d.hold0 && d.straight0 && !d.addTails && !d.getDeferred);
    CHECK(d.w == d.r && d.w == d.w0 + 512);                         // ... leaves wPos and rPos advanced together
    d = decide(one, { 1024 }, 1536, f);
    CHECK(d.direct && d.w == d.r && d.w0 == 1024 && d.w == 2560);
    // ... and not with input waiting (fill != 0)
    d = decide(one, { 100 }, 512, f);
    CHECK(!d.direct && !d.straight0 && !d.hold0);
    // ... not with the ring not empty: 300 + 212 samples fill a partition and read 212 of it, fill is 0 again
    d = decide(one, { 300, 212 }, 512, f);
    CHECK(d.w0 == 512 && !d.direct && d.straight0 && d.hold0);
    // ... not with a hole in the map, or fewer rows than the call has
    d = decide(one, {}, 512, hole);
    CHECK(!d.direct && !d.straight0 && !d.hold0);
    d = decide(one, {}, 512, fewer);
    CHECK(!d.direct && !d.straight0 && !d.hold0);
    // ... not with n % P0 != 0
    d = decide(one, {}, 511, f);
    CHECK(!d.direct && !d.straight0);
    d = decide(one, {}, 513, f);
    CHECK(!d.direct && !d.straight0);
    // ... not with chunks shorter than the partition: the first chunk's Get() finds the ring empty
    d = decide(half, {}, 512, factsFor(256));
    CHECK(!d.direct && d.straight0 && d.hold0 && !d.addTails && d.getDeferred);

    // addTails: P0 == B == kP, 2 or 3 layers, no direct head, on a direct call; getDeferred: its complement on the non-direct side
    d = decide(two, {}, 512, f);
    CHECK(d.direct && d.addTails && !d.getDeferred);
    d = decide(three, {}, 1024, f);
    CHECK(d.direct && d.addTails && !d.getDeferred);
    d = decide(two, {}, 512, head);
    CHECK(d.direct && !d.addTails && !d.getDeferred);
    d = decide(wide, {}, 1024, factsFor(1024));
    CHECK(d.direct && !d.addTails && !d.getDeferred && !d.hold0 && d.straight0);        // P0 == B but not kP
    d = decide(one, {}, 512, f);
    CHECK(d.direct && !d.addTails && !d.getDeferred);                                   // no tails
    d = decide(two, { 300 }, 512, f);
    CHECK(!d.direct && !d.addTails && d.getDeferred);
    d = decide(three, { 300 }, 512, f);
    CHECK(!d.direct && !d.addTails && d.getDeferred);
    d = decide(two, { 300 }, 512, head);
    CHECK(!d.direct && !d.addTails && !d.getDeferred);
    d = decide(one, { 300 }, 512, f);
    CHECK(!d.direct && !d.addTails && !d.getDeferred);

    // hold0: only at P0 == kP on a straight layer 0
    d = decide(two, {}, 2048, f);
    CHECK(d.hold0 && d.straight0);
    d = decide(two, { 300 }, 2048, f);
    CHECK(!d.hold0 && !d.straight0);
    d = decide(wide, {}, 2048, factsFor(1024));
    CHECK(!d.hold0 && d.straight0);
    // a straight tail layer: the call is whole partitions of it too, and nothing accumulates
    {
        std::vector<Layer> layers = makeLayers(two, 8 * 512);
        NucCallPlan p;
        planNucCall(p, layers.data(), layers.size(), 4096, f);
        CHECK(p.layer[1].straight && p.nAcc == 0 && p.layer[1].nb == 1 && p.put(1)[0] == 0);
        for (Layer& t : layers) t.fill = 0;
        planNucCall(p, layers.data(), layers.size(), 512, f);
        CHECK(!p.layer[1].straight && p.nAcc == 1 && p.accLayer[0] == 1 && p.layer[1].nb == 0 && p.layer[1].rem == 512);
    }
}

int main()
{
    const Plan plans[] = {
        { "64", 64, 1, { 64 }, { 4 }, { 1 }, { 0 } },
        { "64/256", 64, 2, { 64, 256 }, { 8, 5 }, { 1, 2 }, { 0, 512 } },
        { "64/256/1024", 64, 3, { 64, 256, 1024 }, { 8, 8, 6 }, { 1, 2, 1 }, { 0, 512, 2560 } },
        // ppc small against K: five Adds to complete, four whole chunks to a partition -- every block is abandoned unless short
        // chunks bring more Adds
        { "64/256 abandoning", 64, 2, { 64, 256 }, { 8, 9 }, { 1, 2 }, { 0, 512 } },
        { "64/256/1024 abandoning", 64, 3, { 64, 256, 1024 }, { 8, 9, 18 }, { 1, 2, 1 }, { 0, 512, 2560 } },
        // a quantum that is no power of two: layer 0 reads short; 10 or 11 Adds to a tail partition that needs 11
        { "48 in 64/512", 48, 2, { 64, 512 }, { 8, 11 }, { 1, 1 }, { 0, 512 } },
        // the tail partition above its output delay: the reader skips blocks (lti_valid == 0)
        { "64/256 time-varying", 64, 2, { 64, 256 }, { 2, 3 }, { 1, 1 }, { 0, 128 } },
    };
    Saw saw;
    for (const Plan& pl : plans) {
        splitInvariance(pl, 3 * 4 * pl.P[pl.L - 1] / pl.B + 5, saw);
        capacity(pl);
    }
    CHECK(saw.shortRead && saw.timeVaryingSkip);
    for (int t = 0; t < 2; ++t)
        CHECK(saw.tailRead[t] && saw.tailSkip[t] && saw.completed[t] && saw.abandonedInCall[t] && saw.abandonedAcross[t]);
    decisions();
    std::printf("nuc_replay_check: %d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
