// nuc_replay.hpp -- the integer state of the reference's non-uniform convolver, replayed on the host once per call of a plan
// group (engine_native.cpp) before anything is launched: Add()'s input fill per layer and the distributed tail MAC
// (src/MKLNonUniformConvolver.cpp:1431-1545), Get()'s output ring with its short reads and the delay-line reader
// (:1376-1402, :1606-1688), one Add + Get pair per chunk of block_size samples.  planNucCall steps that state over the chunks of
// one call and returns everything the call's launches need as plain data: the chunk table that goes to the device, blocks and
// remainder per layer, and the decisions that pick the launch sequence (which layers are transformed straight from the call's
// input, whether layer 0 writes the output rows itself, whether the tails run ahead of it or its ring read waits for them).
// Integers only; no HIP, no engine: engine_native.cpp builds the plan in groupsAppend and then only carries it out.
// tests/sanitize/nuc_replay_check.cpp drives this header alone, on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace cpqi {

// cpq_nuc_plan has three layers: part_size[3] and its kin.  A call's plan below is sized by that, and so are the three
// accumulator destinations one gather launch takes (engine_native.cpp: dst[3]) -- at most three layers accumulate.
constexpr int kNucMaxLayers = 3;

// What a layer carries over when its group is resized or a member is moved to a group of its own: plain host state.
struct LayerState {
    int head = 0, histSel = 0, accSel = 0, fill = 0;     // FDL ring head, ping-pong selectors, input fill (inputPos)
    // host replay of the reference's integer state: layer 0 -- samples written to / read from the output ring
    // (m_ringAvail = wPos - rPos); tail layers -- delayWriteCursor / delayReadCursor, the distributed MAC's progress
    bool distributing = false;
    int nextPart = 0;
    long long wPos = 0, rPos = 0;
};

// The planners are templates over the layer type: whatever derives from LayerState and has the geometry the replay reads as
// members -- P (partition size), K (partitions of the IR), ppc (partsPerCallback, :988-994), outputDelay
// (outputDelaySamples, :1005-1024), nbMax (blocks one call can fill).  NativeLayer owns those values.

// entries of the largest chunk table a call of up to maxCall samples in chunks of B can need
template <typename Layer>
int nucTabEntries(const Layer* layers, size_t L, int maxCall, int B)
{
    const int chunks = (maxCall + B - 1) / B + 1;
    int n = 2 * chunks;                                             // layer 0: pos, cnt per chunk
    for (size_t l = 1; l < L; ++l) n += chunks + layers[l].nbMax + 1;     // sched per chunk, put position per block
    return n;
}

// the engine facts the decisions read
struct NucCallFacts {
    int B = 0;                  // chunk length (block_size)
    int nCh = 0;                // rows of the call's buffers
    int usedCh = 0;             // the group's launched local channels
    bool identityMap = false;   // local channel i = row i of the call's buffers
    bool anyDirect = false;     // a direct head sits between layer 0 and the tails in Get()
    int kP = 0;                 // the partition size whose forward transform carries side work and whose inverse adds the tails
};

struct NucCallPlan {
    int n = 0, chunks = 0;
    size_t L = 0;
    // The chunk table as the device reads it: layer 0's read position and count per chunk; per tail layer the delay-line read
    // position per chunk (-1 = skip) and the delay-line position of every block whose partition fills in this call (-1: the
    // block is abandoned inside the call and never reaches the delay line).
    std::vector<long long> tab;
    size_t offs[2 * kNucMaxLayers + 1] = {};    // layer l: [2 l] pos / sched, [2 l + 1] cnt / put positions; [2 L] = tab.size()
    long long w0 = 0, r0 = 0;                   // layer 0's write / read positions before the call
    int lastGot = 0;                            // Get()'s return value summed over the chunks
    struct Layer {
        int nb = 0, rem = 0;                    // partitions that fill in this call, input left over behind them
        bool straight = false;                  // all nb blocks are transformed straight from the call's input: nothing accumulates
    };
    Layer layer[kNucMaxLayers];
    int nAcc = 0, accLayer[kNucMaxLayers] = {}; // the layers that accumulate the call's input (the ones that are not straight)
    // layer 0 at kP samples, transformed straight from the input, is held back: its launch can carry the other layers'
    // accumulation and the call's table (one launch instead of two and a copy)
    bool hold0 = false;
    // Whole-block call on an empty ring, every chunk's Get() taking exactly the chunk this call's blocks produce, members = all
    // rows in order: the inverse transform writes the output rows itself, no ring put / get (the ring stays empty, its positions
    // advanced together by the replay)
    bool direct = false;
    // Layer 0's transform adds the tail layers' delay-line blocks as it stores the output rows: every kP-sample block is one
    // chunk and nothing sits between layer 0 and the tails in Get() (no direct head).  The tail layers then run FIRST.
    bool addTails = false;
    // Get() reads layer 0's ring chunk by chunk and then adds the tails' delay-line blocks: with nothing in between (no direct
    // head) the read waits for the tails' read-add, whose pass over the output does both
    bool getDeferred = false;
    // a launch outcome, not a decision: the table went out with the call's first launch (kernel arguments).  Recorded by
    // groupsAppend, which knows the launchers' limits.
    bool tabOnDevice = false;

    const long long* pos0() const { return tab.data() + offs[0]; }
    const long long* cnt0() const { return tab.data() + offs[1]; }
    const long long* sched(size_t l) const { return tab.data() + offs[2 * l]; }
    const long long* put(size_t l) const { return tab.data() + offs[2 * l + 1]; }
};

// One call of n samples: steps the layers' replay state (wPos, rPos, distributing, nextPart -- fill, head and the selectors move
// when the blocks are launched) and refills `p` in place.  L <= kNucMaxLayers.
template <typename Layer>
void planNucCall(NucCallPlan& p, Layer* layers, size_t L, int n, const NucCallFacts& f)
{
    const int q = f.B;
    p.n = n;
    p.chunks = (n + q - 1) / q;
    p.L = L;
    p.w0 = layers[0].wPos;
    p.r0 = layers[0].rPos;
    const bool rowsAreCallRows = f.identityMap && f.usedCh == f.nCh;
    const bool wasEmpty = layers[0].fill == 0 && p.r0 == p.w0;      // no input waiting, nothing in the output ring
    size_t at = 0;
    p.nAcc = 0;
    for (size_t l = 0; l < L; ++l) {
        const Layer& t = layers[l];
        const int total = t.fill + n;
        p.layer[l].nb = total / t.P;
        p.layer[l].rem = total - p.layer[l].nb * t.P;
        // A layer whose accumulator is empty and for which the call is whole partitions needs no accumulation when the group's
        // rows are the call's rows
        p.layer[l].straight = rowsAreCallRows && t.fill == 0 && n % t.P == 0 && n / t.P <= t.nbMax;
        if (!p.layer[l].straight) p.accLayer[p.nAcc++] = (int)l;
        p.offs[2 * l] = at; at += (size_t)p.chunks;
        p.offs[2 * l + 1] = at;
        at += (l == 0) ? (size_t)p.chunks : (size_t)p.layer[l].nb;
    }
    p.offs[2 * L] = at;
    p.tab.assign(at, -1);
    p.hold0 = p.layer[0].straight && layers[0].P == f.kP;

    int fillOf[kNucMaxLayers], nbOf[kNucMaxLayers], pendingIdx[kNucMaxLayers];      // pendingIdx: this call's block whose MAC is still being distributed
    for (size_t l = 0; l < L; ++l) { fillOf[l] = layers[l].fill; nbOf[l] = 0; pendingIdx[l] = -1; }
    p.lastGot = 0;
    p.direct = rowsAreCallRows && wasEmpty && n % layers[0].P == 0;
    for (int c = 0; c < p.chunks; ++c) {
        const int len = std::min(q, n - c * q);
        for (size_t l = 0; l < L; ++l) {
            Layer& t = layers[l];
            // Add(): input accumulation; a partition that fills is transformed at once (:1448-1494)
            fillOf[l] += len;
            while (fillOf[l] >= t.P) {
                fillOf[l] -= t.P;
                if (l == 0) t.wPos += t.P;                          // processLayerBlock -> ringWrite
                else {
                    // a block still distributing is abandoned (:1487-1490): it never reaches the delay line (one of an
                    // earlier call already sits at wPos and is overwritten by this one)
                    if (t.distributing && pendingIdx[l] >= 0) p.tab[p.offs[2 * l + 1] + (size_t)pendingIdx[l]] = -1;
                    p.tab[p.offs[2 * l + 1] + (size_t)nbOf[l]] = t.wPos;    // where delayLineWrite will put it -- if its MAC completes
                    pendingIdx[l] = nbOf[l];
                    t.distributing = true;
                    t.nextPart = 0;
                }
                ++nbOf[l];
            }
            if (l > 0 && t.distributing) {                          // distributed MAC, once per Add() (:1497-1545)
                t.nextPart = std::min(t.nextPart + t.ppc, t.K);
                if (t.nextPart >= t.K) { t.wPos += t.P; t.distributing = false; t.nextPart = 0; }
            }
            // Get()
            if (l == 0) {
                const long long avail = t.wPos - t.rPos;
                const long long toRead = std::min<long long>(len, avail);
                p.tab[p.offs[0] + (size_t)c] = t.rPos;
                p.tab[p.offs[1] + (size_t)c] = toRead;
                // direct: this chunk's Get() takes exactly the chunk this call's blocks produce
                p.direct = p.direct && t.rPos == p.w0 + (long long)c * q && toRead == len;
                p.lastGot += (int)toRead;
                t.rPos += toRead;
            } else {
                const long long maxRead = t.wPos >= t.outputDelay ? t.wPos - t.outputDelay : 0;
                const long long start = std::max(t.rPos, maxRead);
                if (start + len <= t.wPos) { p.tab[p.offs[2 * l] + (size_t)c] = start; t.rPos = start + len; }
            }
        }
    }
    p.addTails = p.direct && L >= 2 && L <= 3 && layers[0].P == f.kP && f.B == f.kP && !f.anyDirect;
    p.getDeferred = !p.direct && !f.anyDirect && L >= 2 && L <= 3;
    p.tabOnDevice = false;
}

}  // namespace cpqi
