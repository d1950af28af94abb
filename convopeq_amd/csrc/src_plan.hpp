// src_plan.hpp -- the plan of one cpq_src_process call: pure functions, no HIP (compiled alone into
// tests/sanitize/src_plan_check.cpp).  src_host.hpp holds the object that computes the rows from it, engine_src.cpp the C ABI.
//
// A stream is the concatenation x of everything received since creation, reset or the last flush, zero before its first index
// (start) and, at a flush, zero from its end on.  With (L, M, T, taps) of cpq::resampleDesign, output j is
//     acc = 0;  for k = 0 ... T - 1:  acc = fma(taps[(j M) mod L][k], x[floor(j M / L) + T / 2 - k], acc)
// and a call emits every j, in order, whose newest input floor(j M / L) + T / 2 has been received (with flush: every j below
// ceil(n_total L / M)).  Positions are 64-bit and never multiplied by L or M: with j = q L + r,
//     floor(j M / L) = q M + floor(r M / L),      (j M) mod L = (r M) mod L
// so a stream may run on while its input and output positions stay below 2^62.  What the loop over a call's outputs sees is
// call-relative and 32-bit: v, an index into the
// call's virtual row [ history | new samples ] (v = input index - base), the centre c = floor(j M / L) + T / 2 - base of an
// output and its phase.  Between calls the object keeps the samples from the first one its next output reads: at most
// T + ceil(M / L) per channel.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "resample_design.hpp"

namespace cpq {

struct SrcGeometry { int L = 1, M = 1, T = 0; };
struct SrcState {
    int64_t start = 0;      // first input index of the stream: x is zero before it
    int64_t nRecv = 0;      // one past the newest input received
    int64_t jNext = 0;      // the next output
    int hLen = 0;           // samples kept: inputs nRecv - hLen ... nRecv - 1
};
struct SrcCall {
    int64_t j0 = 0, j1 = 0;     // the call emits outputs j0 ... j1 - 1
    int64_t base = 0;           // input index of v = 0
    int c0 = 0, phase = 0;      // of output j0
    int nVirt = 0;              // hLen + n_in: length of the virtual row
    int hKeep = 0;              // history extent behind the call
    SrcState next;
};

// floor(j M / L)
inline int64_t srcFloorIn(int64_t j, int L, int M) { return (j / L) * M + ((j % L) * M) / L; }
// (j M) mod L
inline int srcPhase(int64_t j, int L, int M) { return (int)(((j % L) * M) % L); }
// the first j with floor(j M / L) >= x, that is ceil(x L / M); x >= 0
inline int64_t srcFirstOutAt(int64_t x, int L, int M) { return (x / M) * L + ((x % M) * L + M - 1) / M; }
// most samples the object keeps per channel
inline int srcHistoryBound(const SrcGeometry& g) { return g.T + (g.M + g.L - 1) / g.L; }
// most outputs of a call of maxIn samples, flush included
inline int64_t srcMaxOut(const SrcGeometry& g, int maxIn) { return srcFirstOutAt((int64_t)maxIn + g.T / 2, g.L, g.M) + 1; }

inline SrcState srcInitial(const SrcGeometry& g, int64_t startPeriod)
{
    SrcState s;
    s.start = s.nRecv = startPeriod * g.M;
    s.jNext = startPeriod * g.L;
    return s;
}

inline int64_t srcFirstRead(const SrcGeometry& g, const SrcState& s, int64_t j)
{
    return std::max<int64_t>(s.start, srcFloorIn(j, g.L, g.M) - g.T / 2 + 1);
}

// the call of nIn samples on state s; fresh: the state a flush leaves
inline SrcCall srcPlan(const SrcGeometry& g, const SrcState& s, int nIn, bool flush, const SrcState& fresh)
{
    SrcCall c;
    const int64_t nRecv = s.nRecv + nIn;
    int64_t j1;
    if (flush) j1 = srcFirstOutAt(nRecv, g.L, g.M);
    else {
        const int64_t x = nRecv - g.T / 2;
        j1 = x > 0 ? srcFirstOutAt(x, g.L, g.M) : 0;
    }
    c.j0 = s.jNext;
    c.j1 = std::max(j1, s.jNext);
    c.base = s.nRecv - s.hLen;
    c.nVirt = s.hLen + nIn;
    c.c0 = (int)(srcFloorIn(c.j0, g.L, g.M) + g.T / 2 - c.base);
    c.phase = srcPhase(c.j0, g.L, g.M);
    if (flush) {
        c.next = fresh;
        c.hKeep = 0;
    } else {
        c.next = s;
        c.next.nRecv = nRecv;
        c.next.jNext = c.j1;
        c.hKeep = (int)std::max<int64_t>(0, nRecv - srcFirstRead(g, s, c.j1));
        c.next.hLen = c.hKeep;
    }
    return c;
}

// the call's outputs of one channel, in the order of the definition: virt is the virtual row, zero outside 0 ... nVirt - 1
inline void srcRowHost(const SrcGeometry& g, const double* taps, const double* virt, const SrcCall& call, double* out)
{
    int c = call.c0, phase = call.phase;
    for (int64_t o = 0; o < call.j1 - call.j0; ++o) {
        const double* h = taps + (size_t)phase * g.T;
        // the terms outside the row multiply a zero and leave the sum as it is: they are passed over
        const int k0 = std::max(0, c - (call.nVirt - 1)), k1 = std::min(g.T - 1, c);
        double acc = 0.0;
        for (int k = k0; k <= k1; ++k) acc = std::fma(h[k], virt[c - k], acc);
        out[o] = acc;
        phase += g.M;           // the next output: (j M) mod L and floor(j M / L) stepped, no product
        c += phase / g.L;
        phase %= g.L;
    }
}

}  // namespace cpq
