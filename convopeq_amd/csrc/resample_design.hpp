// resample_design.hpp -- host side of the IR sample-rate conversion: the polyphase filter of a rate pair, the call checks, the
// host path and the tail trim.  See resample_design.cpp; the device side is resample_kernels.hip / engine_resample.cpp.
#pragma once

#include <cstdint>
#include <vector>

#include "convopeq_mi355x.h"

namespace cpq {

constexpr double kResampleAttenDb = 180.0;      // the Kaiser window's design attenuation
constexpr double kResampleEdge = 0.98;          // -6 dB point as a fraction of the lower Nyquist frequency
constexpr double kResampleHalfBand = 0.02;      // the transition reaches this far to either side of it: 0.96 ... 1.0

struct ResampleDesign {
    int L = 0, M = 0, T = 0;
    double groupDelay = 0.0, cutoff = 0.0;
    std::vector<double> taps;       // [L][T]
};
// CPQ_OK, or CPQ_ERR_UNSUPPORTED with the reason in why (a rate that is no whole number of Hz in 8000 ... 768000, L or M above 1280)
int resampleDesign(double inRate, double outRate, ResampleDesign& d, const char** why);
// ceil(n L / M)
inline int64_t resampleOutLen(int n, int L, int M) { return ((int64_t)n * L + M - 1) / M; }

// What every resample call checks before it allocates: CPQ_OK with copy set (rates no more than 1e-6 apart), CPQ_OK with the
// design filled, or the refusal with its reason in why.  designKnown: d already is the design of (in->sample_rate, targetRate) --
// a batch designs once per source rate, the design being the expensive part of the check.
int resampleCheck(const cpq_ir_buffer* in, double targetRate, int phase, bool& copy, ResampleDesign& d, const char** why, bool designKnown);
// outputs j0 ... j1 - 1 of one row, in the order convopeq_mi355x.h states
void resampleRowHost(const ResampleDesign& d, const double* x, int n, double* y, int64_t j0, int64_t j1);
// resampleIR's tail: rows [channels][nOut] -> out, every channel cut at its own effective length; CPQ_ERR_OOM
int resampleFinish(const double* rows, int channels, int nOut, double rate, cpq_ir_buffer* out);
int resampleCopy(const cpq_ir_buffer* in, cpq_ir_buffer* out);

}  // namespace cpq
