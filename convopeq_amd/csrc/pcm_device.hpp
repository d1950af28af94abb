// pcm_device.hpp -- the integer code of a sample (include/convopeq_mi355x.h, "out, S24/S32"), which the PCM converters
// (pcm_kernels.hip) and the quantizer (quant_kernels.hip) share.  Included inside a kernel file, after kernels.hpp.
#pragma once

#include "kernels.hpp"

namespace cpq {
namespace {

// rint(x * 2^(bits-1)), ties to even, saturated, NaN -> 0
template <int BITS>
__device__ __forceinline__ int pcmQuantize(double x)
{
    constexpr double kScale = (double)(1ll << (BITS - 1));
    double v = rint(x * kScale);
    if (v != v) v = 0.0;
    v = (-kScale < v) ? v : -kScale;
    v = (v < kScale - 1.0) ? v : kScale - 1.0;
    return (int)v;
}

}  // namespace
}  // namespace cpq
