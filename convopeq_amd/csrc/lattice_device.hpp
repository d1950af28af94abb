// lattice_device.hpp -- the device code the dither stage (dither_kernels.hip) and the shaper scorer (score_kernels.hip) share:
// the xoshiro256++ draw and LatticeNoiseShaper::processSample (src/LatticeNoiseShaper.h:178-293), one sample of one channel.
// Included inside a kernel file, after kernels.hpp; every function is inlined into the kernel that calls it.
#pragma once

#include "kernels.hpp"

namespace cpq {
namespace {

__device__ __forceinline__ unsigned long long dRotl(unsigned long long x, int k) { return (x << k) | (x >> (64 - k)); }

__device__ __forceinline__ double dUniform(unsigned long long (&s)[4])
{
    const unsigned long long result = dRotl(s[0] + s[3], 23) + s[0];
    const unsigned long long t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = dRotl(s[3], 45);
    return (double)(result >> 11) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ double dFiniteOrZero(double v) { return fabs(v) < __builtin_huge_val() ? v : 0.0; }

// LatticeNoiseShaper::processSample: x in, yq out; st, c and s are the channel's states, coefficients and generator
__device__ __forceinline__ double dLatticeSample(double x, double (&st)[kLatticeOrder], const double (&c)[kLatticeOrder],
                                                 unsigned long long (&s)[4], const DitherParams& p)
{
    // computeFeedback: lanes j = 0..3 of mul_pd then fmadd_pd, the horizontal add, then state[8] on its own
    const double p0 = __builtin_fma(st[4], c[4], st[0] * c[0]);
    const double p1 = __builtin_fma(st[5], c[5], st[1] * c[1]);
    const double p2 = __builtin_fma(st[6], c[6], st[2] * c[2]);
    const double p3 = __builtin_fma(st[7], c[7], st[3] * c[3]);
    const double fb = ((p0 + p2) + (p1 + p3)) + st[8] * c[8];
    const double y = x + fb;
    double v = y;                                                           // quantize: a NaN passes both comparisons
    if (v < -1.0) v = -1.0;
    else if (v > p.maxV) v = p.maxV;
    const double u1 = dUniform(s);
    const double u2 = dUniform(s);
    v += (u1 + u2 - 1.0) * p.scale;
    const double q = __builtin_rint(v * p.invScale);
    const double minQ = -p.invScale, maxQ = p.invScale - 1.0;
    const double yq = (q < minQ ? minQ : (maxQ < q ? maxQ : q)) * p.scale;  // std::clamp: a NaN stays
    const double lim = 2.0 * p.scale;
    const double error = dFiniteOrZero(yq - y);
    double f = error < -lim ? -lim : (lim < error ? lim : error);
#pragma unroll
    for (int i = 0; i < kLatticeOrder; ++i) {                               // advanceState
        const double b = st[i];
        const double nf = f + c[i] * b;
        const double nb = c[i] * f + b;
        st[i] = nb < -2.0 ? -2.0 : (2.0 < nb ? 2.0 : nb);
        f = nf;
    }
    return yq;
}

}  // namespace
}  // namespace cpq
