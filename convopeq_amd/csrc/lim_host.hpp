// lim_host.hpp -- the object behind cpq_limiter (CPQ_LIM_HOST): state, history, gains, telemetry and the rows of a call on the
// host, from the definition and the plan of lim_plan.hpp.  No HIP (compiled into tests/sanitize/lim_plan_check.cpp).  A call
// evaluates the six steps as they are written, over the whole call at once: the yardstick the device object is held to, bit for bit.
#pragma once

#include <vector>

#include "lim_plan.hpp"

namespace cpq {

struct LimHost {
    int W = 0, mask = 0, streams = 0;
    double c = 1.0;
    std::vector<double> gains;          // [streams]
    std::vector<double> hist;           // [2 streams][limHalo(W)]: the tail of u
    std::vector<LimPartial> tel;        // [streams]
    std::vector<double> u[2], r, m;
    LimState s;

    void init(int window, int phaseMask, double ceiling, int nStreams)
    {
        W = window; mask = phaseMask; c = ceiling; streams = nStreams;
        gains.assign((size_t)streams, 1.0);
        hist.assign(2 * (size_t)streams * (size_t)limHalo(W), 0.0);
        tel.assign((size_t)streams, LimPartial{ 1.0, 0 });
        s = LimState{};
    }
    void reset()
    {
        s = LimState{};
        tel.assign((size_t)streams, LimPartial{ 1.0, 0 });
    }
    // rows [2 streams][stride]; the caller has checked strides and capacity.  Returns the outputs per row.
    int process(const double* in, long long inStride, int n, double* out, long long outStride, bool flush)
    {
        const LimCall call = limPlan(W, s, n, flush);
        const LimLaunch a = limLaunch(W, mask, c, call, streams, inStride, outStride, 0);
        const int halo = limHalo(W), reach = limReach(W), M = limM(W), len = call.nOut + halo, nR = call.nOut + reach;
        const int lo = call.hLen - halo;        // v of slot 0
        u[0].resize((size_t)len); u[1].resize((size_t)len);
        r.resize((size_t)nR); m.resize((size_t)nR);
        for (int st = 0; st < streams; ++st) {
            const double g = gains[(size_t)st];
            for (int ch = 0; ch < 2; ++ch)
                for (int k = 0; k < len; ++k) u[ch][(size_t)k] = limVirt(a, hist.data(), in, g, 2 * st + ch, lo + k);
            for (int q = 0; q < nR; ++q) r[(size_t)q] = limRequired(&u[0][(size_t)q + kPeakHist], &u[1][(size_t)q + kPeakHist], mask, c);
            for (int q = M - 1; q < nR; ++q) {
                double v = r[(size_t)q];
                for (int j = 1; j < M; ++j) v = r[(size_t)(q - j)] < v ? r[(size_t)(q - j)] : v;
                m[(size_t)q] = v;
            }
            LimPartial t = call.first ? LimPartial{ 1.0, 0 } : tel[(size_t)st];
            for (int o = 0; o < call.nOut; ++o) {
                const double env = limEnvelope(&m[(size_t)(o + reach)], W);
                limFold(t, env, env < 1.0 ? 1 : 0);
                for (int ch = 0; ch < 2; ++ch) out[(long long)(2 * st + ch) * outStride + o] = u[ch][(size_t)limDelaySlot(W, o)] * env;
            }
            tel[(size_t)st] = t;
            for (int ch = 0; ch < 2; ++ch)      // slot of v: v - lo; the kept tail is v = keepShift ... keepShift + keepLen - 1
                for (int k = 0; k < a.keepLen; ++k) hist[(size_t)(2 * st + ch) * (size_t)halo + (size_t)k] = u[ch][(size_t)(a.keepShift + k - lo)];
        }
        s = call.next;
        return call.nOut;
    }
};

}  // namespace cpq
