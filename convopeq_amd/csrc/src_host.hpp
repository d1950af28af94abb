// src_host.hpp -- the object behind cpq_src (CPQ_SRC_HOST): state, history and the rows of a call on the host, from the plan of
// src_plan.hpp.  No HIP (compiled into tests/sanitize/src_plan_check.cpp).  Equal rates (copy): T = 0, rows copied.
#pragma once

#include <vector>

#include "src_plan.hpp"

namespace cpq {

struct SrcHost {
    SrcGeometry g;
    bool copy = false;
    int channels = 0;
    int64_t startPeriod = 0;
    std::vector<double> taps;
    std::vector<double> hist;       // [channels][srcHistoryBound]
    std::vector<double> virt;
    SrcState s;

    SrcState fresh() const { return srcInitial(g, startPeriod); }
    void reset() { s = fresh(); }
    int64_t outCount(int nIn, bool flush) const
    {
        if (copy) return nIn;
        const SrcCall c = srcPlan(g, s, nIn, flush, fresh());
        return c.j1 - c.j0;
    }
    // rows [channel][stride]; the caller has checked capacity and strides
    int process(const double* in, size_t inStride, int nIn, double* out, size_t outStride, bool flush)
    {
        if (copy) {
            for (int ch = 0; ch < channels && nIn > 0; ++ch) std::copy(in + ch * inStride, in + ch * inStride + nIn, out + ch * outStride);
            return nIn;
        }
        const SrcCall c = srcPlan(g, s, nIn, flush, fresh());
        const size_t hs = (size_t)srcHistoryBound(g);
        virt.resize((size_t)c.nVirt);
        for (int ch = 0; ch < channels; ++ch) {
            std::copy(hist.begin() + ch * hs, hist.begin() + ch * hs + s.hLen, virt.begin());
            if (nIn > 0) std::copy(in + ch * inStride, in + ch * inStride + nIn, virt.begin() + s.hLen);
            srcRowHost(g, taps.data(), virt.data(), c, out + ch * outStride);
            std::copy(virt.begin() + (c.nVirt - c.hKeep), virt.begin() + c.nVirt, hist.begin() + ch * hs);
        }
        s = c.next;
        return (int)(c.j1 - c.j0);
    }
};

}  // namespace cpq
