// engine_upload.cpp -- the pinned staging ring behind the small host -> device uploads of a call (see engine_internal.hpp): every
// stage's tables (plan groups, EQ, processor level) go through stageUpload.
#include "engine_internal.hpp"

using namespace cpqi;

namespace cpqi {

// Small host -> device uploads on the processing path (chunk schedules, per-stream gains / flags / fade tables): staged
// through a ring of pinned memory so that the copy is truly stream-ordered, never blocks the host, and never reads host
// storage that has gone out of scope (a pageable hipMemcpyAsync is only safe because the runtime happens to stage it
// synchronously).  Uploads larger than a quarter of the ring take the plain copy and wait for it.
int stageUpload(cpq_engine* e, void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) return CPQ_OK;
    ++e->uploadSeq;
    PinnedRing& r = e->pinned;
    if (!r.host) {
        r.cap = (size_t)8 << 20;
        CPQ_TRY(allocAll(e, { { r.host, r.cap } }, "pinned staging ring could not be allocated"));
    }
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (need > r.cap / 4) {
        CPQ_HIP(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream));
        CPQ_HIP(e, hipStreamSynchronize(e->stream));
        return CPQ_OK;
    }
    if (r.head + need > r.cap) r.head = 0;
    const size_t begin = r.head, end = r.head + need;
    // uploads still in flight that own bytes of [begin, end) must have run; they retire in issue order
    size_t done = 0;
    for (; done < r.pending.size(); ++done) {
        const PinnedRing::Pending& p = r.pending[done];
        bool overlapsLater = false;
        for (size_t k = done; k < r.pending.size() && !overlapsLater; ++k)
            overlapsLater = r.pending[k].begin < end && begin < r.pending[k].end;
        if (!overlapsLater) break;
        CPQ_HIP(e, hipEventSynchronize(p.ev));
        r.freeEvents.push_back(p.ev);
    }
    if (done) r.pending.erase(r.pending.begin(), r.pending.begin() + (long)done);
    // retire whatever has completed anyway (keeps the list short)
    while (!r.pending.empty() && hipEventQuery(r.pending.front().ev) == hipSuccess) {
        r.freeEvents.push_back(r.pending.front().ev);
        r.pending.erase(r.pending.begin());
    }
    (void)hipGetLastError();            // hipEventQuery reports "not ready" as an error code
    std::memcpy(r.host + begin, src, bytes);
    CPQ_HIP(e, hipMemcpyAsync(dst, r.host + begin, bytes, hipMemcpyHostToDevice, e->stream));
    hipEvent_t ev;
    if (!r.freeEvents.empty()) { ev = r.freeEvents.back(); r.freeEvents.pop_back(); }
    else CPQ_HIP(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    CPQ_HIP(e, hipEventRecord(ev, e->stream));
    r.pending.push_back(PinnedRing::Pending{ begin, end, ev });
    r.head = end;
    return CPQ_OK;
}

void freePinnedRing(cpq_engine* e)
{
    PinnedRing& r = e->pinned;
    if (!r.host) return;
    for (auto& p : r.pending) (void)hipEventDestroy(p.ev);
    for (auto& ev : r.freeEvents) (void)hipEventDestroy(ev);
    r.pending.clear();
    r.freeEvents.clear();
    r.host.reset();
}

}  // namespace cpqi
