// object_support.hpp -- what the objects beside cpq_engine (cpq_loudness, cpq_limiter, cpq_quantizer, cpq_scorer, cpq_learner; not yet cpq_src) and the
// engine-less loader calls (cpq_ir_resample*, cpq_ir_minimum_phase*) share, written once:
//
//   failTo          the message into the object's lastError (the sink), or into cpq_last_error(NULL) before an object exists
//   CPQ_OBJ_HIP     a HIP call that ends the calling function with CPQ_ERR_DEVICE, the call's text and no HIP error left pending
//   TimingEvents    owner of N events: all created or none, destroyed with their owner
//   RowStage        rows of doubles on the device for rows that arrive on the host (or in place): grown on demand after the
//                   stream has passed the allocation that goes, and the one spelling of the pitched copy up and down
//   setStream       "one stream": what was enqueued on the old stream has run before a call on the new one touches the state
//   guardAlloc      a callable whose std::exception is CPQ_ERR_OOM "host allocation failed"
//
// Needs only the HIP runtime, device_buffers.hpp and cpqi::fail; includes nothing of the engine.
#pragma once

#include "device_buffers.hpp"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <string>

namespace cpqi {

// sink: the object's lastError, or null before an object exists (cpq_last_error(NULL) and the objects' *_last_error(NULL) have it)
inline int failTo(std::string* sink, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (!sink) return fail(nullptr, code, "%s", buf);
    *sink = buf;
    return code;
}

#define CPQ_OBJ_HIP(sink, call)                                                                                   \
    do {                                                                                                          \
        hipError_t err__ = (call);                                                                                \
        if (err__ != hipSuccess) {                                                                                \
            (void)hipGetLastError();                                                                              \
            return cpqi::failTo((sink), CPQ_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(err__));        \
        }                                                                                                         \
    } while (0)

// Destroyed with the object that holds it: a member declared after the device buffers goes before them, and nothing here waits,
// so whoever destroys the owner has waited for the work that records into its events.
template <int N>
class TimingEvents {
public:
    TimingEvents() = default;
    TimingEvents(const TimingEvents&) = delete;
    TimingEvents& operator=(const TimingEvents&) = delete;
    ~TimingEvents() { reset(); }

    void reset()
    {
        for (auto& e : ev_) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
    // all N events, or none of them and CPQ_ERR_DEVICE
    int create(std::string* sink)
    {
        for (auto& e : ev_) {
            const hipError_t err = hipEventCreate(&e);
            if (err == hipSuccess) continue;
            e = nullptr;
            reset();
            (void)hipGetLastError();
            return failTo(sink, CPQ_ERR_DEVICE, "hipEventCreate(&e) failed: %s", hipGetErrorString(err));
        }
        return CPQ_OK;
    }
    hipEvent_t operator[](int i) const { return ev_[i]; }
    // milliseconds from event i to event j, both recorded and passed; -1.0 where the runtime cannot say, with no error left pending
    double elapsed(int i, int j) const
    {
        float ms = 0.0f;
        if (ev_[i] && ev_[j] && hipEventElapsedTime(&ms, ev_[i], ev_[j]) == hipSuccess) return ms;
        (void)hipGetLastError();
        return -1.0;
    }

private:
    hipEvent_t ev_[N] = {};
};

// [rows][cap] doubles.  The capacity a call asks for is the caller's policy; the row stride the kernels see is cap.
struct RowStage {
    DeviceBuffer<double> buf;
    int cap = 0;            // samples per row
    size_t rows = 0;

    // rows of at least n samples.  A request above the capacity replaces the allocation (contents are not kept), after the stream
    // has passed whatever reads the one that goes: an empty stage waits for nothing.  CPQ_ERR_OOM leaves the buffer empty and the
    // capacity 0.
    int ensure(std::string* sink, hipStream_t stream, int n)
    {
        if (n <= cap) return CPQ_OK;
        if (buf) CPQ_OBJ_HIP(sink, hipStreamSynchronize(stream));
        if (grow(nullptr, buf, cap, n, rows, "row buffer") != CPQ_OK)
            return failTo(sink, CPQ_ERR_OOM, "row buffer of %d samples could not be allocated", n);
        return CPQ_OK;
    }
    // n samples of every row from src (rows at `stride` samples) into the stage, or from the stage to dst, enqueued on stream
    int upload(std::string* sink, const double* src, int64_t stride, int n, hipMemcpyKind kind, hipStream_t stream)
    {
        CPQ_OBJ_HIP(sink, hipMemcpy2DAsync(buf, pitch(cap), src, pitch(stride), pitch(n), rows, kind, stream));
        return CPQ_OK;
    }
    int download(std::string* sink, double* dst, int64_t stride, int n, hipMemcpyKind kind, hipStream_t stream) const
    {
        CPQ_OBJ_HIP(sink, hipMemcpy2DAsync(dst, pitch(stride), buf, pitch(cap), pitch(n), rows, kind, stream));
        return CPQ_OK;
    }
    static size_t pitch(int64_t samples) { return (size_t)samples * sizeof(double); }
};

// The refusals that every call on rows in and rows out makes first, in their documented order: null, n_samples, strides, and for
// device rows the 16-byte alignment.  What follows (partial overlap, with kRowsOverlap) is the caller's: it knows its row count.
inline int checkRowPair(std::string* sink, const double* in, int64_t inStride, const double* out, int64_t outStride, int n, int maxN, bool deviceRows)
{
    if (!in || !out) return failTo(sink, CPQ_ERR_INVALID_ARG, "null buffer");
    if (n < 1 || n > maxN) return failTo(sink, CPQ_ERR_INVALID_ARG, "n_samples=%d outside 1..%d", n, maxN);
    if (inStride < n || outStride < n)
        return failTo(sink, CPQ_ERR_INVALID_ARG, "row strides %lld and %lld, rows of %d", (long long)inStride, (long long)outStride, n);
    if (deviceRows && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u))
        return failTo(sink, CPQ_ERR_INVALID_ARG, "buffers must be 16-byte aligned");
    return CPQ_OK;
}
constexpr const char* kRowsOverlap = "input and output rows overlap in part: in place takes the same pointer and stride";

inline int setStream(std::string* sink, hipStream_t& stream, void* next)
{
    CPQ_OBJ_HIP(sink, hipStreamSynchronize(stream));
    stream = (hipStream_t)next;
    return CPQ_OK;
}

// f's own status, or CPQ_ERR_OOM where it threw (the host containers of these objects throw nothing but std::bad_alloc)
template <typename F>
int guardAlloc(std::string* sink, F&& f)
{
    try {
        return f();
    } catch (const std::exception&) {
        return failTo(sink, CPQ_ERR_OOM, "host allocation failed");
    }
}

}  // namespace cpqi
