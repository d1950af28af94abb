// device_buffers.hpp -- ownership of the engine's device (and pinned host) allocations.  The only place of the library that
// calls hipMalloc / hipHostMalloc / hipFree / hipHostFree.
//
//   DeviceBuffer<T>   move-only owner of one allocation of count() elements; converts to T* where a pointer is passed on
//   allocAll          fills a group of empty buffers, or leaves every one of them empty and reports CPQ_ERR_OOM
//   grow              the capacity-tracked buffers: a larger request replaces the allocation, contents are not kept
//
// A failed allocation leaves nothing behind: the members are empty and the HIP error is cleared (the runtime neither nulls the
// caller's pointer nor forgets the error by itself).  Needs only the HIP runtime and cpqi::fail.
#pragma once

#include "convopeq_mi355x.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <initializer_list>

struct cpq_engine;

namespace cpqi {

int fail(cpq_engine* e, int code, const char* fmt, ...);

// the untyped allocation behind DeviceBuffer<T>: what allocAll handles
class RawBuffer {
public:
    RawBuffer() = default;
    RawBuffer(const RawBuffer&) = delete;
    RawBuffer& operator=(const RawBuffer&) = delete;
    ~RawBuffer() { reset(); }

    void reset()
    {
        if (p_) (void)(pinned_ ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        bytes_ = 0;
    }
    // replaces what the buffer holds; on failure the buffer is empty and no HIP error is left pending
    bool allocBytes(size_t bytes, bool zero = false)
    {
        reset();
        void* p = nullptr;
        if ((pinned_ ? hipHostMalloc(&p, bytes) : hipMalloc(&p, bytes)) != hipSuccess) { (void)hipGetLastError(); return false; }
        p_ = p;
        bytes_ = bytes;
        if (zero && hipMemset(p_, 0, bytes) != hipSuccess) { (void)hipGetLastError(); reset(); return false; }
        return true;
    }
    explicit operator bool() const { return p_ != nullptr; }

protected:
    explicit RawBuffer(bool pinned) : pinned_(pinned) {}
    void take(RawBuffer& o)
    {
        p_ = o.p_; bytes_ = o.bytes_;
        o.p_ = nullptr; o.bytes_ = 0;
    }
    void* p_ = nullptr;
    size_t bytes_ = 0;
    bool pinned_ = false;
};

template <typename T, bool Pinned = false>
class DeviceBuffer : public RawBuffer {
public:
    DeviceBuffer() : RawBuffer(Pinned) {}
    DeviceBuffer(DeviceBuffer&& o) noexcept : RawBuffer(Pinned) { take(o); }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept
    {
        if (this != &o) { reset(); take(o); }
        return *this;
    }
    bool alloc(size_t count, bool zero = false) { return allocBytes(count * sizeof(T), zero); }
    T* get() const { return static_cast<T*>(p_); }
    operator T*() const { return get(); }
    size_t count() const { return bytes_ / sizeof(T); }
};

template <typename T>
using PinnedBuffer = DeviceBuffer<T, true>;

struct AllocItem {
    template <typename T, bool Pinned>
    AllocItem(DeviceBuffer<T, Pinned>& b, size_t count, bool zeroIt = false) : buf(&b), bytes(count * sizeof(T)), zero(zeroIt) {}
    RawBuffer* buf;
    size_t bytes;
    bool zero;
};

// All or nothing: every buffer of the group filled (and zeroed where asked), or every one of them empty and CPQ_ERR_OOM with the
// message.  The group must be empty: a group that holds a buffer is refused (CPQ_ERR_INVALID_ARG) and stays as it is -- a feature
// is allocated once, and its "is allocated" test is any member of the group.
template <typename... Args>
int allocAll(cpq_engine* e, std::initializer_list<AllocItem> items, const char* fmt, Args... args)
{
    for (const AllocItem& it : items)
        if (*it.buf) return fail(e, CPQ_ERR_INVALID_ARG, "buffer group allocated twice");
    for (const AllocItem& it : items)
        if (!it.buf->allocBytes(it.bytes, it.zero)) {
            for (const AllocItem& u : items) u.buf->reset();
            (void)hipGetLastError();
            return fail(e, CPQ_ERR_OOM, fmt, args...);
        }
    return CPQ_OK;
}

// buf holds perUnit * cap elements; a need above cap frees it and allocates perUnit * need (contents are not kept).  After a
// failure the buffer is empty and cap is 0.
template <typename T, typename... Args>
int grow(cpq_engine* e, DeviceBuffer<T>& buf, int& cap, int need, size_t perUnit, const char* fmt, Args... args)
{
    if (need <= cap) return CPQ_OK;
    buf.reset();
    cap = 0;
    if (!buf.alloc(perUnit * (size_t)need)) return fail(e, CPQ_ERR_OOM, fmt, args...);
    cap = need;
    return CPQ_OK;
}

}  // namespace cpqi
