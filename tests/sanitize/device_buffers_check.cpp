// Host-only driver for convopeq_amd/csrc/device_buffers.hpp (tests/test_device_buffers_cpu.py): no kernel, nothing launched.
// The only failing request is an impossible one (2^60 bytes), which the runtime refuses without touching device memory -- with no
// device at all every request fails (hipErrorNoDevice), which exercises the same path.  Nothing here tries to exhaust memory.
#include "device_buffers.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

struct cpq_engine { std::string lastError; };

namespace cpqi {
int fail(cpq_engine* e, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (e) e->lastError = buf;
    return code;
}
}  // namespace cpqi

using namespace cpqi;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

constexpr size_t kImpossible = (size_t)1 << 60;     // bytes

int main()
{
    cpq_engine eng;
    cpq_engine* e = &eng;
    int nDev = 0;
    const bool haveDevice = hipGetDeviceCount(&nDev) == hipSuccess && nDev > 0;
    (void)hipGetLastError();
    std::printf("devices visible: %d\n", haveDevice ? nDev : 0);
    // "No error left pending": hipGetLastError() == hipSuccess wherever the runtime has a device.  Without one the runtime cannot
    // initialise and EVERY call reports hipErrorNoDevice, hipGetLastError() itself included, however often it is called (seen
    // with ROCm 7: two calls in a row both return 100): nothing an owner does can make it hipSuccess there, so the driver checks
    // that it reports that state and nothing else.
    const hipError_t quiet = haveDevice ? hipSuccess : hipErrorNoDevice;
    CHECK(hipGetLastError() == quiet);

    {   // never filled, and moved from: nothing to free, nothing reported
        DeviceBuffer<double> never;
        PinnedBuffer<int> neverPinned;
        DeviceBuffer<double> from;
        DeviceBuffer<double> to(std::move(from));
        to = std::move(never);
        CHECK(!never && !neverPinned && !from && !to);
        CHECK(to.get() == nullptr && to.count() == 0 && static_cast<double*>(to) == nullptr);
    }
    CHECK(hipGetLastError() == quiet);

    {   // a group whose SECOND member cannot be had: failure reported, every member empty (the first included), no error pending
        DeviceBuffer<int> first;
        DeviceBuffer<char> second;
        DeviceBuffer<double> third;
        PinnedBuffer<int> fourth;
        const int rc = allocAll(e, { { first, 16, true }, { second, kImpossible }, { third, 16 }, { fourth, 16 } },
                                "group of %d could not be allocated", 4);
        CHECK(rc == CPQ_ERR_OOM);
        CHECK(eng.lastError == "group of 4 could not be allocated");
        CHECK(!first && !second && !third && !fourth);
        CHECK(first.get() == nullptr && first.count() == 0 && second.count() == 0);
        CHECK(hipGetLastError() == quiet);
    }

    {   // grow after a failure: capacity 0, buffer empty, no error pending
        DeviceBuffer<double> gains;
        int cap = 0;
        const int rc = grow(e, gains, cap, 8, kImpossible / (8 * sizeof(double)), "gains could not be allocated");
        CHECK(rc == CPQ_ERR_OOM && cap == 0 && !gains && gains.count() == 0);
        CHECK(eng.lastError == "gains could not be allocated");
        CHECK(hipGetLastError() == quiet);
    }

    if (!haveDevice) {
        std::printf("skipped: no device visible -- allocations that succeed, zeroing, the refused second allocAll, grow on a filled buffer\n");
    } else {
        DeviceBuffer<int> flags;
        DeviceBuffer<double> state;
        PinnedBuffer<int> host;
        int rc = allocAll(e, { { flags, 64, true }, { state, 33 }, { host, 64, true } }, "small group could not be allocated");
        CHECK(rc == CPQ_OK && flags && state && host);
        CHECK(flags.count() == 64 && state.count() == 33 && host.count() == 64);
        std::vector<int> back(64, -1);
        CHECK(hipMemcpy(back.data(), flags, sizeof(int) * 64, hipMemcpyDeviceToHost) == hipSuccess);
        bool zero = true;
        for (int i = 0; i < 64; ++i) zero = zero && back[(size_t)i] == 0 && host[i] == 0;
        CHECK(zero);
        // a filled group is refused and stays as it is
        int* const flagsWas = flags;
        double* const stateWas = state;
        rc = allocAll(e, { { flags, 8 }, { state, 8 } }, "small group could not be allocated");
        CHECK(rc == CPQ_ERR_INVALID_ARG && flags.get() == flagsWas && state.get() == stateWas && flags.count() == 64);
        // ... also when only one member is filled: the empty one stays empty
        DeviceBuffer<double> extra;
        rc = allocAll(e, { { extra, 8 }, { state, 8 } }, "small group could not be allocated");
        CHECK(rc == CPQ_ERR_INVALID_ARG && !extra && state.get() == stateWas);
        // move: the pointer changes hands, the source is empty
        DeviceBuffer<double> moved;
        moved = std::move(state);
        CHECK(!state && moved.get() == stateWas && moved.count() == 33);
        // grow: larger requests replace the buffer, smaller ones leave it; an impossible one leaves nothing
        DeviceBuffer<double> gains;
        int cap = 0;
        CHECK(grow(e, gains, cap, 4, 3, "gains") == CPQ_OK && cap == 4 && gains.count() == 12);
        double* const gainsWas = gains;
        CHECK(grow(e, gains, cap, 2, 3, "gains") == CPQ_OK && cap == 4 && gains.get() == gainsWas);
        CHECK(grow(e, gains, cap, 8, kImpossible / (8 * sizeof(double)), "gains") == CPQ_ERR_OOM && cap == 0 && !gains);
        CHECK(hipGetLastError() == quiet);
        // the same impossible group with a device present: the first member was really allocated, and is given back
        DeviceBuffer<int> first;
        DeviceBuffer<char> second;
        rc = allocAll(e, { { first, 16, true }, { second, kImpossible } }, "group could not be allocated");
        CHECK(rc == CPQ_ERR_OOM && !first && !second);
        CHECK(hipGetLastError() == quiet);
    }

    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
