// Host-only driver for convopeq_amd/csrc/object_support.hpp (tests/test_object_support_cpu.py): no kernel, nothing launched.
// Without a device every runtime call fails (hipErrorNoDevice), which is the path the first half checks: what the scaffold
// reports, where it reports it, and what it leaves behind.  The only impossible request is one the runtime refuses without touching
// device memory (2^57 samples = 2^60 bytes).  The second half needs calls that succeed: it runs where a device is visible and is
// printed as skipped elsewhere.
#include "object_support.hpp"

#include <cstring>
#include <new>
#include <vector>

static std::string g_global;        // what cpq_last_error(NULL) would answer

namespace cpqi {
int fail(cpq_engine*, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_global = buf;
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

static int syncNull(std::string* sink)
{
    CPQ_OBJ_HIP(sink, hipStreamSynchronize(nullptr));
    return CPQ_OK;
}

static uint64_t bits(double v)
{
    uint64_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

int main()
{
    int nDev = 0;
    const bool haveDevice = hipGetDeviceCount(&nDev) == hipSuccess && nDev > 0;
    (void)hipGetLastError();
    std::printf("devices visible: %d\n", haveDevice ? nDev : 0);
    // what "no error left pending" can mean: see device_buffers_check.cpp
    const hipError_t quiet = haveDevice ? hipSuccess : hipErrorNoDevice;

    {   // failTo: the sink or the global, never both; 512 bytes
        std::string sink = "old";
        g_global = "untouched";
        CHECK(failTo(&sink, CPQ_ERR_INVALID_ARG, "%d samples outside 0..%d", 7, 5) == CPQ_ERR_INVALID_ARG);
        CHECK(sink == "7 samples outside 0..5" && g_global == "untouched");
        CHECK(failTo(nullptr, CPQ_ERR_UNSUPPORTED, "say %s", "which") == CPQ_ERR_UNSUPPORTED);
        CHECK(g_global == "say which" && sink == "7 samples outside 0..5");
        const std::string big(2000, 'x');
        CHECK(failTo(&sink, CPQ_ERR_OOM, "%s", big.c_str()) == CPQ_ERR_OOM);
        CHECK(sink.size() == 511 && sink == std::string(511, 'x'));
        CHECK(failTo(nullptr, CPQ_ERR_OOM, "%s", big.c_str()) == CPQ_ERR_OOM);
        CHECK(g_global.size() == 511 && g_global == std::string(511, 'x'));
    }

    {   // guardAlloc: the callable's own status, or CPQ_ERR_OOM for what it threw
        std::string sink;
        CHECK(guardAlloc(&sink, [] { return (int)CPQ_OK; }) == CPQ_OK && sink.empty());
        CHECK(guardAlloc(&sink, [] { return (int)CPQ_ERR_NOT_READY; }) == CPQ_ERR_NOT_READY && sink.empty());
        CHECK(guardAlloc(&sink, []() -> int { throw std::bad_alloc(); }) == CPQ_ERR_OOM);
        CHECK(sink == "host allocation failed");
        g_global.clear();
        CHECK(guardAlloc(nullptr, []() -> int { throw std::bad_alloc(); }) == CPQ_ERR_OOM && g_global == "host allocation failed");
    }

    {   // an impossible stage: CPQ_ERR_OOM, nothing held, no error pending; an empty stage waits for no stream on the way
        std::string sink;
        RowStage stage;
        stage.rows = (size_t)1 << 40;
        CHECK(stage.ensure(&sink, nullptr, 1 << 17) == CPQ_ERR_OOM);
        CHECK(!stage.buf && stage.buf.count() == 0 && stage.cap == 0);
        CHECK(sink == "row buffer of 131072 samples could not be allocated");
        CHECK(stage.ensure(&sink, nullptr, 0) == CPQ_OK && !stage.buf);
        CHECK(hipGetLastError() == quiet);
    }

    if (!haveDevice) {
        // every runtime call fails
        std::string sink;
        CHECK(syncNull(&sink) == CPQ_ERR_DEVICE);
        CHECK(sink.find("hipStreamSynchronize(nullptr) failed: ") == 0 && sink.size() > std::strlen("hipStreamSynchronize(nullptr) failed: "));
        g_global.clear();
        CHECK(syncNull(nullptr) == CPQ_ERR_DEVICE && g_global == sink);
        {
            TimingEvents<3> ev;
            sink.clear();
            CHECK(ev.create(&sink) == CPQ_ERR_DEVICE && sink.find("hipEventCreate(&e) failed: ") == 0);
            CHECK(!ev[0] && !ev[1] && !ev[2]);
            CHECK(ev.elapsed(0, 1) == -1.0 && ev.elapsed(1, 2) == -1.0);
        }       // destructs with nothing to destroy
        hipStream_t stream = nullptr;
        int marker = 0;
        sink.clear();
        CHECK(setStream(&sink, stream, &marker) == CPQ_ERR_DEVICE && stream == nullptr && !sink.empty());     // the old stream stays
        CHECK(hipGetLastError() == quiet);
        std::printf("skipped: no device visible -- stage growth, the strided round trip, elapsed time of recorded events, setStream\n");
    } else {
        std::string sink;
        CHECK(syncNull(&sink) == CPQ_OK && sink.empty());
        {   // growth: only a request above the capacity replaces the allocation.  The old one is freed before the new one is
            // made, so the runtime may hand the same address back: "replaced" is read from the size of the allocation behind the
            // pointer (rows of 512 KB, so that no rounding of the runtime hides 5 against 9 of them), and the move is printed.
            auto allocated = [](const void* p) {
                hipDeviceptr_t base = nullptr;
                size_t size = 0;
                return hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess ? size : (size_t)0;
            };
            const size_t rows = (size_t)1 << 16, row = rows * sizeof(double);
            RowStage stage;
            stage.rows = rows;
            CHECK(stage.ensure(&sink, nullptr, 5) == CPQ_OK && stage.cap == 5 && stage.buf.count() == 5 * rows);
            double* const was = stage.buf;
            CHECK(allocated(was) >= 5 * row && allocated(was) < 9 * row);
            CHECK(stage.ensure(&sink, nullptr, 4) == CPQ_OK && stage.cap == 5 && stage.buf.get() == was);
            CHECK(stage.ensure(&sink, nullptr, 9) == CPQ_OK && stage.cap == 9 && stage.buf.count() == 9 * rows);
            CHECK(stage.buf.get() != nullptr && allocated(stage.buf) >= 9 * row);
            std::printf("growth 5 -> 9: the pointer %s\n", stage.buf.get() != was ? "moved" : "is the freed one, handed back");
            CHECK(sink.empty());
        }
        {   // [3][5] with host strides 7 up and 9 down through a stage of capacity 6: every sample to the bit, every padding intact
            const double kPad = -777.25;
            RowStage stage;
            stage.rows = 3;
            CHECK(stage.ensure(&sink, nullptr, 6) == CPQ_OK);
            CHECK(hipMemset(stage.buf, 0xff, 18 * sizeof(double)) == hipSuccess);
            std::vector<double> up(3 * 7, kPad), down(3 * 9, kPad);
            for (int r = 0; r < 3; ++r)
                for (int i = 0; i < 5; ++i) up[(size_t)(r * 7 + i)] = (r + 1) * 1.0e-3 / (i + 3) - (i == 2 ? 0.0 : 1.0e300 * r);
            up[0] = -0.0;
            CHECK(stage.upload(&sink, up.data(), 7, 5, hipMemcpyHostToDevice, nullptr) == CPQ_OK);
            CHECK(stage.download(&sink, down.data(), 9, 5, hipMemcpyDeviceToHost, nullptr) == CPQ_OK);
            CHECK(hipStreamSynchronize(nullptr) == hipSuccess);
            bool same = true, padded = true;
            for (int r = 0; r < 3; ++r) {
                for (int i = 0; i < 5; ++i) same = same && bits(down[(size_t)(r * 9 + i)]) == bits(up[(size_t)(r * 7 + i)]);
                for (int i = 5; i < 9; ++i) padded = padded && bits(down[(size_t)(r * 9 + i)]) == bits(kPad);
                for (int i = 5; i < 7; ++i) padded = padded && bits(up[(size_t)(r * 7 + i)]) == bits(kPad);
            }
            CHECK(same);
            CHECK(padded);
            // the stage's own padding (column 5 of every row) was not written: still the 0xff pattern
            std::vector<double> all(18);
            CHECK(hipMemcpy(all.data(), stage.buf, 18 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
            CHECK(bits(all[5]) == ~(uint64_t)0 && bits(all[11]) == ~(uint64_t)0 && bits(all[17]) == ~(uint64_t)0);
            CHECK(bits(all[6]) == bits(up[7]) && sink.empty());
        }
        {   // events: created, recorded, passed
            TimingEvents<2> ev;
            CHECK(ev.elapsed(0, 1) == -1.0);            // not created yet
            CHECK(ev.create(&sink) == CPQ_OK && ev[0] && ev[1]);
            CHECK(hipEventRecord(ev[0], nullptr) == hipSuccess && hipEventRecord(ev[1], nullptr) == hipSuccess);
            CHECK(hipStreamSynchronize(nullptr) == hipSuccess);
            CHECK(ev.elapsed(0, 1) >= 0.0);
        }
        {   // setStream: the old stream synchronised, then replaced
            hipStream_t made = nullptr, stream = nullptr;
            CHECK(hipStreamCreate(&made) == hipSuccess);
            CHECK(setStream(&sink, stream, made) == CPQ_OK && stream == made);
            CHECK(setStream(&sink, stream, nullptr) == CPQ_OK && stream == nullptr);
            CHECK(hipStreamDestroy(made) == hipSuccess);
        }
        CHECK(hipGetLastError() == quiet && sink.empty());
    }

    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
