// engine_resample.cpp -- cpq_ir_resample / cpq_ir_resample_batch: ConvolverProcessorInternal::resampleIR
// (src/convolver/ConvolverProcessor.ResampleAndFallback.cpp:18-108) for many IRs at once.  No engine object: a loader stage that
// owns its device buffers for the length of the call.  The filter, the call checks, the host path and the tail trim are
// resample_design.cpp's; the kernel is resample_kernels.hip.  Per source rate of the batch:
//   taps  [L][T]          the filter of (source rate, target rate)
//   x     rows back to back, every channel of every IR of that rate one row
//   y     the rows' ceil(n L / M) outputs back to back
//   rows, tiles           ResampleRow per row, ResampleTile per workgroup
// one upload, one launch, one download; the trim is host work on the downloaded rows.
#include "engine_internal.hpp"

#include "object_support.hpp"

namespace {

thread_local double g_lastKernelMs = -1.0;

// the IRs `members` of the batch share a source rate and the design d: their rows through one launch, then the trim into out[i]
int runGroup(const cpq_ir_buffer* const* in, const std::vector<int>& members, const cpq::ResampleDesign& d, double targetRate,
             cpq_ir_buffer* out, double& kernelMs)
{
    const int tile = cpq::resampleTile(d.L, d.M);
    std::vector<cpq::ResampleRow> rows;
    std::vector<cpq::ResampleTile> tiles;
    long long inTotal = 0, outTotal = 0;
    for (int i : members) {
        const int n = in[i]->n_samples, nOut = (int)cpq::resampleOutLen(n, d.L, d.M);
        for (int ch = 0; ch < in[i]->n_channels; ++ch) {
            const int r = (int)rows.size();
            rows.push_back(cpq::ResampleRow{ inTotal, outTotal, n, nOut });
            for (long long j0 = 0; j0 < nOut; j0 += tile) tiles.push_back(cpq::ResampleTile{ r, (int)j0 });
            inTotal += n;
            outTotal += nOut;
        }
    }
    if (tiles.size() > 0x7fffffffu) return cpqi::fail(nullptr, CPQ_ERR_UNSUPPORTED, "more than 2^31 - 1 tiles in one launch");

    cpqi::DeviceBuffer<double> taps, x, y;
    cpqi::DeviceBuffer<cpq::ResampleRow> dRows;
    cpqi::DeviceBuffer<cpq::ResampleTile> dTiles;
    CPQ_TRY(cpqi::allocAll(nullptr, { { taps, d.taps.size() }, { x, (size_t)inTotal }, { y, (size_t)outTotal }, { dRows, rows.size() },
                                      { dTiles, tiles.size() } },
                           "resample buffers for %lld input and %lld output samples could not be allocated", inTotal, outTotal));
    cpqi::TimingEvents<2> t;
    CPQ_TRY(t.create(nullptr));
    CPQ_OBJ_HIP(nullptr, hipMemcpy(taps, d.taps.data(), d.taps.size() * sizeof(double), hipMemcpyHostToDevice));
    CPQ_OBJ_HIP(nullptr, hipMemcpy(dRows, rows.data(), rows.size() * sizeof(rows[0]), hipMemcpyHostToDevice));
    CPQ_OBJ_HIP(nullptr, hipMemcpy(dTiles, tiles.data(), tiles.size() * sizeof(tiles[0]), hipMemcpyHostToDevice));
    size_t r = 0;
    for (int i : members) {     // a buffer's channels are contiguous: one copy per IR
        const size_t count = (size_t)in[i]->n_channels * (size_t)in[i]->n_samples;
        CPQ_OBJ_HIP(nullptr, hipMemcpy(x.get() + rows[r].inOff, in[i]->data, count * sizeof(double), hipMemcpyHostToDevice));
        r += (size_t)in[i]->n_channels;
    }
    CPQ_OBJ_HIP(nullptr, hipEventRecord(t[0], nullptr));
    cpq::launch_ir_resample(nullptr, taps, d.L, d.M, d.T, x, y, dRows, dTiles, (int)tiles.size());
    CPQ_OBJ_HIP(nullptr, hipGetLastError());
    CPQ_OBJ_HIP(nullptr, hipEventRecord(t[1], nullptr));
    std::vector<double> host((size_t)outTotal);
    CPQ_OBJ_HIP(nullptr, hipMemcpy(host.data(), y, host.size() * sizeof(double), hipMemcpyDeviceToHost));
    float ms = 0.0f;
    CPQ_OBJ_HIP(nullptr, hipEventElapsedTime(&ms, t[0], t[1]));
    kernelMs += ms;

    r = 0;
    for (int i : members) {
        const int rc = cpq::resampleFinish(host.data() + rows[r].outOff, in[i]->n_channels, rows[r].nOut, targetRate, &out[i]);
        if (rc != CPQ_OK) return cpqi::fail(nullptr, rc, "host allocation of a converted IR failed");
        r += (size_t)in[i]->n_channels;
    }
    return CPQ_OK;
}

int resampleBatch(const cpq_ir_buffer* const* in, int n, double targetRate, int phase, cpq_ir_buffer* out)
{
    // every refusal first: nothing is allocated for a batch that holds one
    std::vector<char> copy((size_t)n, 0);
    std::vector<double> rates;                  // the source rates that need a launch, in order of appearance
    std::vector<cpq::ResampleDesign> designs;
    std::vector<std::vector<int>> members;
    for (int i = 0; i < n; ++i) {
        size_t g = 0;           // a source rate seen before brings its design along
        while (in[i] && g < rates.size() && rates[g] != in[i]->sample_rate) ++g;
        const bool known = in[i] && g < rates.size();
        cpq::ResampleDesign fresh;
        bool isCopy = false;
        const char* why = "";
        const int rc = cpq::resampleCheck(in[i], targetRate, phase, isCopy, known ? designs[g] : fresh, &why, known);
        if (rc != CPQ_OK) return cpqi::fail(nullptr, rc, "IR %d: %s", i, why);
        copy[i] = isCopy;
        if (isCopy) continue;
        if (!known) {
            g = rates.size();
            rates.push_back(in[i]->sample_rate);
            designs.push_back(std::move(fresh));
            members.emplace_back();
        }
        members[g].push_back(i);
    }
    if (!rates.empty()) CPQ_TRY(cpqi::checkCurrentDevice());
    double kernelMs = 0.0;
    for (size_t g = 0; g < rates.size(); ++g) CPQ_TRY(runGroup(in, members[g], designs[g], targetRate, out, kernelMs));
    for (int i = 0; i < n; ++i)
        if (copy[i] && cpq::resampleCopy(in[i], &out[i]) != CPQ_OK) return cpqi::fail(nullptr, CPQ_ERR_OOM, "host allocation of a copied IR failed");
    g_lastKernelMs = rates.empty() ? -1.0 : kernelMs;
    return CPQ_OK;
}

}  // namespace

extern "C" {

int32_t cpq_ir_resample_batch(const cpq_ir_buffer* const* in, int32_t n, double target_rate, int32_t phase, cpq_ir_buffer* out)
{
    if (!out || n < 0) return cpqi::fail(nullptr, CPQ_ERR_INVALID_ARG, "null output or a negative count");
    for (int i = 0; i < n; ++i) std::memset(&out[i], 0, sizeof(out[i]));
    if (n > 0 && !in) return cpqi::fail(nullptr, CPQ_ERR_INVALID_ARG, "null buffer list");
    const int rc = cpqi::guardAlloc(nullptr, [&] { return resampleBatch(in, n, target_rate, phase, out); });
    if (rc != CPQ_OK)
        for (int i = 0; i < n; ++i) {
            cpq_ir_buffer_free(&out[i]);
            std::memset(&out[i], 0, sizeof(out[i]));
        }
    return rc;
}

int32_t cpq_ir_resample(const cpq_ir_buffer* in, double target_rate, int32_t phase, cpq_ir_buffer* out)
{
    return cpq_ir_resample_batch(&in, 1, target_rate, phase, out);
}

double cpq_ir_resample_last_kernel_ms(void) { return g_lastKernelMs; }

}  // extern "C"
