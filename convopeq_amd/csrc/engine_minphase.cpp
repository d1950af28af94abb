// engine_minphase.cpp -- cpq_ir_minimum_phase / _batch and cpq_ir_prepare_batch: ConvolverProcessorInternal::convertToMinimumPhase
// (src/convolver/ConvolverProcessor.ResampleAndFallback.cpp:333-469) for many IRs at once.  No engine object: a loader stage that
// owns its device buffers for the length of the call.  What runs is minphase_plan.hpp's: the rows (one per channel of an IR)
// grouped by FFT size, each group cut into chunks under the workspace cap, each chunk a list of launches of
// minphase_kernels.hip.  Per chunk:
//   x, y    the rows' samples back to back, in and out
//   z       [rows][N] complex scratch (FFT sizes above the LDS bound only)
//   rows, flags     MinphaseRow and the "not finite" word per row
// one upload, the launches, one download (the rows are gathered into and scattered from one host buffer).  The twiddle tables are
// uploaded once per call (the 4096th roots) and once per FFT size (the two levels of the N-th roots); they are not counted
// against the cap (at most 160 KB).
#include "engine_internal.hpp"
#include "ir_ingest.hpp"
#include "object_support.hpp"

namespace {

thread_local double g_lastKernelMs = -1.0;

bool validBuffer(const cpq_ir_buffer* b) { return b && b->data && b->n_channels > 0 && b->n_samples > 0; }

const double2* c2(const double* p) { return reinterpret_cast<const double2*>(p); }

// one chunk of a group: its rows up, the plan's launches, the rows down into out[.]; marked[i] is set where a row of IR i was flagged
int runChunk(const cpq_ir_buffer* const* in, const cpq::MinphaseGroup& g, const cpq::MinphaseChunk& c, cpq::MinphaseTables tables,
             cpq_ir_buffer* out, std::vector<char>& marked, const cpqi::TimingEvents<2>& t, double& kernelMs)
{
    std::vector<cpq::MinphaseRow> rows(c.count);
    long long off = 0;
    for (size_t r = 0; r < c.count; ++r) {
        rows[r] = cpq::MinphaseRow{ off, g.rows[c.first + r].n, 0 };
        off += g.rows[c.first + r].n;
    }
    const bool big = g.log2n1 > 0;
    cpqi::DeviceBuffer<double> x, y;
    cpqi::DeviceBuffer<double2> z;
    cpqi::DeviceBuffer<cpq::MinphaseRow> dRows;
    cpqi::DeviceBuffer<int> flags;
    const size_t nZ = big ? c.count << g.log2n : 1;
    CPQ_TRY(cpqi::allocAll(nullptr, { { x, (size_t)c.samples }, { y, (size_t)c.samples }, { z, nZ }, { dRows, c.count }, { flags, c.count } },
                           "minimum-phase buffers for %zu rows of %lld points could not be allocated", c.count, 1LL << g.log2n));
    CPQ_OBJ_HIP(nullptr, hipMemcpy(dRows, rows.data(), rows.size() * sizeof(rows[0]), hipMemcpyHostToDevice));
    CPQ_OBJ_HIP(nullptr, hipMemset(flags, 0, c.count * sizeof(int)));
    std::vector<double> host((size_t)c.samples);          // the rows back to back: one copy each way
    for (size_t r = 0; r < c.count; ++r) {
        const cpq::MinphaseRowRef& ref = g.rows[c.first + r];
        std::memcpy(host.data() + rows[r].off, in[ref.ir]->data + (size_t)ref.ch * (size_t)ref.n, (size_t)ref.n * sizeof(double));
    }
    CPQ_OBJ_HIP(nullptr, hipMemcpy(x, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
    CPQ_OBJ_HIP(nullptr, hipEventRecord(t[0], nullptr));
    for (const cpq::MinphaseLaunch& l : cpq::minphaseLaunches(g, (long long)c.count)) {
        if (l.kernel == cpq::kMinphaseKSmall) cpq::launch_minphase_small(nullptr, x, y, dRows, flags, tables, g.log2n, (long long)c.count);
        else if (l.kernel == cpq::kMinphaseKCols)
            cpq::launch_cfft_cols(nullptr, l.op, z, x, y, dRows, flags, tables, g.log2n1, g.log2n2, (long long)c.count);
        else cpq::launch_cfft_rows(nullptr, l.op, z, flags, tables, g.log2n1, g.log2n2, (long long)c.count, 1.0);
        CPQ_OBJ_HIP(nullptr, hipGetLastError());
    }
    CPQ_OBJ_HIP(nullptr, hipEventRecord(t[1], nullptr));
    std::vector<int> hostFlags(c.count);
    CPQ_OBJ_HIP(nullptr, hipMemcpy(host.data(), y, host.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < c.count; ++r) {
        const cpq::MinphaseRowRef& ref = g.rows[c.first + r];
        std::memcpy(out[ref.ir].data + (size_t)ref.ch * (size_t)ref.n, host.data() + rows[r].off, (size_t)ref.n * sizeof(double));
    }
    CPQ_OBJ_HIP(nullptr, hipMemcpy(hostFlags.data(), flags, c.count * sizeof(int), hipMemcpyDeviceToHost));
    float ms = 0.0f;
    CPQ_OBJ_HIP(nullptr, hipEventElapsedTime(&ms, t[0], t[1]));
    kernelMs += ms;
    for (size_t r = 0; r < c.count; ++r)
        if (hostFlags[r]) marked[(size_t)g.rows[c.first + r].ir] = 1;
    return CPQ_OK;
}

int minphaseBatch(const cpq_ir_buffer* const* in, int n, long long workspace, cpq_ir_buffer* out, int32_t* status)
{
    // every refusal first: nothing is allocated for a call that holds one
    std::vector<int> channels((size_t)n), samples((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!validBuffer(in[i])) return cpqi::fail(nullptr, CPQ_ERR_INVALID_ARG, "IR %d: null or empty buffer", i);
        channels[(size_t)i] = in[i]->n_channels;
        samples[(size_t)i] = in[i]->n_samples;
    }
    std::vector<char> refused;
    const std::vector<cpq::MinphaseGroup> groups = cpq::minphaseGroups(channels.data(), samples.data(), n, refused);
    const long long cap = workspace > 0 ? workspace : cpq::kMinphaseDefaultWorkspace;
    std::vector<std::vector<cpq::MinphaseChunk>> chunks(groups.size());
    for (size_t g = 0; g < groups.size(); ++g)
        if (!cpq::minphaseChunks(groups[g], cap, chunks[g]))
            return cpqi::fail(nullptr, CPQ_ERR_INVALID_ARG, "workspace_bytes %lld is below the %lld bytes one row of %lld points needs", cap,
                              cpq::minphaseRowNeed(groups[g]), 1LL << groups[g].log2n);
    for (int i = 0; i < n; ++i) status[i] = refused[(size_t)i] ? CPQ_ERR_UNSUPPORTED : CPQ_OK;
    if (groups.empty()) return CPQ_OK;
    CPQ_TRY(cpqi::checkCurrentDevice());

    for (int i = 0; i < n; ++i) {
        if (refused[(size_t)i]) continue;
        out[i].n_channels = in[i]->n_channels;
        out[i].n_samples = in[i]->n_samples;
        out[i].sample_rate = in[i]->sample_rate;
        out[i].data = static_cast<double*>(std::calloc((size_t)in[i]->n_channels * (size_t)in[i]->n_samples, sizeof(double)));
        if (!out[i].data) return cpqi::fail(nullptr, CPQ_ERR_OOM, "IR %d: host allocation of the converted IR failed", i);
    }

    cpqi::TimingEvents<2> t;
    CPQ_TRY(t.create(nullptr));
    const std::vector<double> roots = cpq::minphaseStageRoots();
    cpqi::DeviceBuffer<double> dRoots;
    CPQ_TRY(cpqi::allocAll(nullptr, { { dRoots, roots.size() } }, "the twiddle table could not be allocated"));
    CPQ_OBJ_HIP(nullptr, hipMemcpy(dRoots, roots.data(), roots.size() * sizeof(double), hipMemcpyHostToDevice));
    std::vector<char> marked((size_t)n, 0);
    double kernelMs = 0.0;
    for (size_t g = 0; g < groups.size(); ++g) {
        std::vector<double> hi, lo;
        cpq::minphaseSplitRoots(groups[g].log2n, hi, lo);
        cpqi::DeviceBuffer<double> dHi, dLo;
        CPQ_TRY(cpqi::allocAll(nullptr, { { dHi, hi.size() }, { dLo, lo.size() } }, "the twiddle tables of %lld points could not be allocated",
                               1LL << groups[g].log2n));
        CPQ_OBJ_HIP(nullptr, hipMemcpy(dHi, hi.data(), hi.size() * sizeof(double), hipMemcpyHostToDevice));
        CPQ_OBJ_HIP(nullptr, hipMemcpy(dLo, lo.data(), lo.size() * sizeof(double), hipMemcpyHostToDevice));
        const cpq::MinphaseTables tables{ c2(dRoots), c2(dHi), c2(dLo) };
        for (const cpq::MinphaseChunk& c : chunks[g]) CPQ_TRY(runChunk(in, groups[g], c, tables, out, marked, t, kernelMs));
    }
    for (int i = 0; i < n; ++i)
        if (marked[(size_t)i]) {
            cpq_ir_buffer_free(&out[i]);
            std::memset(&out[i], 0, sizeof(out[i]));
            status[i] = CPQ_ERR_UNSUPPORTED;
        }
    g_lastKernelMs = kernelMs;
    return CPQ_OK;
}

void freeAll(cpq_ir_buffer* out, int n)
{
    for (int i = 0; i < n; ++i) {
        cpq_ir_buffer_free(&out[i]);
        std::memset(&out[i], 0, sizeof(out[i]));
    }
}

int prepareBatch(const cpq_ir_buffer* const* loaded, int n, double rate, float targetSec, int phase, const cpq_ir_buffer* const* current,
                 const double* currentScale, cpq_ir_prepared* out)
{
    for (int i = 0; i < n; ++i) {
        const int rc = cpq::irPrepareTrim(loaded[i], rate, targetSec, phase, current ? current[i] : nullptr, &out[i]);
        if (rc != CPQ_OK) return cpqi::fail(nullptr, rc, "IR %d: %s", i, cpq::irPrepareWhy(rc));
    }
    if (phase == CPQ_PHASE_MINIMUM && n > 0) {
        std::vector<const cpq_ir_buffer*> ptrs((size_t)n);
        std::vector<cpq_ir_buffer> mp((size_t)n);
        std::vector<int32_t> status((size_t)n, CPQ_OK);
        for (int i = 0; i < n; ++i) ptrs[(size_t)i] = &out[i].ir;
        const int rc = cpq_ir_minimum_phase_batch(ptrs.data(), n, 0, mp.data(), status.data());
        if (rc != CPQ_OK) return rc;        // the reason is already in cpq_last_error
        // a conversion the reference gives up on leaves the IR as trimmed
        for (int i = 0; i < n; ++i) {
            if (status[(size_t)i] == CPQ_OK) cpq::irPrepareAccept(&mp[(size_t)i], &out[i].ir);
            cpq_ir_buffer_free(&mp[(size_t)i]);
        }
    }
    for (int i = 0; i < n; ++i) {
        const int rc = cpq::irPrepareFinish(current ? current[i] : nullptr, currentScale ? currentScale[i] : 1.0, &out[i]);
        if (rc != CPQ_OK) return cpqi::fail(nullptr, rc, "IR %d: %s", i, cpq::irPrepareWhy(rc));
    }
    return CPQ_OK;
}

}  // namespace

extern "C" {

int32_t cpq_ir_minimum_phase_batch(const cpq_ir_buffer* const* in, int32_t n, int64_t workspace_bytes, cpq_ir_buffer* out, int32_t* status)
{
    g_lastKernelMs = -1.0;
    if (n < 0 || workspace_bytes < 0) return cpqi::fail(nullptr, CPQ_ERR_INVALID_ARG, "a negative count or workspace_bytes");
    if (n > 0 && (!in || !out || !status)) return cpqi::fail(nullptr, CPQ_ERR_INVALID_ARG, "null buffer list, output or status");
    for (int i = 0; i < n; ++i) std::memset(&out[i], 0, sizeof(out[i]));
    const int rc = cpqi::guardAlloc(nullptr, [&] { return minphaseBatch(in, n, workspace_bytes, out, status); });
    if (rc != CPQ_OK) freeAll(out, n);
    return rc;
}

int32_t cpq_ir_minimum_phase(const cpq_ir_buffer* in, cpq_ir_buffer* out)
{
    if (!out) return cpqi::fail(nullptr, CPQ_ERR_INVALID_ARG, "null output");
    int32_t status = CPQ_OK;
    const int32_t rc = cpq_ir_minimum_phase_batch(&in, 1, 0, out, &status);
    if (rc == CPQ_OK && status != CPQ_OK)
        return cpqi::fail(nullptr, status, "the reference gives up on this IR: 4 n above 8388608, or a value that is not finite");
    return rc;
}

double cpq_ir_minimum_phase_last_kernel_ms(void) { return g_lastKernelMs; }

int32_t cpq_ir_prepare_batch(const cpq_ir_buffer* const* loaded, int32_t n, double sample_rate, float target_ir_length_sec, int32_t phase_mode,
                             const cpq_ir_buffer* const* current_ir, const double* current_scale, cpq_ir_prepared* out)
{
    if (n < 0) return cpqi::fail(nullptr, CPQ_ERR_INVALID_ARG, "a negative count");
    if (n > 0 && (!loaded || !out)) return cpqi::fail(nullptr, CPQ_ERR_INVALID_ARG, "null buffer list or output");
    for (int i = 0; i < n; ++i) std::memset(&out[i], 0, sizeof(out[i]));
    const int rc = cpqi::guardAlloc(nullptr, [&] { return prepareBatch(loaded, n, sample_rate, target_ir_length_sec, phase_mode, current_ir, current_scale, out); });
    if (rc != CPQ_OK)
        for (int i = 0; i < n; ++i) {
            cpq_ir_prepared_free(&out[i]);
            std::memset(&out[i], 0, sizeof(out[i]));
        }
    return rc;
}

}  // extern "C"
