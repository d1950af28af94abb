// engine_quant.cpp -- cpq_quantizer: the stream's gain, a noise shaper and the PCM pack of fp64 rows, an object of its own beside
// cpq_engine.  The definition of a call, its refusals and the object that computes on the host (CPQ_QUANT_HOST) are
// quant_host.hpp's.  The device object (CPQ_QUANT_DEVICE) launches quant_kernels.hip's one kernel per call: this file checks,
// allocates, launches and copies, and holds no arithmetic of its own.
//
// The device object keeps the rules of cpq_limiter's, with object_support.hpp where they share.  The shaper's
// state -- err [kDitherMaxOrder][2 S], rng [4][2 S], coef [kLatticeOrder][2 S] -- and the gains [S] live on the device, laid out
// as the engine's dither stage keeps them; the QuantHost inside the object is the host's copy of gains and coefficients and its
// sample count, not its rows.  Cleared and seeded synchronously at create.  What changes that state outside a call (reset,
// set_gains, set_adaptive_coeffs) first waits for the stream, then copies synchronously.  One stream, one launch per call.
#include "engine_internal.hpp"

#include "object_support.hpp"
#include "quant_host.hpp"

using cpqi::failTo;

struct cpq_quantizer {
    cpq::QuantHost h;
    cpq::DitherParams params = {};
    std::string lastError;
    bool device = false;
    hipStream_t stream = nullptr;
    cpqi::DeviceBuffer<double> err, coef, gains;        // [kDitherMaxOrder][2 S], [kLatticeOrder][2 S], [S]
    cpqi::DeviceBuffer<unsigned long long> rng;         // [4][2 S]
    cpqi::RowStage rowsIn;                              // [2 S][cap]: host rows on their way in
    cpqi::DeviceBuffer<unsigned char> bytesOut;         // host bytes on their way out: rows at a pitch of its own
    int bytesCap = 0;                                   // samples per channel bytesOut has room for, at any layout
    bool timed = false;
    cpqi::TimingEvents<2> ev;                           // the last member: destroyed before the buffers are freed
};

namespace {

int nCh(const cpq_quantizer* p) { return 2 * p->h.streams; }

int checkCall(cpq_quantizer* p, const void* in, int64_t inStride, const void* pcm, int64_t pitch, int32_t layout, int32_t n, bool deviceRows)
{
    if (const char* why = cpq::quantCallFault(in, inStride, pcm, pitch, p->h.format, layout, p->h.streams, n, deviceRows))
        return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "%s (n_samples=%d, in_stride=%lld, pcm_pitch_bytes=%lld, layout=%d)", why, n,
                      (long long)inStride, (long long)pitch, layout);
    return CPQ_OK;
}

// the generator words of a fresh object, [4][2 S]
std::vector<unsigned long long> seedWords(const cpq_quantizer* p)
{
    const size_t C = (size_t)nCh(p);
    std::vector<unsigned long long> words(4 * C);
    for (int side = 0; side < 2; ++side) {
        unsigned long long s[4];
        cpq::ditherSeed(p->h.shaper, p->h.rate, p->h.bits, side, s);
        for (int k = 0; k < 4; ++k)
            for (size_t ch = (size_t)side; ch < C; ch += 2) words[(size_t)k * C + ch] = s[k];
    }
    return words;
}

// synchronous: errors to 0, generators to their seeds
int clearDevice(cpq_quantizer* p, std::string* sink)
{
    const std::vector<unsigned long long> words = seedWords(p);
    CPQ_OBJ_HIP(sink, hipMemset(p->err, 0, sizeof(double) * cpq::kDitherMaxOrder * (size_t)nCh(p)));
    CPQ_OBJ_HIP(sink, hipMemcpy(p->rng, words.data(), sizeof(unsigned long long) * words.size(), hipMemcpyHostToDevice));
    return CPQ_OK;
}

// synchronous: the coefficient table of every stream from the host's copy
int uploadCoef(cpq_quantizer* p, std::string* sink)
{
    const size_t C = (size_t)nCh(p);
    std::vector<double> table(cpq::kLatticeOrder * C);
    for (int i = 0; i < cpq::kLatticeOrder; ++i)
        for (size_t ch = 0; ch < C; ++ch) table[(size_t)i * C + ch] = p->h.d[ch / 2].coeffs[i];
    CPQ_OBJ_HIP(sink, hipMemcpy(p->coef, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice));
    return CPQ_OK;
}

int createDevice(cpq_quantizer* p)
{
    const size_t C = (size_t)nCh(p);
    CPQ_TRY(cpqi::allocAll(nullptr, { { p->err, cpq::kDitherMaxOrder * C }, { p->coef, cpq::kLatticeOrder * C }, { p->gains, C / 2 }, { p->rng, 4 * C } },
                           "the shaper state of %d streams could not be allocated", p->h.streams));
    CPQ_TRY(p->ev.create(nullptr));
    CPQ_TRY(clearDevice(p, nullptr));
    CPQ_TRY(uploadCoef(p, nullptr));
    CPQ_OBJ_HIP(nullptr, hipMemcpy(p->gains, p->h.gains.data(), sizeof(double) * (C / 2), hipMemcpyHostToDevice));
    CPQ_OBJ_HIP(nullptr, hipDeviceSynchronize());       // the clears have run before the first call, whatever its stream
    return CPQ_OK;
}

// a checked call on device rows and device bytes: enqueued on the object's stream
int runDevice(cpq_quantizer* p, const double* dIn, int64_t inStride, void* dPcm, int64_t pitch, int layout, int n)
{
    const cpq::QuantLaunch a{ n, nCh(p), cpq::ditherOrder(p->h.shaper), p->h.format, layout, inStride, pitch };
    CPQ_OBJ_HIP(&p->lastError, hipEventRecord(p->ev[0], p->stream));
    if (!cpq::launch_quantize(p->stream, dIn, dPcm, a, p->params, p->gains, p->coef, p->err, p->rng))
        return failTo(&p->lastError, CPQ_ERR_UNSUPPORTED, "no quantizer kernel for shaper %d, format %d, layout %d", p->h.shaper, p->h.format, layout);
    CPQ_OBJ_HIP(&p->lastError, hipGetLastError());
    CPQ_OBJ_HIP(&p->lastError, hipEventRecord(p->ev[1], p->stream));
    p->h.pos += n;
    p->timed = true;
    return CPQ_OK;
}

// host rows and host bytes through the object's buffers; synchronises
int runDeviceHostRows(cpq_quantizer* p, const double* in, int64_t inStride, void* pcm, int64_t pitch, int layout, int n)
{
    const int format = p->h.format;
    const size_t rows = (size_t)cpq::pcm::rowsOf(layout, p->h.streams);
    const size_t width = (size_t)cpq::pcm::widthBytes(format, layout, n);
    const size_t devPitch = (width + 15) & ~(size_t)15;                 // every row of the stage starts on 16 bytes
    CPQ_TRY(p->rowsIn.ensure(&p->lastError, p->stream, n));
    if (n + 16 > p->bytesCap) {
        // 2 S bps (n + 16) bytes hold rows of either layout at devPitch
        if (p->bytesOut) CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
        if (cpqi::grow(nullptr, p->bytesOut, p->bytesCap, n + 16, (size_t)nCh(p) * (size_t)cpq::pcm::bytesPerSample(format), "byte buffer") != CPQ_OK)
            return failTo(&p->lastError, CPQ_ERR_OOM, "byte buffer of %d samples could not be allocated", n);
    }
    CPQ_TRY(p->rowsIn.upload(&p->lastError, in, inStride, n, hipMemcpyHostToDevice, p->stream));
    CPQ_TRY(runDevice(p, p->rowsIn.buf, p->rowsIn.cap, p->bytesOut.get(), (int64_t)devPitch, layout, n));
    CPQ_OBJ_HIP(&p->lastError, hipMemcpy2DAsync(pcm, (size_t)pitch, p->bytesOut.get(), devPitch, width, rows, hipMemcpyDeviceToHost, p->stream));
    CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
    return CPQ_OK;
}

}  // namespace

extern "C" {

int32_t cpq_quantizer_create(int32_t n_streams, double sample_rate, int32_t shaper, int32_t bit_depth, int32_t container_format, uint32_t flags,
                             cpq_quantizer** out)
{
    if (!out) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (n_streams < 1 || n_streams > 32767) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "n_streams %d outside 1..32767", n_streams);
    if (flags & ~(uint32_t)(CPQ_QUANT_HOST | CPQ_QUANT_DEVICE)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "unknown flags");
    if ((flags & CPQ_QUANT_HOST) && (flags & CPQ_QUANT_DEVICE))
        return failTo(nullptr, CPQ_ERR_INVALID_ARG, "CPQ_QUANT_HOST and CPQ_QUANT_DEVICE exclude each other");
    if (!(sample_rate > 0.0) || !std::isfinite(sample_rate)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "sample_rate must be finite and > 0");
    if (!cpq::ditherOrder(shaper)) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "unknown dither shaper %d", shaper);
    if (!cpq::quantContainer(container_format))
        return failTo(nullptr, CPQ_ERR_INVALID_ARG, "container_format %d is not CPQ_PCM_S16, CPQ_PCM_S24 or CPQ_PCM_S32", container_format);
    if (bit_depth < 1 || bit_depth > 32) return failTo(nullptr, CPQ_ERR_INVALID_ARG, "bit_depth %d outside 1..32", bit_depth);
    if (bit_depth > cpq::quantWidth(container_format))
        return failTo(nullptr, CPQ_ERR_UNSUPPORTED, "bit_depth %d above the %d bits of the container", bit_depth, cpq::quantWidth(container_format));
    if (!flags) return failTo(nullptr, CPQ_ERR_UNSUPPORTED, "say CPQ_QUANT_HOST or CPQ_QUANT_DEVICE");
    return cpqi::guardAlloc(nullptr, [&]() -> int {
        std::unique_ptr<cpq_quantizer, void (*)(cpq_quantizer*)> p(new cpq_quantizer(), cpq_quantizer_destroy);
        if (!p->h.init(n_streams, sample_rate, shaper, bit_depth, container_format))
            return failTo(nullptr, CPQ_ERR_INVALID_ARG, "no design for shaper %d at %d bits", shaper, bit_depth);
        p->device = (flags & CPQ_QUANT_DEVICE) != 0;
        const cpq::DitherHost& d0 = p->h.d[0];
        std::copy(d0.coeffs, d0.coeffs + cpq::kDitherMaxOrder, p->params.c);
        p->params.scale = d0.scale;
        p->params.invScale = d0.invScale;
        p->params.maxV = 1.0 - (1.0 / d0.invScale);
        p->params.headroom = 1.0;
        p->params.scrub = 0;
        p->rowsIn.rows = 2 * (size_t)n_streams;
        if (p->device) {
            CPQ_TRY(cpqi::checkCurrentDevice());
            CPQ_TRY(createDevice(p.get()));
        }
        *out = p.release();
        return CPQ_OK;
    });
}

void cpq_quantizer_destroy(cpq_quantizer* p) { delete p; }

const char* cpq_quantizer_last_error(const cpq_quantizer* p) { return p ? p->lastError.c_str() : cpq_last_error(nullptr); }

int32_t cpq_quantizer_set_stream(cpq_quantizer* p, void* stream)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!p->device) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "cpq_quantizer_set_stream on a host object");
    return cpqi::setStream(&p->lastError, p->stream, stream);
}

int32_t cpq_quantizer_reset(cpq_quantizer* p)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (p->device) {
        CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
        CPQ_TRY(cpqi::guardAlloc(&p->lastError, [&] { return clearDevice(p, &p->lastError); }));
    }
    p->h.reset();
    return CPQ_OK;
}

int32_t cpq_quantizer_set_gains(cpq_quantizer* p, const double* gains)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!gains) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "null gains");
    for (int s = 0; s < p->h.streams; ++s)
        if (!std::isfinite(gains[s]) || gains[s] < 0.0) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "the gain of stream %d is not finite and >= 0", s);
    if (p->h.pos)
        return failTo(&p->lastError, CPQ_ERR_NOT_READY, "gains are set at the start of a programme: %lld samples were taken; reset first", (long long)p->h.pos);
    if (p->device) {
        CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
        CPQ_OBJ_HIP(&p->lastError, hipMemcpy(p->gains, gains, (size_t)p->h.streams * sizeof(double), hipMemcpyHostToDevice));
    }
    std::copy(gains, gains + p->h.streams, p->h.gains.begin());
    return CPQ_OK;
}

int32_t cpq_quantizer_set_adaptive_coeffs(cpq_quantizer* p, int32_t stream, const double* k, int32_t n)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (p->h.shaper != CPQ_DITHER_ADAPTIVE9) return failTo(&p->lastError, CPQ_ERR_NOT_READY, "the object does not run the adaptive shaper");
    if (stream != CPQ_ALL_STREAMS && (stream < 0 || stream >= p->h.streams))
        return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "stream %d outside 0..%d", stream, p->h.streams - 1);
    if (n < 0 || n > cpq::kLatticeOrder) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "%d coefficients outside 0..%d", n, cpq::kLatticeOrder);
    if (n > 0 && !k) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "null coefficients");
    const int s0 = stream == CPQ_ALL_STREAMS ? 0 : stream, s1 = stream == CPQ_ALL_STREAMS ? p->h.streams : stream + 1;
    if (p->device) CPQ_OBJ_HIP(&p->lastError, hipStreamSynchronize(p->stream));
    p->h.setAdaptive(s0, s1, k, n);
    if (!p->device) return CPQ_OK;
    CPQ_TRY(cpqi::guardAlloc(&p->lastError, [&] { return uploadCoef(p, &p->lastError); }));
    // reset() of those streams: rows 0 .. kLatticeOrder - 1 of their channels
    CPQ_OBJ_HIP(&p->lastError, hipMemset2D(p->err.get() + 2 * s0, sizeof(double) * (size_t)nCh(p), 0, sizeof(double) * 2 * (size_t)(s1 - s0), cpq::kLatticeOrder));
    return CPQ_OK;
}

int32_t cpq_quantizer_get_adaptive_coeffs(const cpq_quantizer* p, int32_t stream, double k[9])
{
    if (!p || !k) return CPQ_ERR_INVALID_ARG;
    if (p->h.shaper != CPQ_DITHER_ADAPTIVE9) return CPQ_ERR_NOT_READY;
    if (stream < 0 || stream >= p->h.streams) return CPQ_ERR_INVALID_ARG;
    std::copy(p->h.d[(size_t)stream].coeffs, p->h.d[(size_t)stream].coeffs + cpq::kLatticeOrder, k);
    return CPQ_OK;
}

int32_t cpq_quantizer_process_device(cpq_quantizer* p, const double* d_in, int64_t in_stride, void* d_pcm, int64_t pcm_pitch_bytes, int32_t layout,
                                     int32_t n_samples)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    if (!p->device) return failTo(&p->lastError, CPQ_ERR_INVALID_ARG, "cpq_quantizer_process_device on a host object");
    CPQ_TRY(checkCall(p, d_in, in_stride, d_pcm, pcm_pitch_bytes, layout, n_samples, true));
    return runDevice(p, d_in, in_stride, d_pcm, pcm_pitch_bytes, layout, n_samples);
}

int32_t cpq_quantizer_process(cpq_quantizer* p, const double* in, int64_t in_stride, void* pcm, int64_t pcm_pitch_bytes, int32_t layout, int32_t n_samples)
{
    if (!p) return CPQ_ERR_INVALID_ARG;
    CPQ_TRY(checkCall(p, in, in_stride, pcm, pcm_pitch_bytes, layout, n_samples, false));
    if (p->device) return runDeviceHostRows(p, in, in_stride, pcm, pcm_pitch_bytes, layout, n_samples);
    p->h.process(in, in_stride, n_samples, static_cast<unsigned char*>(pcm), pcm_pitch_bytes, layout);
    return CPQ_OK;
}

double cpq_quantizer_last_kernel_ms(cpq_quantizer* p)
{
    if (!p || !p->device || !p->timed) return -1.0;
    if (hipEventSynchronize(p->ev[1]) != hipSuccess) {
        (void)hipGetLastError();
        return -1.0;
    }
    return p->ev.elapsed(0, 1);
}

}  // extern "C"
