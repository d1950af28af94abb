// engine_pcm.cpp -- packed PCM in and out (include/convopeq_mi355x.h): cpq_pcm_unpack / cpq_pcm_pack and the whole-chain call
// with a converter at each end.  The host-pointer call is viaStaging's loop (stagedCall, engine_internal.hpp) with copies that
// carry packed bytes: upload packed, unpack into the staging rows, the unchanged body, pack from the staging rows, download
// packed.  Layout arithmetic: pcm_layout.hpp; kernels: pcm_kernels.hip.  cpq_pcm_unpack / cpq_pcm_pack keep their own
// round trips: packed bytes on one side and, for the pack, rows that go up into stageOut -- hostRoundTrip would need both.
#include "engine_internal.hpp"
#include "pcm_layout.hpp"

using namespace cpqi;
namespace pcm = cpq::pcm;

namespace {

int checkFormat(cpq_engine* e, int format, int layout, bool output)
{
    if (pcm::bytesPerSample(format) < 0) return fail(e, CPQ_ERR_INVALID_ARG, "unknown PCM format %d", format);
    if (!pcm::validLayout(layout)) return fail(e, CPQ_ERR_INVALID_ARG, "unknown PCM layout %d", layout);
    if (output && format == CPQ_PCM_S16 && !(e->ditherShaper != CPQ_DITHER_OFF && e->ditherBits <= 16))
        return fail(e, CPQ_ERR_UNSUPPORTED, "16-bit output needs the dither stage at 16 bits or fewer (cpq_engine_set_dither)");
    return CPQ_OK;
}

int checkAligned(cpq_engine* e, const void* pcmBuf, int format, const void* rows)
{
    if (reinterpret_cast<uintptr_t>(pcmBuf) % (uintptr_t)pcm::alignmentOf(format))
        return fail(e, CPQ_ERR_INVALID_ARG, "packed buffer must be aligned to its %d-byte element", pcm::alignmentOf(format));
    if (reinterpret_cast<uintptr_t>(rows) & 7u) return fail(e, CPQ_ERR_INVALID_ARG, "rows must be 8-byte aligned");
    return CPQ_OK;
}

// the converters alone: arguments of both directions
int checkConvert(cpq_engine* e, const void* pcmBuf, int format, int layout, uint32_t flags, const void* rows, int n, bool output)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!pcmBuf || !rows) return fail(e, CPQ_ERR_INVALID_ARG, "null buffer");
    CPQ_TRY(checkFormat(e, format, layout, output));
    if (flags & ~CPQ_PCM_SANITIZE) return fail(e, CPQ_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
    if (n <= 0 || n > e->maxCall) return fail(e, CPQ_ERR_INVALID_ARG, "n=%d outside 1..%d (max_blocks_per_call * block_size)", n, e->maxCall);
    return checkAligned(e, pcmBuf, format, rows);
}

// the packed pair on the device, sized for the call's formats at the longest call; a call that needs more replaces the group
int ensurePcmBuffers(cpq_engine* e, int inFormat, int outFormat)
{
    const int S = e->desc.n_streams;
    const int64_t nMax = e->maxCall;
    const size_t needIn = inFormat < 0 ? 0 : (size_t)pcm::totalBytes(inFormat, CPQ_PCM_PLANAR, S, nMax);
    const size_t needOut = outFormat < 0 ? 0 : (size_t)pcm::totalBytes(outFormat, CPQ_PCM_PLANAR, S, nMax);
    if (e->pcmIn && needIn <= e->pcmInCap && needOut <= e->pcmOutCap) return CPQ_OK;
    const size_t capIn = std::max({ needIn, e->pcmInCap, (size_t)16 }), capOut = std::max({ needOut, e->pcmOutCap, (size_t)16 });
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    e->pcmIn.reset();
    e->pcmOut.reset();
    e->pcmInCap = e->pcmOutCap = 0;
    CPQ_TRY(allocAll(e, { { e->pcmIn, capIn }, { e->pcmOut, capOut } }, "packed PCM buffers of %zu + %zu bytes could not be allocated", capIn, capOut));
    e->pcmInCap = capIn;
    e->pcmOutCap = capOut;
    return CPQ_OK;
}

int enqueueUnpack(cpq_engine* e, const void* dPcm, int format, int layout, uint32_t flags, double* dRows, int n)
{
    ProfScope p(e, CPQ_K_PCM);
    if (!cpq::launch_pcm_unpack(e->stream, dPcm, format, layout, dRows, n, e->desc.n_streams, (flags & CPQ_PCM_SANITIZE) ? callbackLen(e) : 0))
        return fail(e, CPQ_ERR_UNSUPPORTED, "no unpack kernel for PCM format %d", format);      // a missing kernel is an error
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

int enqueuePack(cpq_engine* e, const double* dRows, void* dPcm, int format, int layout, int n)
{
    ProfScope p(e, CPQ_K_PCM);
    if (!cpq::launch_pcm_pack(e->stream, dRows, dPcm, format, layout, n, e->desc.n_streams))
        return fail(e, CPQ_ERR_UNSUPPORTED, "no pack kernel for PCM format %d", format);
    CPQ_HIP(e, hipGetLastError());
    return CPQ_OK;
}

// everything cpq_engine_process_block_pcm[_device] refuses, before any state moves or anything is enqueued
int checkPcmCall(cpq_engine* e, const void* in, int inFormat, const void* out, int outFormat, int layout, uint32_t flags, int n)
{
    if (!e) return CPQ_ERR_INVALID_ARG;
    if (!in || !out) return fail(e, CPQ_ERR_INVALID_ARG, "null buffer");
    CPQ_TRY(checkFormat(e, inFormat, layout, false));
    CPQ_TRY(checkFormat(e, outFormat, layout, true));
    if (flags & ~CPQ_PCM_SANITIZE) return fail(e, CPQ_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
    CPQ_TRY(checkBlockCall(e, in, out, n));
    if (!pcm::buffersAllowed(in, inFormat, out, outFormat, layout, e->desc.n_streams, n))
        return fail(e, CPQ_ERR_INVALID_ARG, "in and out overlap: they may be the same buffer only when format and layout are equal");
    return CPQ_OK;
}

// packed bytes over the bus: the staging rows are filled by the unpack kernel and emptied by the pack kernel (PcmBody)
struct PcmHostIo {
    const void* in; int inFormat;
    void* out; int outFormat;
    int layout;
    const void* hostIn() const { return in; }
    const void* hostOut() const { return out; }
    int uploadAll(cpq_engine* e, int n) const
    {
        CPQ_HIP(e, hipMemcpyAsync(e->pcmIn, in, (size_t)pcm::totalBytes(inFormat, layout, e->desc.n_streams, n), hipMemcpyHostToDevice, e->stream));
        return CPQ_OK;
    }
    int downloadAll(cpq_engine* e, int n) const
    {
        CPQ_HIP(e, hipMemcpyAsync(out, e->pcmOut, (size_t)pcm::totalBytes(outFormat, layout, e->desc.n_streams, n), hipMemcpyDeviceToHost, e->stream));
        return CPQ_OK;
    }
    int uploadChunk(cpq_engine* e, int i, size_t chunkLen, int n) const
    {
        const pcm::ChunkCopy c = pcm::chunkCopy(inFormat, layout, e->desc.n_streams, n, (int64_t)chunkLen, i);
        CPQ_HIP(e, hipMemcpy2DAsync(e->pcmIn + c.devOffset, (size_t)c.devPitch, static_cast<const char*>(in) + c.hostOffset, (size_t)c.hostPitch,
                                    (size_t)c.width, (size_t)c.rows, hipMemcpyHostToDevice, e->copyIn));
        return CPQ_OK;
    }
    int downloadChunk(cpq_engine* e, int i, size_t chunkLen, int n) const
    {
        const pcm::ChunkCopy c = pcm::chunkCopy(outFormat, layout, e->desc.n_streams, n, (int64_t)chunkLen, i);
        CPQ_HIP(e, hipMemcpy2DAsync(static_cast<char*>(out) + c.hostOffset, (size_t)c.hostPitch, e->pcmOut + c.devOffset, (size_t)c.devPitch,
                                    (size_t)c.width, (size_t)c.rows, hipMemcpyDeviceToHost, e->copyOut));
        return CPQ_OK;
    }
};

}  // namespace

extern "C" {

int32_t cpq_pcm_bytes_per_sample(int32_t format) { return pcm::bytesPerSample(format); }

int32_t cpq_pcm_unpack_device(cpq_engine* e, const void* dPcm, int32_t format, int32_t layout, uint32_t flags, double* dRows, int32_t n)
{
    CPQ_TRY(checkConvert(e, dPcm, format, layout, flags, dRows, n, false));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueueUnpack(e, dPcm, format, layout, flags, dRows, n);
}

int32_t cpq_pcm_pack_device(cpq_engine* e, const double* dRows, void* dPcm, int32_t format, int32_t layout, int32_t n)
{
    CPQ_TRY(checkConvert(e, dPcm, format, layout, 0, dRows, n, true));
    CPQ_HIP(e, hipSetDevice(e->device));
    return enqueuePack(e, dRows, dPcm, format, layout, n);
}

int32_t cpq_pcm_unpack(cpq_engine* e, const void* pcmBuf, int32_t format, int32_t layout, uint32_t flags, double* rows, int32_t n)
{
    CPQ_TRY(checkConvert(e, pcmBuf, format, layout, flags, rows, n, false));
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_TRY(ensureCallBuffer(e, e->stageIn, "upload staging"));
    CPQ_TRY(ensurePcmBuffers(e, format, -1));
    const int S = e->desc.n_streams;
    CPQ_HIP(e, hipMemcpyAsync(e->pcmIn, pcmBuf, (size_t)pcm::totalBytes(format, layout, S, n), hipMemcpyHostToDevice, e->stream));
    CPQ_TRY(enqueueUnpack(e, e->pcmIn, format, layout, flags, e->stageIn, n));
    CPQ_HIP(e, hipMemcpyAsync(rows, e->stageIn, (size_t)e->nCh * n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

int32_t cpq_pcm_pack(cpq_engine* e, const double* rows, void* pcmBuf, int32_t format, int32_t layout, int32_t n)
{
    CPQ_TRY(checkConvert(e, pcmBuf, format, layout, 0, rows, n, true));
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_TRY(ensureCallBuffer(e, e->stageOut, "download staging"));
    CPQ_TRY(ensurePcmBuffers(e, -1, format));
    const int S = e->desc.n_streams;
    CPQ_HIP(e, hipMemcpyAsync(e->stageOut, rows, (size_t)e->nCh * n * sizeof(double), hipMemcpyHostToDevice, e->stream));
    CPQ_TRY(enqueuePack(e, e->stageOut, e->pcmOut, format, layout, n));
    CPQ_HIP(e, hipMemcpyAsync(pcmBuf, e->pcmOut, (size_t)pcm::totalBytes(format, layout, S, n), hipMemcpyDeviceToHost, e->stream));
    CPQ_HIP(e, hipStreamSynchronize(e->stream));
    return CPQ_OK;
}

int32_t cpq_engine_process_block_pcm_device(cpq_engine* e, const void* dIn, int32_t inFormat, void* dOut, int32_t outFormat,
                                            int32_t layout, uint32_t flags, int32_t nSamples)
{
    CPQ_TRY(checkPcmCall(e, dIn, inFormat, dOut, outFormat, layout, flags, nSamples));
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_TRY(ensureCallBuffer(e, e->stageIn, "upload staging"));
    CPQ_TRY(ensureCallBuffer(e, e->stageOut, "download staging"));
    CPQ_TRY(enqueueUnpack(e, dIn, inFormat, layout, flags, e->stageIn, nSamples));
    CPQ_TRY(meteredChain(e, e->stageIn, e->stageOut, nSamples));
    return enqueuePack(e, e->stageOut, dOut, outFormat, layout, nSamples);
}

int32_t cpq_engine_process_block_pcm(cpq_engine* e, const void* in, int32_t inFormat, void* out, int32_t outFormat, int32_t layout,
                                     uint32_t flags, int32_t nSamples)
{
    CPQ_TRY(checkPcmCall(e, in, inFormat, out, outFormat, layout, flags, nSamples));
    CPQ_HIP(e, hipSetDevice(e->device));
    CPQ_TRY(ensurePcmBuffers(e, inFormat, outFormat));
    PcmHostIo io{ in, inFormat, out, outFormat, layout };
    // body sees the time chunks of the call in order, each of `len` samples per channel: chunk i's packed bytes sit at the
    // device offsets pcm::chunkCopy gives.  Chunks are whole callbacks, so the sanitise phase of each starts at 0.
    int chunk = 0;
    const int S = e->desc.n_streams;
    auto body = [&](const double* a, double* b, int len) -> int {
        const int64_t offIn = pcm::chunkCopy(inFormat, layout, S, nSamples, len, chunk).devOffset;
        const int64_t offOut = pcm::chunkCopy(outFormat, layout, S, nSamples, len, chunk).devOffset;
        ++chunk;
        CPQ_TRY(enqueueUnpack(e, e->pcmIn + offIn, inFormat, layout, flags, const_cast<double*>(a), len));
        CPQ_TRY(meteredChain(e, a, b, len));
        return enqueuePack(e, b, e->pcmOut + offOut, outFormat, layout, len);
    };
    return stagedCall(e, io, nSamples, body, e->osFactor);
}

}  // extern "C"
