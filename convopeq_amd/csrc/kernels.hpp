// kernels.hpp -- launchers of the gfx950 kernels of libconvopeq_mi355x (implemented in *.hip).
// All launchers enqueue on `stream` and never synchronise.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "host_design.hpp"
#include "minphase_plan.hpp"
#include "src_device_plan.hpp"
#include "prog_plan.hpp"
#include "lim_plan.hpp"
#include "learn_plan.hpp"

namespace cpq {

// partition size with dedicated wave-level FFT kernels; other powers of two (64..2048) use generic kernels
constexpr int kP = 512;            // samples per partition == complex bins per packed spectrum
constexpr int kMacPrefetch = 4;    // FDL/IR rows kept in flight per lane in k_fdl_mac
constexpr int kMacMaxTile = 32;    // largest outputs-per-lane tile; partition counts are padded to it
constexpr int kBands = 20;

struct FftTables {
    const double2* tw512;    // exp(-2 pi i m / P),  m < P   (P = partition size; 512 in the headline config)
    const double2* tw1024;   // exp(-2 pi i k / 2P), k < P
    // P > 4096 (four-step transforms, P = M1 * 512): the same values in the order the passes walk them, so that a wave reads
    // 64 consecutive entries instead of 64 cache lines (fill_big_twiddles):
    const double2* twCol = nullptr;     // [k1][n2] = tw512[n2 k1]         (column-pass twiddle W_P^(n2 k1))
    const double2* twSplit = nullptr;   // [k1][k2] = tw1024[k1 + M1 k2]   (real-FFT split of bin k1 + M1 k2)
};
// host: the two reordered tables of P entries each from tw512 / tw1024 (P > 4096)
void fill_big_twiddles(const double2* tw512, const double2* tw1024, int P, double2* twCol, double2* twSplit);

// Overlap-save framing + 1024-point real FFT of T blocks per channel into the frequency-domain delay
// line (FDL) ring; also saves the last block as the next call's overlap history.
// forceSplit > 0 (P = 4096 only, the diagnostic entry): that many workgroups walk a channel's frames instead of the launcher's choice
void launch_rfft_fwd_ols(hipStream_t stream, const double* in, int64_t chStride, const double* histOld,
                         double* histNew, double2* X, double2* XDN, FftTables tw, int P, int nCh, int T,
                         int head, int ringSlots, double2* scratch = nullptr, int forceSplit = 0);

// P = 512 only (rfft_fwd_can_carry_side): the same launch also copies every block into up to two other accumulators
// (dst[a] + channel * dstStride[a] + dstOff[a], offsets even) and stores a table of <= kGatherTabMax entries to tabDst -- a plan
// group's input accumulation and chunk tables on the call's first launch instead of a k_rows_gather_multi launch of their own.
bool rfft_fwd_can_carry_side(int P, int nSide, const int64_t* dstStride, const int64_t* dstOff, int nTab);
void launch_rfft_fwd_ols_side(hipStream_t stream, const double* in, int64_t chStride, const double* histOld, double* histNew, double2* X,
                              double2* XDN, FftTables tw, int nCh, int T, int head, int ringSlots, int nSide, double* const* dst,
                              const int64_t* dstStride, const int64_t* dstOff, long long* tabDst, const long long* tab, int nTab,
                              double* tailDst = nullptr, int64_t tailStride = 0, int tailLen = 0);      // tail*: the tailLen samples behind the T blocks of every source row -> tailDst rows
// One tail layer's tap on the output (Get(), :1620-1633): the layer's delay line ([channel][ringSize], a power of two), the ring
// position each chunk -- or, for the inverse transform below, each block -- reads from (negative: nothing to add) and the layer's
// gain: out = out + ring (gain within 1e-12 of 1) or out + ring * gain.  An empty tap (ring == nullptr) means "no such layer".
struct RingTap {
    const double* ring = nullptr;
    int ringSize = 2;
    const long long* sched = nullptr;
    double gain = 0.0;
};
// P = 512 inverse transform that also adds the delay-line blocks of up to two tail layers to the rows it stores: block t reads
// tap x at x.sched[t], a before b (b may be empty)
void launch_rfft_inv_ols_add(hipStream_t stream, const double2* Y, double* out, int64_t chStride, FftTables tw, int nCh, int T,
                             RingTap a, RingTap b);

// IR partition spectra: frames [h[k*P .. (k+1)*P) | 0] for k < nParts.
void launch_ir_spectra(hipStream_t stream, const double* heff, int heffLen, double2* H, double2* HDN,
                       FftTables tw, int P, int nParts, double2* scratch = nullptr);

// H[k][bin] *= gain[bin] (gain has P+1 entries: bins 0..P) for nParts partition spectra
void launch_spectrum_gain(hipStream_t stream, double2* H, double2* HDN, const double* gain, int P, int nParts);

// Y[c][t][bin] = sum_{k<K} X[c][slot(head+t-k)][bin] * H[ir(c)][k][bin] for t < T and every element bin < P (P: a power of two
// >= 64); slot(s) = s & (ringSlots - 1).  Element 0 packs (DC, Nyquist), two independent real MACs: the 4- and 8-row tiles and the
// cooperative kernel produce it themselves, the 16- and 32-row tiles store a complex product there that launch_fdl_mac_dcnyq
// (fdl_mac_needs_dcnyq) must overwrite.
// tile: 0 = automatic (fdl_mac_variant), 4 / 8 / 16 / 32 = that register tile, kMacTileCoop / kMacTileRows128 = the cooperative
// kernel's 64- / 128-row workgroup at any T (engines only pass 0 / 4 / 8 / 16 / 32: cpq_engine_create).
// What a call consumes: IR rows 0 .. K - 1 of the slots irSlot[] names and ring slots head + t - k (t < T, k < K); every
// accumulation is guarded by k < K, so neither the zero padding behind row K nor the rest of the ring enters a result.
// What it may LOAD (and discard) beyond that, TT = the variant's tile:
//   IR rows     0 .. max(K, kMacPrefetch) - 1 (register tiles: the prologue fetches kMacPrefetch rows whatever K is),
//               0 .. max(K, 8) - 1 (cooperative kernel: the prologue stages one chunk of 8 rows)
//   ring slots  head - max(K - 1, kMacPrefetch) .. head + alignUp(T, TT) - 1 (register tiles),
//               head - alignUp(K, 8) .. head + alignUp(T, 64) - 1 (cooperative kernel; alignUp(T, 128) with 128-row workgroups),
//               every index masked by ringSlots - 1
// So a slot needs max(K, 8) allocated rows -- both engine rules (alignUp(K, 32) + 16 rows and more per slot, alignUp(K, 32) + 32
// rows per layer of a layered slot) allocate at least 48 -- and the ring any power of two >= K + T - 1 slots, so that the
// consumed slots are distinct (the engines allocate nextPow2(alignUp(K, 32) + 32 + T)).
// hPrivate: every channel has its own IR rows (no CPQ_ALL_STREAMS sharing): single-tile calls may then stream them past the cache
constexpr int kMacTileCoop = -1;
constexpr int kMacTileRows128 = -2;      // the cooperative kernel's 128-row workgroup at any T
// what fdl_mac_variant returns for the two cooperative geometries (a register tile returns its size)
constexpr int kMacVariantCoop = 0;
constexpr int kMacVariantRows128 = 128;
void launch_fdl_mac(hipStream_t stream, int tile, const double2* X, const double2* H, const int* irSlot,
                    double2* Y, int P, int nCh, int K, int ringSlots, int head, int T, int64_t hSlotStride,
                    bool hPrivate = false);      // K = partitions in use (walked in steps of the variant's tile)

// packed bin 0: DC and Nyquist are two independent real MACs.
// kernel variant launch_fdl_mac uses for (tile, T) (kMacVariantCoop / kMacVariantRows128 = workgroup-cooperative) and the
// multiple kPad must be padded to
int fdl_mac_variant(int tile, int T);
int fdl_mac_kpad_align(int tile, int T);
bool fdl_mac_needs_dcnyq(int tile, int T);    // only the 16- and 32-row register tiles leave packed bin 0 to launch_fdl_mac_dcnyq
void launch_fdl_mac_dcnyq(hipStream_t stream, const double2* XDN, const double2* HDN, const int* irSlot,
                          double2* Y, int P, int nCh, int K, int ringSlots, int head, int T, int hdnStride);

// inverse 1024-point real FFT of Y, scaled 1/N, second half (P samples) to out.
// P > 4096 (8192 ... 131072): four-step transforms through `scratch` ([transforms][P] double2); the spectra are
// then stored permuted (element k1 * 512 + k2 = bin k1 + (P / 512) k2), consistently in all three launchers.
// forceSplit: as in launch_rfft_fwd_ols.
void launch_rfft_inv_ols(hipStream_t stream, const double2* Y, double* out, int64_t chStride, FftTables tw,
                         int P, int nCh, int T, double2* scratch = nullptr, int forceSplit = 0);
// The same transform with its result stored straight into per-channel rings: block t of channel c at ring[c][(p_t + i) &
// (ringSize - 1)], p_t = pos[t] (device table; negative: the block is dropped) or pos0 + t P when pos is null -- the
// output-ring / delay-line write of a plan-group layer without the pass over the blocks in between.
void launch_rfft_inv_ols_ring(hipStream_t stream, const double2* Y, double* ring, int ringSize, const long long* pos,
                              long long pos0, FftTables tw, int P, int nCh, int T, double2* scratch = nullptr);

// Device tables of one cascade -- the EQ's 20 TPT-SVF bands, or the output filter's DF-II-T sections in band slots 0 .. 2 --
// for every stream s and its channels ch = 0, 1.  The one place that states their layout:
struct CascadeTables {
    double* coef = nullptr;      // [2 s + ch][kBands][6]   a1 a2 a3 m0 m1 m2; DF-II-T section: b0 b1 b2 a1 a2 -
    int* flags = nullptr;        // [2 s + ch][kBands]      bit 0 active, 1 not a Stereo band, 2 DF-II-T, 3 parallel, 4 / 5 Mid / Side
    double* satGain = nullptr;   // [2 s + ch][2]           saturation, total gain
    double* state = nullptr;     // [2 s + ch][kBands][2]   carried across calls
    double* tp = nullptr;        // [s][kBands * kSvfTpTableDoubles]   tables of the time-parallel kernels (below)
    static constexpr size_t stateDoubles(int nCh) { return (size_t)nCh * kBands * 2; }
    static constexpr size_t stateAt(int s, int ch, int band) { return ((size_t)(2 * s + ch) * kBands + band) * 2; }
};

// 20-band TPT-SVF cascade over the tables t (t.tp is not read), lane = (channel, band), bands skewed in time across lanes.
// streamPairs: one wave per stream (its L and R channel) instead of 3 channels per wave -- required when a band has flag
// bits 4/5 (Mid / Side component band).
void launch_svf_cascade(hipStream_t stream, const double* in, double* out, int64_t chStride, int nCh,
                        int nSamples, CascadeTables t, bool streamPairs);

// Time-parallel SVF cascade (svf_kernels.hip): whole 8192-sample spans on k_svf_cascade_tpv<8> (one workgroup per channel, or
// chained spans, below), what is left from 1024 samples up as one span of 1 ... 7 waves x 1024 samples whose tail may be
// padding, the rest (and calls below 1024 samples) on k_svf_cascade_short.  nSamples: any number.
// t.tp: one TpBandTables (host_design.hpp, kSvfTpTableDoubles = 600 doubles) per (stream, band): for each chunk length LC in
// kSvfTpLc ({16, 8}): Mk[6][4] = A^(LC 2^k), Mw[4] = A^(64 LC), P[64][4] = A^(LC (c+1)); then the 16-sample chunk's end-state
// map e[2][16] = A^(15-k) B.
// chain / chainSpans / chainGrid: chained spans for engines whose channels do not fill whole rounds of the workgroups the chip
// holds of the span kernel (chainGrid = 2 per CU): the (span, channel) pairs of a call are dealt to chainGrid workgroups, a band's state is
// handed from span to span through `chain` (svf_chain_bytes(channels, largest call) bytes, zero-initialised once,
// chainSpans = svf_chain_spans(largest call); used by one launch at a time).  chainSpans = 0: one workgroup per channel;
// `chain` (svf_chain_bytes(channels, 0) bytes, zero-initialised once; may be nullptr) then only holds the arrival counters by
// which the two workgroups of a CU take turns at raised priority.
void launch_svf_cascade_tp(hipStream_t stream, const double* in, double* out, int64_t chStride, int nCh,
                           int nSamples, CascadeTables t, void* chain = nullptr, int chainSpans = 0,
                           int chainGrid = 0);
size_t svf_chain_bytes(int nCh, int maxSamples);
int svf_chain_spans(int maxSamples);

// Processor-level dry/wet stage (ConvolverProcessor::process): out = sanitize(wet) * wetG + dryDelayed * dryG over one
// range of a call.  The dry signal is read from the delay ring ([nCh][ringSize], the call's input already written at
// absolute position pos0 = position of the range's first sample) dNew[stream] samples back; the first xLen[stream]
// samples are cross-faded from the delay dOld[stream] with the gains xGains[stream][i] (latency change); gains:
// [streams][2] = {wetG, dryG}; rampLen / rampGains: per-sample mix gains of the first samples of the CALL (rampOff =
// offset of this range in the call).
void launch_convproc_mix(hipStream_t stream, const double* wet, double* out, int64_t chStride, int nCh, int nSamples,
                         const double* gains, const double* ring, int ringSize, long long pos0, const int* dNew,
                         const int* dOld, const int* xLen, const double* xGains, int xCap, int wetValid,
                         const int* rampLen = nullptr, const double* rampGains = nullptr, int rampCap = 0, int rampOff = 0,
                         const int* wetOn = nullptr);       // wetOn[stream] == 0: that stream's convolver rests (delayed dry only)
void launch_ring_regrow(hipStream_t stream, const double* oldRing, int oldSize, double* newRing, int newSize, long long end,
                        int nCh);

// EQ AGC (EQProcessor::processAGC): per-callback-block RMS in the reference's accumulation order, then envelopes /
// gain per block (one thread per stream) and the linear gain ramp with the reference's incremental-add pattern.
// rms: [nCh][T]; state: [S][3] = envIn, envOut, gain; gains: [S][T][2] = start gain, per-sample increment.
void launch_agc_block_rms(hipStream_t stream, const double* x, int64_t chStride, int nCh, int B, int T, double* rms);
void launch_agc_apply(hipStream_t stream, double* data, int64_t chStride, int S, int B, int T, const double* rmsIn,
                      const double* rmsOut, double* state, const int* agcOn, double* gains, double bAtt, double bRel,
                      double bSm);

// applyGainRamp_AVX2 for the streams flagged in `on`: gains [S][T][2] = start gain, per-sample increment per callback
void launch_gain_ramp(hipStream_t stream, double* data, int64_t chStride, int S, int B, int T, const double* gains,
                      const int* on);

// FilterSpec tail layers at the reference's partition size: input accumulation, delay-line write, delay-line read-add
void launch_rows_copy(hipStream_t stream, const double* src, int64_t srcStride, int64_t srcOff, double* dst,
                      int64_t dstStride, int64_t dstOff, int n, int nCh);
void launch_ring_put(hipStream_t stream, const double* z, int64_t zStride, int n, double* ring, int ringSize,
                     long long pos, int nCh);
// Layered mode with the reader's additions inside the layer-0 inverse transform: the schedule first (launch_tail_schedule),
// then launch_rfft_inv_ols_tail writes out = layer-0 convolution + what the reader adds (from layerOut / the rings), then
// launch_tail_append stores what later calls may still read into the rings.
void launch_rfft_inv_ols_tail(hipStream_t stream, const double2* Y, double* out, int64_t chStride, FftTables tw, int P, int nCh,
                              int T, double2* scratch, const double* layerOut, const double* tailRing, int tailRingSize,
                              const void* tailState, const long long* sched, int nCallbacks, int B, int nTail, double g1, double g2);
void launch_tail_append(hipStream_t stream, const void* state, const double* layerOut, double* ring, int nCh, int nSamples,
                        int ringSlots, int nTail);
// replay of the delay-line reader for the T callbacks of a call (state: 4 long long; sched: [nTail][T], -1 = skip)
void launch_tail_schedule(hipStream_t stream, void* state, long long* sched, int T, int B, int nTail, int pl1, int ol1, int d1,
                          int pl2, int ol2, int d2);

// Plan groups (engine_native.cpp): chMap[local channel] = row of the call's buffers (-1 = unused slot); q = chunk length
// (one Add / Get pair of the reference per chunk); pos / cnt / sched: per chunk, replayed on the host.
// up to three layers' accumulators in one pass over the input
// tabDst / tab / nTab: a small table (<= kGatherTabMax entries) that rides along as kernel arguments and is stored to tabDst by
// the launch -- the call's chunk schedule of a plan group without a host -> device copy of its own
constexpr int kGatherTabMax = 64;
void launch_rows_gather_multi(hipStream_t stream, const double* src, int64_t srcStride, const int* chMap, int nLayers,
                              double* const* dst, const int64_t* dstStride, const int64_t* dstOff, int n, int nCh,
                              long long* tabDst = nullptr, const long long* tab = nullptr, int nTab = 0);
// Get() of a call in one pass over the members' output rows.  ring0 != nullptr: out = layer 0's ring read chunk by chunk
// (cnt[chunk] samples from pos[chunk], zero-filled to the chunk's end), every sample stored; ring0 == nullptr: out is read, and a
// sample is stored only where a tap is scheduled for its chunk.  Then tap a and tap b are added, in that order; either may be empty.
void launch_ring_chunks(hipStream_t stream, double* out, int64_t outStride, const int* chMap, int n, int q, const double* ring0,
                        int ringSize0, const long long* pos, const long long* cnt, RingTap a, RingTap b, int nCh);

// EQ bypass cross-fade for the streams flagged in `on`: out = out * g + dry * (1 - g); g = gains[s][i] for i < len[s], gEnd[s] after
void launch_bypass_blend(hipStream_t stream, double* out, int64_t outStride, const double* dry, int64_t dryStride, int n,
                         int nCh, const int* on, const int* len, const double* gEnd, const double* gains, int cap);
// silent[stream][callback] = no sample of the stream's two channels above 1e-8 in that callback block
void launch_block_silence(hipStream_t stream, const double* x, int64_t chStride, int B, int T, int S, int* silent);
// data[c][i] *= gain[c / 2] (streams with gain exactly 1 are left alone)
void launch_rows_scale(hipStream_t stream, double* data, int64_t stride, int n, int nCh, const double* gain);

// direct head: time-domain FIR of the first <= 32 taps over [history | block] into dout ([nCh][n]); then out += dout
// wetOn[stream] == 0: that stream's head rests (zero output, history kept)
void launch_direct_head(hipStream_t stream, const double* in, int64_t inStride, int n, const double* irRev, const int* taps,
                        const int* irSlot, const double* histOld, double* histNew, double* dout, int nCh,
                        const int* wetOn = nullptr);
void launch_rows_add(hipStream_t stream, double* out, int64_t outStride, const double* add, int n, int nCh);

// ---- half-band oversampler (os_kernels.hip)
// per stream: flags[4] = corruption pending, consecutive auto-clears, hard fallback, silenced in this down call;
// counts[2] = corruption events, auto-clears
struct OsStageArgs {
    const double* in; int64_t inStride;          // [nCh] rows
    double* out; int64_t outStride;
    const double* histOld; double* histNew;      // [nCh][keep] current / next history (ping-pong)
    int keep;
    const double* coef;                          // [convCount] device
    int convCount;                               // 16 .. 512, a power of two
    double centerCoeff;
    int centerOffset;                            // up: centerDelayInput; down: centerTap
    int n;                                       // input-rate outputs per channel: up = input samples, down = output samples
    int nCh;
    int* flags;
    unsigned long long* counts;
};
// the histories a down call's prologue clears / tests: current up and down history of every stage
struct OsHistories {
    double* up[3];
    double* down[3];
    int upKeep[3];
    int downKeep[3];
};
bool os_conv_count_supported(int convCount);
// interpolateStage for every channel: out[c][2n], out[c][2n + 1] from in[c][n]
void launch_os_interp(hipStream_t stream, const OsStageArgs& a);
// decimateStage for every channel: out[c][n] from in[c][2n]; nonSilent[c] == 0 takes the silence path; a nonzero output
// sets nonSilentNext[c] (the next, lower stage's input test; may be null)
void launch_os_decim(hipStream_t stream, const OsStageArgs& a, const int* nonSilent, int* nonSilentNext);
// processDown's per-stream prologue (auto-clear, hard fallback, clearAllStages) + nonSilent[stage][c] = history test
void launch_os_down_state(hipStream_t stream, const OsHistories& hs, int nStages, int nStreams, int* flags,
                          unsigned long long* counts, int* nonSilent);
// nonSilent[c] |= any |in[c][0..m)| > 1e-20
void launch_os_scan(hipStream_t stream, const double* in, int64_t stride, int m, int nCh, int* nonSilent);

// ---- meters (meter_kernels.hip): LoudnessMeter and TruePeakDetector on a call's base-rate rows, one record per callback
// K-weighting of every channel: chSum / chPeak [nCh][cbCap] = sum of squares and peak of callback k (cb samples, the last one of
// a ragged call shorter); tab = two sections of kMeterSectionDoubles; state [nCh][8] carried across calls
void launch_meter_kweight(hipStream_t stream, const double* in, int64_t stride, int n, int cb, int nCh, const double* tab,
                          double* state, double* chSum, double* chPeak, int cbCap);
// tp[stream][k] (bit pattern of a double >= 0, zeroed by the caller) = max |4x interpolated sample| of callback k over both
// channels; n is a multiple of cb, cb >= 8; hist [nCh][32] = the last scrubbed inputs, ping-pong; coef0 [32], coef1 [16]
void launch_meter_true_peak(hipStream_t stream, const double* in, int64_t stride, int n, int cb, int nCh, const double* histOld,
                            double* histNew, const double* coef0, const double* coef1, unsigned long long* tp, int cbCap);
struct MeterFinishArgs {
    int flags;                                   // CPQ_METER_*
    int n, cb, nCb;                              // samples and callbacks of the call
    int nStore;                                  // the first nStore callbacks find room in the ring
    int cbCap, ringSize;
    unsigned long long write0, index0;           // ring write counter and blockCounter before the call
    const double* chSum; const double* chPeak;
    const unsigned long long* tp;
    double* hold;                                // [streams] peakHold
    cpq_meter_block* ring;                       // [streams][ringSize]
};
void launch_meter_finish(hipStream_t stream, const MeterFinishArgs& a, int nStreams);

// ---- output stage (out_kernels.hip): DSPCore::processOutputDouble's base-rate steps on rows [nCh][n]; in and out may be the same
// DC blocker (tab = two sections of kOutSectionDoubles, dcState [nCh][2] carried across calls, cb = callback length: the state
// guards sit at the callback ends) and / or the headroom multiply with the scrub; nothing is launched when both are off
void launch_out_pre(hipStream_t stream, const double* in, int64_t inStride, double* out, int64_t outStride, int n, int cb, int nCh,
                    bool dcBlock, bool headroom, const double* tab, double* dcState);
// SimplePeakLimiter (env [nStreams] carried across calls) and / or the clamp; nothing is launched when both are off
void launch_out_post(hipStream_t stream, const double* in, int64_t inStride, double* out, int64_t outStride, int n, int nStreams,
                     bool limiter, bool clamp, double release, double* env);

// ---- soft clipper (softclip_kernels.hip): softClipBlockAVX2 in place on rows [nCh][n], callbacks of cb samples (the last one
// of the call shorter); channel c reads row c / 2 of tab ([streams][kSoftClipTabDoubles], softclip_design.hpp), a row whose first
// entry is 0 leaves its stream's rows alone
void launch_soft_clip(hipStream_t stream, double* data, int64_t stride, int n, int cb, int nCh, const double* tab);

// ---- dither stage (dither_kernels.hip): headroom, the 4- or 15-tap or the 9th-order lattice noise shaper and (scrub) the scrub
// on rows [nCh][n]; in and out may be the same rows.  err [kDitherMaxOrder][nCh] (tap k of channel c at k * nCh + c, k = 0 the
// newest; the lattice's states in rows 0 .. 8) and rng [4][nCh] are carried across calls.  order: 4, 16 or kLatticeOrder, which
// reads coef [kLatticeOrder][nCh] (the channel's own reflection coefficients) and not p.c; false: no kernel for that order.
constexpr int kDitherTile = CPQ_DITHER_TILE;    // samples of a row a wave stages in LDS at a time
struct DitherParams {
    double c[kDitherMaxOrder];
    double scale, invScale, maxV;               // 2^-(bits-1), 2^(bits-1), 1 - scale
    double headroom;                            // kOutHeadroom or 1.0
    int scrub;
};
bool launch_dither(hipStream_t stream, const double* in, int64_t inStride, double* out, int64_t outStride, int n, int nCh, int order,
                   const DitherParams& p, const double* coef, double* err, unsigned long long* rng);

// ---- packed PCM converters (pcm_kernels.hip): cpq_pcm_format x cpq_pcm_layout <-> fp64 rows [2 nStreams][n]
constexpr int kPcmTile = 4096;     // samples of the packed side per workgroup: 4096 of a planar row, 2048 stereo frames
// pcm aligned to its element (S24: any byte), rows to 8 bytes; sanitizeCb > 0: CPQ_PCM_SANITIZE with callbacks of that many
// samples (the last one of a row shorter when n is no multiple).  false: no kernel for that format.
bool launch_pcm_unpack(hipStream_t stream, const void* pcm, int format, int layout, double* rows, int n, int nStreams, int sanitizeCb);
bool launch_pcm_pack(hipStream_t stream, const double* rows, void* pcm, int format, int layout, int n, int nStreams);

// ---- quantizer (quant_kernels.hip): rows [nCh][n] at inStride, times gain[row / 2], through the shaper of `order` (as
// launch_dither: err, rng and coef carried the same way; p.headroom and p.scrub are not read: 1.0, none), packed at the width of
// format (CPQ_PCM_S16 / S24 / S32) into pcm: planar, channel r's row at r * pitch bytes; interleaved, stream s's at s * pitch.
// pcm and pitch aligned to the element (S24: any byte); one launch.  false: no kernel for that order, format or layout.
struct QuantLaunch {
    int n, nCh, order, format, layout;
    int64_t inStride, pitch;
};
bool launch_quantize(hipStream_t stream, const double* in, void* pcm, const QuantLaunch& a, const DitherParams& p, const double* gain,
                     const double* coef, double* err, unsigned long long* rng);

// ---- shaper scorer (score_kernels.hip): NoiseShaperLearner::evaluateCandidateMapped for many learners and candidates at once.
// Rows are kScoreLen doubles.  Nothing here checks an index: every table below is built by engine_score.cpp from validated counts.
// one lattice chain (a lane): segment row read, error row written, coefficient set [9], generator start [4]
struct ScoreChain { int src, dst, coef, rng; };
// seg rows -> err rows: a fresh LatticeNoiseShaper (p: scale, invScale, maxV, headroom) over every chain, err = yq - x * headroom
void launch_score_lattice(hipStream_t stream, const double* seg, double* err, const ScoreChain* chains, int nChains, const double* coef,
                          const unsigned long long* rng, const DitherParams& p);
// levelled segment rows of one learner: seg[row][i] = recent[row & 1][start[row >> 1] + i] * gain[row >> 1]; recent rows of
// `stride` doubles
void launch_score_level(hipStream_t stream, const double* recent, int64_t stride, const int* start, const double* gain, double* seg,
                        int nSegments);
// the per-bin tables of ScoreTables on the device, twiddles exp(-2 pi i k / 4096), k < 2048
struct ScoreDeviceTables {
    const double *weight, *bark, *athDb, *athPow, *width, *thrSpread, *spreadTonal, *spreadNoise;
    const int *band, *range, *bandStart;
    const double2* tw;
    int flatStart, flatEnd, highStart, ultraStart;
    double ultraShare, flatWeight, hfWeight, weightSum;
};
// one evaluation (a workgroup): rows 2 row and 2 row + 1 of `rows` are L and R; thr: the segment's masking thresholds row
// (thresholds mode: the row written); slot: where parts and blended land; alpha: the level's blend factor
struct ScoreEval { int row, thr, slot; double alpha; };
// thresholdsOnly: precomputeMaskingThresholds of segment rows (thr written).  Otherwise MklFftEvaluator::evaluate of error rows:
// parts[slot] and blended[slot] = alpha * sqrt(composite / 4096) * 1000 + (1 - alpha) * rms * 1000
void launch_score_spectrum(hipStream_t stream, const double* rows, double* thr, const ScoreEval* evals, int nEvals,
                           const ScoreDeviceTables& t, cpq_score_parts* parts, double* blended, bool thresholdsOnly);
// per (learner, candidate) pair: state 1 -> CPQ_SCORE_UNSTABLE, no segments or no weight -> DBL_MAX, else the level-weighted mean
// of the level means of blended[pair][16] (segments in evaluation order), counts [learner][4], in the reference's order
void launch_score_reduce(hipStream_t stream, const double* blended, const int* counts, const int* state, int nLearners, int nCand,
                         const double* levelWeights, double* scores);

// ---- IR sample-rate conversion (resample_kernels.hip): the polyphase filter taps [L][T] over a batch of rows of one source rate.
// x and y hold the rows back to back; row r reads x[inOff ... inOff + n) and writes y[outOff ... outOff + nOut).  A workgroup
// takes one tile: outputs j0 ... j0 + resampleTile() - 1 of tiles[block].row (cut at nOut).  Nothing here checks an index: the
// tables are engine_resample.cpp's, built from validated lengths.
constexpr int kResampleTileMax = 256;       // outputs a workgroup takes while M <= 8 L; 64 beyond, so that the stage fits LDS
constexpr int kResampleChunk = 256;         // taps a workgroup stages the row for at a time
struct ResampleRow { long long inOff, outOff; int n, nOut; };
struct ResampleTile { int row, j0; };
int resampleTile(int L, int M);
int resampleSpan(int L, int M, int tile);   // input samples the first taps of a tile's outputs spread over
void launch_ir_resample(hipStream_t stream, const double* taps, int L, int M, int T, const double* x, double* y, const ResampleRow* rows,
                        const ResampleTile* tiles, int nTiles);

// ---- streaming sample-rate conversion of audio (resample_kernels.hip), the device object of cpq_src: the call src_device_plan.hpp
// states in `a`, over hist [channels][a.hBound] and the caller's rows.  launch_src_resample writes out[ch][0 ... a.nOut) and launches
// nothing for a call without outputs; launch_src_keep then moves the kept samples to the front of hist, and launches nothing where
// srcKeepMoves says nothing moves.  Both go to one stream, in that order.  Nothing here checks an index: `a` is engine_src.cpp's,
// built from a planned and validated call.
void launch_src_resample(hipStream_t stream, const double* taps, const double* hist, const double* in, double* out, const SrcLaunch& a);
void launch_src_keep(hipStream_t stream, double* hist, const double* in, const SrcLaunch& a);

// ---- minimum-phase conversion of IR rows (minphase_kernels.hip), launched as minphase_plan.hpp lists.  x and y hold the rows of a
// chunk back to back: row r reads x[off ... off + n) and writes y[off ... off + n); z is its complex scratch [rows][N] (four-step
// path only); flags[r] becomes non-zero where the row holds a non-finite value after the exponential or in its output.  Tables:
// roots = the 4096th roots (minphaseStageRoots), hi / lo = the two levels of the N-th roots (minphaseSplitRoots).  Nothing here
// checks an index: the tables and grids are engine_minphase.cpp's and engine_diag.cpp's, built from validated lengths.
struct MinphaseRow { long long off; int n, pad; };
struct MinphaseTables { const double2 *roots, *hi, *lo; };
void launch_minphase_small(hipStream_t stream, const double* x, double* y, const MinphaseRow* rows, int* flags, MinphaseTables t,
                           int log2n, long long nRows);
void launch_cfft_cols(hipStream_t stream, int op, double2* z, const double* x, double* y, const MinphaseRow* rows, int* flags,
                      MinphaseTables t, int log2n1, int log2n2, long long nRows);
// scale multiplies what kRowsInv stores (1 / N when the row pass is the whole transform, log2n1 == 0)
void launch_cfft_rows(hipStream_t stream, int op, double2* z, int* flags, MinphaseTables t, int log2n1, int log2n2, long long nRows,
                      double scale);

// ---- programme loudness (prog_kernels.hip), the object cpq_loudness: the call prog_plan.hpp states in `c`, over rows [2 streams] of
// c.stride doubles.  tab = the meters' two section tables; state [2 streams][8] and part [2 streams] (the partial hop sum of a
// channel) are carried across calls; hops [streams][c.maxHops].  launch_prog_finish writes one ProgRecord per stream from the
// first f.nHops hop sums.  Nothing here checks an index: `c` and `f` are engine_prog.cpp's, built from a planned and validated call.
void launch_prog_hops(hipStream_t stream, const double* in, const ProgCall& c, const double* tab, double* state, double* part, double* hops);
void launch_prog_finish(hipStream_t stream, const double* hops, const ProgFinish& f, int nStreams, ProgRecord* out);
// true peak per programme: c.rows rows of c.n samples; pk [c.rows][kPeakState] (history and the two running maxima) is read and
// written.  launch_prog_apply: out = in * gain[row / 2] over c.rows rows, gain [c.rows / 2] on the device; in may be out.
void launch_prog_peak(hipStream_t stream, const double* in, const PeakCall& c, double* pk);
void launch_prog_apply(hipStream_t stream, const double* in, const ApplyCall& c, const double* gain, double* out);

// ---- look-ahead true-peak limiter (lim_kernels.hip), the device object of cpq_limiter: the call lim_plan.hpp states in `a`, over
// hist [2 streams][a.hBound], gains [streams], the caller's rows in and out (which do not overlap) and part [streams][a.partStride].
// launch_lim_apply writes out[row][0 ... a.nOut) and one partial per tile; launch_lim_keep then moves the kept tail of u to the front
// of hist and folds the partials into tel [streams].  Both go to one stream, in that order.  Nothing here checks an index: `a` is
// engine_lim.cpp's, built from a planned and validated call.
void launch_lim_apply(hipStream_t stream, const double* hist, const double* gains, const double* in, double* out, LimPartial* part, const LimLaunch& a);
void launch_lim_keep(hipStream_t stream, double* hist, const double* gains, const double* in, const LimPartial* part, LimPartial* tel, const LimLaunch& a);


// ---- shaper learner (learn_kernels.hip): one generation of CmaEsOptimizer for every learner with active[learner] != 0, on states
// [nLearners] in place.  launch_learn_ask draws z, factors the covariance and stores z, candidates and mapped [nLearners][18][9],
// the clamped sets to coef [nLearners * 18][9] and the stability flags to flag [nLearners * 18] (the scorer's buffers for a call
// of 18 candidates).  launch_learn_tell runs update() and the best tracking on scores [nLearners * 18] and stores the sort to
// order [nLearners][18] and the generation's best score to history[learner * histStride + g].  Nothing here checks an index.
void launch_learn_ask(hipStream_t stream, cpq_learn_state* states, const int* active, int nLearners, double margin, bool stabilityCheck,
                      double* coef, int* flag, double* z, double* candidates, double* mapped);
void launch_learn_tell(hipStream_t stream, cpq_learn_state* states, const int* active, int nLearners, const cpq_learn_params& p,
                       const double* candidates, const double* mapped, const double* scores, int* order, double* history, int histStride,
                       int g);

}  // namespace cpq
