"""Times the device object of cpq_quantizer on resident rows against the engine's two calls for the same bytes: one launch of
k_quantize (cpq_quantizer_last_kernel_ms, events around the launch) beside cpq_dither_process_device + cpq_pcm_pack_device on an
engine with the same shaper, depth and rate (events around the pair), at 256 streams x 48000 samples, S16 and S24, all three
shapers.  These are the figures of RESULTS.md, "Quantizer".

    python tools/quant_bench.py [--streams 256] [--samples 48000] [--reps 5] [--out profiles/quant_bench.json]

Both sides are warmed with one call of the timed shape, and that first call's bytes are compared: at gain 1.0 they must be equal.
The timed calls alternate between the two sides.  A channel is one dependent chain, so the time follows the samples per channel
and hardly the stream count."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rate", type=float, default=48000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import convopeq_amd as amd
    from convopeq_amd import _capi as K

    S, n = a.streams, a.samples
    block = 512
    eng = amd.BatchedEngine(S, block_size=block, max_ir_len=1024, max_blocks_per_call=(n + block - 1) // block, sample_rate=a.rate,
                            call_mode=amd.CPQ_CALLS_ANY)
    gen = torch.Generator(device="cuda").manual_seed(S)
    rows = 0.25 * torch.randn((2 * S, n), dtype=torch.float64, device="cuda", generator=gen)
    shaped = torch.empty_like(rows)
    results = []
    for shaper, name in ((K.CPQ_DITHER_FIXED4, "fixed4"), (K.CPQ_DITHER_FIXED15, "fixed15"), (K.CPQ_DITHER_ADAPTIVE9, "adaptive9")):
        for fmt, fname, bits in ((K.CPQ_PCM_S16, "s16", 16), (K.CPQ_PCM_S24, "s24", 24)):
            eng.set_dither(K.CPQ_DITHER_OFF)
            eng.set_dither(shaper, bits)                        # a change: errors cleared, reseeded
            q = amd.Quantizer(S, a.rate, shaper, bits, fmt, device=True)
            r, width = q.packed_shape(K.CPQ_PCM_INTERLEAVED, n)
            fused_out = torch.zeros((r, width), dtype=torch.uint8, device="cuda")
            two_out = torch.zeros((r, width), dtype=torch.uint8, device="cuda")

            def two_calls():
                eng.dither_process_device(rows.data_ptr(), shaped.data_ptr(), n)
                eng.pcm_pack_device(shaped.data_ptr(), two_out.data_ptr(), fmt, n, K.CPQ_PCM_INTERLEAVED)

            q.process_device(rows, K.CPQ_PCM_INTERLEAVED, fused_out)
            two_calls()
            torch.cuda.synchronize()
            equal = bool(torch.equal(fused_out, two_out))
            fused, two = [], []
            for _ in range(a.reps):
                q.process_device(rows, K.CPQ_PCM_INTERLEAVED, fused_out)
                fused.append(q.last_kernel_ms)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                two_calls()
                ev[1].record()
                torch.cuda.synchronize()
                two.append(ev[0].elapsed_time(ev[1]))
            results.append({"shaper": name, "format": fname, "bit_depth": bits, "streams": S, "samples": n, "layout": "interleaved",
                            "fused_ms": min(fused), "fused_ms_all": fused, "two_calls_ms": min(two), "two_calls_ms_all": two,
                            "fused_over_two_calls": min(fused) / min(two), "fused_us_per_sample": 1e3 * min(fused) / n,
                            "bytes_equal_first_call": equal})
            print(json.dumps(results[-1]))
            del q, fused_out, two_out
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    if not all(r["bytes_equal_first_call"] for r in results):
        sys.exit("the two paths disagree")


if __name__ == "__main__":
    main()
