"""Times the bench-shape step (256 streams x 524288 samples, block 512, FFT partition 4096, conv + EQ, device entry point) with
metering off, loudness only and both meters, and reads the per-kernel times of the profiler.

    python tools/meter_bench.py [--streams 256] [--steps 5] [--warmup 2] [--out profiles/meter_bench.json]

Floors the meter kernels are set against: the loudness pass reads 8 B per sample and channel (2.1 GB at this shape); the
true-peak stages cost 2 * 33 + 2 * 2 * 17 = 134 FMAs per base-rate sample and channel as the reference writes them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ir-len", type=int, default=131072)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meter_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import convopeq_amd as amd
    import oracle_lib as O

    S, B, T = a.streams, 512, 1024
    n = B * T
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=a.ir_len, max_blocks_per_call=T, partition_size=4096)
    ir_l, ir_r = O.gen_ir(a.ir_len, stream=0, channel=0), O.gen_ir(a.ir_len, stream=0, channel=1)
    for s in range(S):
        eng.set_impulse(s, np.roll(ir_l, s), np.roll(ir_r, s))
    po, pa = O.eq_params_bench(0.2), amd.eq_params_default()
    for i in range(20):
        b, o = pa.bands[i], po.bands[i]
        b.frequency, b.gain, b.q, b.enabled, b.type, b.channel_mode = o.frequency, o.gain, o.q, o.enabled, o.type, o.channelMode
    eng.set_eq_params(amd.CPQ_ALL_STREAMS, pa)
    g = torch.Generator(device="cuda").manual_seed(1)
    d_in = 0.05 * torch.randn((2 * S, n), dtype=torch.float64, device="cuda", generator=g)
    d_out = torch.empty_like(d_in)
    torch.cuda.synchronize()
    result = {"streams": S, "samples_per_call": n, "block_size": B, "steps": a.steps, "warmup": a.warmup, "modes": {}}
    for name, flags in (("off", 0), ("loudness", amd.CPQ_METER_LOUDNESS), ("loudness+true_peak", amd.CPQ_METER_LOUDNESS | amd.CPQ_METER_TRUE_PEAK)):
        eng.set_metering(flags)
        eng.profile_enable(False)
        for _ in range(a.warmup):
            eng.process_device(d_in.data_ptr(), d_out.data_ptr(), n)
        eng.synchronize()
        if flags:
            eng.meter_read_blocks()
        times = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            eng.process_device(d_in.data_ptr(), d_out.data_ptr(), n)
            eng.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            if flags:
                eng.meter_read_blocks()
        eng.profile_enable(True)
        eng.profile_reset()
        eng.process_device(d_in.data_ptr(), d_out.data_ptr(), n)
        prof = {k: {"launches": v[0], "ms": v[1]} for k, v in eng.profile_read().items() if v[0]}
        if flags:
            eng.meter_read_blocks()
        result["modes"][name] = {"ms_per_step": sorted(times)[len(times) // 2], "ms_all": times, "kernels_ms_one_step": prof}
        print(name, result["modes"][name]["ms_per_step"], prof.get("k_meter"))
    eng.close()
    result["floors"] = {"loudness_bytes": 8 * 2 * S * n, "true_peak_fma": 134 * 2 * S * n}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"meter_bench": {k: v["ms_per_step"] for k, v in result["modes"].items()}}))


if __name__ == "__main__":
    main()
