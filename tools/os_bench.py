#!/usr/bin/env python3
"""os_bench.py -- throughput of the half-band oversampler kernels on one MI355X.  Prints ONE JSON line.

For F in {2, 4, 8} x {IIR, LinearPhase}: 256 stereo streams x 65536 base-rate samples per call through cpq_os_up_device
and cpq_os_down_device (buffers resident in HBM), kernel milliseconds from the engine's per-kernel event timing
(cpq_profile_*; the down figure includes its state and silence-scan kernels).  The fp64 FMA count is
sum over the stages i of conv_count_i * 2^i per base sample and channel, per direction (8x IIR: 448 up + 448 down);
TFLOP/s = 2 FMA / time, share of the fp64 vector peak (78.6 TF).  F = 2 runs stage 0 alone.

Then cpq_engine_process_block_device at 8x IIR (48 kHz base, 384 kHz inside, 4096-sample partitions): bench EQ preset,
a 4096-tap IR, 256 streams x 65536 base samples per call: step time and the oversampler's share of the kernel time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_VECTOR_PEAK_TFLOPS = 78.6


def fmas_per_base_sample(amd, factor, os_type):
    stages = {2: 1, 4: 2, 8: 3}[factor]
    return sum(amd.os_design_stage(i, os_type)[0]["conv_count"] * (1 << i) for i in range(stages))


def kernel_ms(eng, fn, steps):
    eng.profile_reset()
    for _ in range(steps):
        fn()
    prof = eng.profile_read()
    n, ms = prof.get("k_os_halfband", (0, 0.0))
    assert n == steps, (n, steps)
    return ms / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--base", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import convopeq_amd as amd
    if not torch.cuda.is_available():
        raise SystemExit("os_bench needs a GPU")
    S, nb = args.streams, args.base
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.uniform(-1.0, 1.0, (2 * S, nb))).cuda()
    result = {"streams": S, "base_samples_per_call": nb, "kernels": []}
    up = torch.empty((2 * S, nb * 8), dtype=torch.float64, device="cuda")
    down = torch.empty_like(x)
    for factor in (2, 4, 8):
        for os_type, tname in ((amd.CPQ_OS_IIR, "iir"), (amd.CPQ_OS_LINEAR_PHASE, "linear_phase")):
            eng = amd.BatchedEngine(S, block_size=4096, max_ir_len=4096, max_blocks_per_call=nb * factor // 4096,
                                    sample_rate=48000.0 * factor)
            eng.set_oversampling(factor, os_type)
            eng.profile_enable(True)
            u = up[:, :nb * factor].contiguous() if factor < 8 else up
            fu = lambda: eng.os_up_device(x.data_ptr(), u.data_ptr(), nb)             # noqa: E731
            fd = lambda: eng.os_down_device(u.data_ptr(), down.data_ptr(), nb)        # noqa: E731
            for _ in range(args.warmup):
                fu()
                fd()
            ms_up = kernel_ms(eng, fu, args.steps)
            ms_down = kernel_ms(eng, fd, args.steps)
            fmas = fmas_per_base_sample(amd, factor, os_type) * 2 * S * nb       # per direction
            row = {"factor": factor, "type": tname, "fma_per_base_sample_each_way": fmas_per_base_sample(amd, factor, os_type)}
            for d, ms in (("up", ms_up), ("down", ms_down)):
                tf = 2.0 * fmas / (ms * 1e-3) / 1e12
                row[d] = {"ms": round(ms, 4), "tflops": round(tf, 2), "frac_fp64_peak": round(tf / FP64_VECTOR_PEAK_TFLOPS, 3),
                          "floor_ms": round(2.0 * fmas / (FP64_VECTOR_PEAK_TFLOPS * 1e12) * 1e3, 4)}
            result["kernels"].append(row)
            eng.close()
            del u
    del up, down

    # the whole block at 8x IIR
    import oracle_lib as O
    nbc = nb
    eng = amd.BatchedEngine(S, block_size=4096, max_ir_len=4096, max_blocks_per_call=nbc * 8 // 4096, sample_rate=384000.0)
    eng.prepare_to_play(384000.0, nbc * 8)
    ir = O.gen_ir(4096)
    eng.set_impulse(amd.CPQ_ALL_STREAMS, ir, ir)
    po, pa = O.eq_params_bench(0.2), amd.eq_params_default()
    for i in range(20):
        b, o = pa.bands[i], po.bands[i]
        b.frequency, b.gain, b.q, b.enabled, b.type, b.channel_mode = o.frequency, o.gain, o.q, o.enabled, o.type, o.channelMode
    eng.set_eq_params(amd.CPQ_ALL_STREAMS, pa)
    eng.set_oversampling(8, amd.CPQ_OS_IIR)
    xin = x
    yout = torch.empty_like(xin)
    step = lambda: eng.process_device(xin.data_ptr(), yout.data_ptr(), nbc)     # noqa: E731
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / args.steps
    eng.profile_enable(True)
    eng.profile_reset()
    for _ in range(args.steps):
        step()
    prof = eng.profile_read()
    total = sum(ms for _, ms in prof.values()) / args.steps
    os_ms = prof["k_os_halfband"][1] / args.steps
    fmas = fmas_per_base_sample(amd, 8, amd.CPQ_OS_IIR) * 2 * 2 * S * nbc
    result["process_block_8x_iir"] = {
        "base_samples_per_call": nbc, "internal_samples_per_call": nbc * 8, "ir_taps": 4096, "step_ms": round(step_ms, 4),
        "kernel_ms_total": round(total, 4), "os_ms": round(os_ms, 4), "os_share_of_kernel_time": round(os_ms / total, 3),
        "os_floor_ms": round(2.0 * fmas / (FP64_VECTOR_PEAK_TFLOPS * 1e12) * 1e3, 4),
        "per_kernel_ms": {k: round(v[1] / args.steps, 4) for k, v in prof.items() if v[0]}}
    eng.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
