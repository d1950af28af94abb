"""Kernel times of the true peak per programme and of the gain (cpq_loudness: k_prog_peak, k_prog_apply) at the bench shape: 256
streams x 524288 samples at 48 kHz, device rows, beside k_prog_hops on the same rows in the same session.  An object without the
switch times k_prog_hops; one with it times k_prog_hops + k_prog_peak, which run one behind the other on one stream, so
k_prog_peak is the difference, taken pass by pass with the two objects alternating.  Device events around the calls, median of
--repeats after one warm-up pass.  Prints the two floors of k_prog_peak from BASELINE.md's denominators (8 TB/s of HBM; the fp64
vector rate of 78.6 TFLOP/s counts a fused multiply-add as two, and this kernel fuses nothing: 39.3 T operations/s) and one JSON
line.  For the kernels' own times, run it under a kernel trace."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12
FP64_OPS_PER_S = 78.6e12 / 2.0
OPS_PER_SAMPLE = 4 * 12 + 4 * 11                    # four phases: 12 multiplies and 11 adds each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    import convopeq_amd as amd
    S, n, rate = a.streams, a.samples, 48000
    rows = 0.1 * torch.randn((2 * S, n), dtype=torch.float64, device="cuda")
    seconds = (a.repeats + 2) * n / rate + 1
    plain = amd.ProgrammeLoudness(S, rate, seconds)
    peak = amd.ProgrammeLoudness(S, rate, seconds, true_peak=True)
    gains = np.ones(S)                              # in place, so that every pass reads the same rows
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    hops_ms, both_ms, apply_ms = [], [], []
    for i in range(a.repeats + 1):
        torch.cuda.synchronize()
        ev[0].record()
        plain.process_device(rows)
        ev[1].record()
        peak.process_device(rows)
        ev[2].record()
        peak.apply_device(gains, rows)
        ev[3].record()
        torch.cuda.synchronize()
        if i:                                       # the first pass warms up
            hops_ms.append(ev[0].elapsed_time(ev[1]))
            both_ms.append(ev[1].elapsed_time(ev[2]))
            apply_ms.append(ev[2].elapsed_time(ev[3]))
    tp = max(max(p["true_peak"]) for p in peak.peaks())
    plain.close()
    peak.close()
    peak_ms = [b - h for b, h in zip(both_ms, hops_ms)]
    row_bytes = 2.0 * S * n * 8.0
    hbm_floor_ms = 1e3 * row_bytes / HBM_BYTES_PER_S
    valu_floor_ms = 1e3 * 2.0 * S * n * OPS_PER_SAMPLE / FP64_OPS_PER_S
    med = statistics.median
    out = {"streams": S, "samples": n, "rate": rate, "k_prog_hops_ms": med(hops_ms), "hops_and_peak_ms": med(both_ms),
           "k_prog_peak_ms": med(peak_ms), "k_prog_apply_ms": med(apply_ms), "peak_over_hops": med(peak_ms) / med(hops_ms),
           "peak_hbm_floor_ms": hbm_floor_ms, "peak_valu_floor_ms": valu_floor_ms, "peak_over_valu_floor": med(peak_ms) / valu_floor_ms,
           "peak_over_hbm_floor": med(peak_ms) / hbm_floor_ms, "apply_gb_per_s": 2.0 * row_bytes / med(apply_ms) / 1e6,
           "largest_true_peak": tp, "k_prog_hops_ms_all": hops_ms, "hops_and_peak_ms_all": both_ms, "k_prog_apply_ms_all": apply_ms}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
