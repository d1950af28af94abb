"""Times the device object of cpq_limiter on resident rows: cpq_limiter_last_kernel_ms (events around k_lim_apply and k_lim_keep of
one call) at 256 streams x 524288 samples with W = 72 and at 64 streams with W = 1024, out of place.  The yardsticks stand beside
each time: cpq_loudness_apply_device on the same rows (events around --reps calls), and the HBM floor of 32 B per stereo sample
(both channels in, both out) at 8 TB/s.  These are the figures of RESULTS.md, "Look-ahead true-peak limiter".

    python tools/limiter_bench.py [--samples 524288] [--cases 256 72 64 1024] [--reps 5] [--out profiles/limiter_bench.json]

Every object is warmed with one call before it is timed, so that the timed call reads a full history.  One stream in eight carries
peaks above the ceiling, so that both branches of the required gain run; the time does not depend on the values otherwise."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--cases", type=int, nargs="+", default=[256, 72, 64, 1024], help="pairs: streams window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import convopeq_amd as amd

    rows = []
    for streams, window in zip(a.cases[0::2], a.cases[1::2]):
        gen = torch.Generator(device="cuda").manual_seed(streams + window)
        t = 0.2 * torch.randn((2 * streams, a.samples), dtype=torch.float64, device="cuda", generator=gen)
        t[::16, 1000::4001] = 2.5
        out = torch.empty_like(t)
        lim = amd.TruePeakLimiter(streams, a.rate, -1.0, window, device=True)
        lim.process_device(t, out)                              # warm-up: the history fills
        times = []
        for _ in range(a.reps):
            lim.process_device(t, out)
            times.append(lim.last_kernel_ms)
        lim.process_device(t, t.clone())
        tel = lim.telemetry()
        in_place = []
        for _ in range(2):
            scratch = t.clone()
            lim.process_device(scratch, scratch)
            in_place.append(lim.last_kernel_ms)                 # the launches alone: the copy in front of them is not in it

        loud = amd.ProgrammeLoudness(streams, a.rate, 60.0)
        gains = [0.9] * streams
        loud.apply_device(gains, t, out)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(a.reps):
            loud.apply_device(gains, t, out)
        ev[1].record()
        torch.cuda.synchronize()
        apply_ms = ev[0].elapsed_time(ev[1]) / a.reps

        floor_ms = 32.0 * streams * a.samples / HBM_BYTES_PER_S * 1e3
        best = min(times)
        rows.append({"streams": streams, "window": window, "samples": a.samples, "tile": 1024, "limiter_ms": best, "limiter_ms_all": times,
                     "limiter_in_place_kernels_ms": min(in_place), "apply_device_ms": apply_ms, "hbm_floor_ms": floor_ms,
                     "ratio_to_apply": best / apply_ms, "ratio_to_floor": best / floor_ms,
                     "limited_samples_stream0": tel[0]["limited_samples"], "min_gain_stream0": tel[0]["min_gain"]})
        print(json.dumps(rows[-1]))
        del t, out, lim, loud
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
