"""Times the device object of cpq_src -- 512 channels, calls of 512, 4096 and 65536 samples, 44100 -> 48000 and 96000 -> 48000:
the device-pointer entry (cpq_src_process_device) by events around --calls back-to-back calls on resident rows, the host-row
entry (cpq_src_process on the device object: upload, launches, download) by the clock and by its own events
(cpq_src_last_kernel_ms), and the host object (CPQ_SRC_HOST, one thread) on --host-channels channels, scaled to the channel count
(its time is linear in the channels).  These are the figures of RESULTS.md, "Streaming sample-rate conversion".

    python tools/src_bench.py [--channels 512] [--sizes 512 4096 65536] [--calls 20] [--host-channels 8] [--out profiles/src_bench.json]

Every stream is warmed with one call before it is timed, so that every timed call emits its steady share of outputs and reads a
full history.  Beside each time stands the call's algorithmic traffic over it -- the rows in, the rows out, the history read and
written once per channel; the taps are not counted, they stay in cache -- and the FMA rate, T fused multiply-adds per output,
against the MI355X's fp64 vector peak (39.3e12 FMA/s), as for k_ir_resample."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FMA_PER_S = 78.6e12 / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 4096, 65536])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-row-calls", type=int, default=3)
    ap.add_argument("--host-channels", type=int, default=8)
    ap.add_argument("--pairs", type=int, nargs="+", default=[44100, 48000, 96000, 48000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import convopeq_amd as amd

    rows = []
    for in_rate, out_rate in zip(a.pairs[0::2], a.pairs[1::2]):
        d = amd.resample_design(in_rate, out_rate)
        for size in a.sizes:
            x = np.random.default_rng(size).uniform(-0.5, 0.5, size=(a.channels, size))
            t = torch.from_numpy(x).cuda()

            # device rows: events around the calls, nothing waits in between
            dev = amd.StreamResampler(a.channels, in_rate, out_rate, size, device=True)
            out = torch.empty((a.channels, dev.max_out), dtype=torch.float64, device="cuda")
            first = dev.process_device(t, out=out).cpu().numpy()            # warm-up: the stream passes its latency
            counts = []
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(a.calls):
                counts.append(dev.process_device(t, out=out).shape[1])
            ev[1].record()
            torch.cuda.synchronize()
            device_ms = ev[0].elapsed_time(ev[1]) / a.calls
            n_out = float(np.mean(counts))

            # host rows through the device object
            dev = amd.StreamResampler(a.channels, in_rate, out_rate, size, device=True)
            assert np.array_equal(dev.process(x), first)
            wall, kernel = [], []
            for _ in range(a.host_row_calls):
                t0 = time.perf_counter()
                dev.process(x)
                t1 = time.perf_counter()
                wall.append((t1 - t0) * 1e3)
                kernel.append(dev.last_kernel_ms)

            # the host object on a few channels: the device's bits, and its time
            hc = min(a.host_channels, a.channels)
            ref = amd.StreamResampler(hc, in_rate, out_rate, size, host=True)
            assert np.array_equal(ref.process(x[:hc]), first[:hc])
            host = []
            for _ in range(a.host_row_calls):
                t0 = time.perf_counter()
                ref.process(x[:hc])
                t1 = time.perf_counter()
                host.append((t1 - t0) * 1e3)

            hist = d["T"] - 1                   # samples per channel read from and written to the history by a steady call
            bytes_call = 8.0 * a.channels * (size + n_out + hist + min(hist, size))
            fmas = float(a.channels) * n_out * d["T"]
            row = {"in_rate": in_rate, "out_rate": out_rate, "channels": a.channels, "samples": size, "L": d["L"], "M": d["M"], "T": d["T"],
                   "outputs_per_call": n_out, "calls": a.calls, "algorithmic_bytes": bytes_call, "fma": fmas,
                   "device_rows_ms": device_ms, "device_rows_gb_per_s": bytes_call / (device_ms * 1e-3) / 1e9,
                   "device_rows_fma_per_s": fmas / (device_ms * 1e-3),
                   "host_rows_call_ms": float(np.median(wall)), "host_rows_kernel_ms": float(np.median(kernel)),
                   "host_rows_gb_per_s": bytes_call / (float(np.median(wall)) * 1e-3) / 1e9,
                   "host_object_channels_timed": hc,
                   "host_object_ms_per_channel": float(np.median(host)) / hc}
            row["device_rows_fraction_of_fp64_vector_peak"] = row["device_rows_fma_per_s"] / PEAK_FMA_PER_S
            row["host_object_ms_scaled"] = row["host_object_ms_per_channel"] * a.channels
            row["host_object_gb_per_s"] = bytes_call / (row["host_object_ms_scaled"] * 1e-3) / 1e9
            row["channel_samples_per_s_device_rows"] = a.channels * size / (device_ms * 1e-3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
