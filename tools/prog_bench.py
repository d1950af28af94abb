"""Kernel times of the programme loudness (cpq_loudness) at the bench shape: 256 streams x 524288 samples at 48 kHz, device rows.
Prints k_prog_hops and k_prog_finish (device events around the calls, median of --repeats) beside k_meter_kweight on the same
rows (the engine's profiler), and their ratio, as one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import torch
    import convopeq_amd as amd
    S, n, rate = a.streams, a.samples, 48000
    rows = 0.1 * torch.randn((2 * S, n), dtype=torch.float64, device="cuda")
    obj = amd.ProgrammeLoudness(S, rate, (a.repeats + 2) * n / rate + 1)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    hops_ms, finish_ms = [], []
    for i in range(a.repeats + 1):
        torch.cuda.synchronize()
        ev[0].record()
        obj.process_device(rows)
        ev[1].record()
        torch.cuda.synchronize()
        ev[1].record()
        obj.finish()                                # launch, 16 KB download, synchronise
        ev[2].record()
        torch.cuda.synchronize()
        if i:                                       # the first pass warms up
            hops_ms.append(ev[0].elapsed_time(ev[1]))
            finish_ms.append(ev[1].elapsed_time(ev[2]))
    obj.close()
    # k_meter_kweight on the same rows: one engine call of 524288 samples, loudness records only
    B = 512
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=1024, max_blocks_per_call=n // B, sample_rate=float(rate))
    eng.set_metering(amd.CPQ_METER_LOUDNESS)
    eng.profile_enable(True)
    lib = amd._capi.load()
    import ctypes as C
    for i in range(a.repeats + 1):
        if i == 1:
            eng.profile_reset()
        rc = lib.cpq_meter_process_device(eng._h, C.c_void_p(rows.data_ptr()), n)
        assert rc == 0, rc
        torch.cuda.synchronize()
        eng.meter_read_blocks()
    meter = eng.profile_read().get("k_meter")
    eng.close()
    meter_ms = meter[1] / meter[0]                  # k_meter_kweight and the records' k_meter_finish of one call
    out = {"streams": S, "samples": n, "rate": rate, "k_prog_hops_ms": statistics.median(hops_ms),
           "finish_call_ms": statistics.median(finish_ms), "k_meter_ms": meter_ms,
           "hops_over_meter": statistics.median(hops_ms) / meter_ms, "k_prog_hops_ms_all": hops_ms}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
