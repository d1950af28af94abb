"""Times cpq_ir_resample_batch -- 256 stereo IRs x 131072 samples, 44100 -> 48000 and 96000 -> 48000 -- on the device: the whole
call (upload, launch, download, tail trim) and the kernel alone by the call's own events (cpq_ir_resample_last_kernel_ms), next
to cpq_ir_resample_host on this machine's CPU share (timed on --host-irs IRs and scaled to the batch: the host path's time is
linear in the rows).  These are the figures of RESULTS.md, "IR sample-rate conversion".

    python tools/resample_bench.py [--irs 256] [--samples 131072] [--calls 3] [--warmup 1] [--host-irs 8] [--out profiles/resample_bench.json]

Every IR is seeded noise of its own level under an exponential decay of 12 time constants: the rows differ, and the trim keeps
them whole (the tail stays above -160 dB), so every output is downloaded and copied.
The FMA rate counts T fused multiply-adds per output and is set against the MI355X's fp64 vector peak (78.6 TFLOP/s = 39.3e12
FMA/s)."""
import argparse
import ctypes as C
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
    ap.add_argument("--irs", type=int, default=256)
    ap.add_argument("--samples", type=int, default=131072)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-irs", type=int, default=8)
    ap.add_argument("--pairs", type=int, nargs="+", default=[44100, 48000, 96000, 48000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import convopeq_amd as amd
    from convopeq_amd import _capi as K

    lib = K.load()
    rows = []
    for in_rate, out_rate in zip(a.pairs[0::2], a.pairs[1::2]):
        d = amd.resample_design(in_rate, out_rate)
        n_out = -((-a.samples * d["L"]) // d["M"])
        decay = np.exp(-np.arange(a.samples) / (a.samples / 12.0))
        data = [np.ascontiguousarray(np.random.default_rng(i).standard_normal((2, a.samples)) * decay * (0.1 + 0.001 * i)) for i in range(a.irs)]
        bufs = (K.IrBuffer * a.irs)(*[K.IrBuffer(2, a.samples, float(in_rate), x.ctypes.data_as(K.c_double_p)) for x in data])
        ptrs = (C.POINTER(K.IrBuffer) * a.irs)(*[C.pointer(bufs[i]) for i in range(a.irs)])
        outs = (K.IrBuffer * a.irs)()
        wall, kernel = [], []
        first = None
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            rc = lib.cpq_ir_resample_batch(ptrs, a.irs, float(out_rate), 0, outs)
            t1 = time.perf_counter()
            assert rc == 0, lib.cpq_last_error(None).decode()
            if first is None:
                first = np.ctypeslib.as_array(outs[0].data, shape=(outs[0].n_channels, outs[0].n_samples)).copy()
            kept = [outs[j].n_samples for j in range(a.irs)]
            for j in range(a.irs):
                lib.cpq_ir_buffer_free(C.byref(outs[j]))
            if i >= a.warmup:
                wall.append((t1 - t0) * 1e3)
                kernel.append(lib.cpq_ir_resample_last_kernel_ms())
        host = []
        h = K.IrBuffer()
        for j in range(min(a.host_irs, a.irs)):
            t0 = time.perf_counter()
            rc = lib.cpq_ir_resample_host(C.byref(bufs[j]), float(out_rate), 0, C.byref(h))
            t1 = time.perf_counter()
            assert rc == 0
            if j == 0:
                got = np.ctypeslib.as_array(h.data, shape=(h.n_channels, h.n_samples))
                assert got.shape == first.shape and np.array_equal(got, first)          # the device's bits
            lib.cpq_ir_buffer_free(C.byref(h))
            host.append((t1 - t0) * 1e3)
        fmas = 2.0 * a.irs * n_out * d["T"]
        row = {"in_rate": in_rate, "out_rate": out_rate, "irs": a.irs, "samples": a.samples, "L": d["L"], "M": d["M"], "T": d["T"],
               "outputs_per_row": n_out, "kept_min": int(min(kept)), "kept_max": int(max(kept)), "fma": fmas, "calls": a.calls,
               "host_cpus": len(os.sched_getaffinity(0)), "host_irs_timed": len(host)}
        for name, v in (("call_ms", wall), ("kernel_ms", kernel)):
            row[name] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        row["host_ms_per_ir"] = float(np.median(host))
        row["host_ms_batch_scaled"] = row["host_ms_per_ir"] * a.irs
        row["kernel_fma_per_s"] = fmas / (row["kernel_ms"]["median"] * 1e-3)
        row["kernel_fraction_of_fp64_vector_peak"] = row["kernel_fma_per_s"] / PEAK_FMA_PER_S
        row["host_fma_per_s"] = fmas / a.irs / (row["host_ms_per_ir"] * 1e-3)
        row["call_speedup_over_host"] = row["host_ms_batch_scaled"] / row["call_ms"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
