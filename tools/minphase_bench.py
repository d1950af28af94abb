"""Times cpq_ir_minimum_phase_batch on the device -- 256 stereo IRs x 48000 taps (the bench's own library), 64 mono IRs x 2097152
taps (the largest legal size) and 2048 mono IRs x 1024 taps (the small kernel) -- the whole call (upload, launches, download) and
the launches alone by the call's own events (cpq_ir_minimum_phase_last_kernel_ms), next to the host path
cpq_ir_convert_to_minimum_phase on this machine's CPU (timed on --host-irs IRs and scaled to the batch: the host path's time is
linear in the rows).  These are the figures of RESULTS.md, "Minimum-phase conversion".

    python tools/minphase_bench.py [--shapes 256x2x48000 64x1x2097152 2048x1x1024] [--calls 3] [--warmup 1] [--host-irs 4] [--out profiles/minphase_bench.json]

GB/s is set against the bytes minphase_plan.hpp plans per row (minphaseRowTraffic): 16 n on the small path (the samples in and
out), 16 n + 8 * 16 N above it (five passes over the complex scratch, the first of which reads and the last of which writes
samples instead).  Every IR is seeded noise under an exponential decay with a unit first tap."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LOG2_LDS = 12


def row_traffic(n):
    lg = max(2, (4 * n - 1).bit_length())
    return lg, (16 * n if lg <= LOG2_LDS else 16 * n + 8 * (16 << lg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["256x2x48000", "64x1x2097152", "2048x1x1024"])
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-irs", type=int, default=4)
    ap.add_argument("--workspace", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from convopeq_amd import _capi as K

    lib = K.load()
    rows = []
    for shape in a.shapes:
        irs, ch, n = (int(v) for v in shape.split("x"))
        lg, per_row = row_traffic(n)
        decay = np.exp(-6.0 * np.arange(n) / n)
        data = []
        for i in range(irs):
            x = np.random.default_rng(i).uniform(-0.5, 0.5, (ch, n)) * decay
            x[:, 0] += 1.0
            data.append(np.ascontiguousarray(x))
        bufs = (K.IrBuffer * irs)(*[K.IrBuffer(ch, n, 48000.0, x.ctypes.data_as(K.c_double_p)) for x in data])
        ptrs = (C.POINTER(K.IrBuffer) * irs)(*[C.pointer(bufs[i]) for i in range(irs)])
        outs = (K.IrBuffer * irs)()
        status = (C.c_int32 * irs)()
        wall, kernel = [], []
        first = None
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            rc = lib.cpq_ir_minimum_phase_batch(ptrs, irs, a.workspace, outs, status)
            t1 = time.perf_counter()
            assert rc == 0 and not any(status), lib.cpq_last_error(None).decode()
            if first is None:
                first = np.ctypeslib.as_array(outs[0].data, shape=(ch, n)).copy()
            for j in range(irs):
                lib.cpq_ir_buffer_free(C.byref(outs[j]))
            if i >= a.warmup:
                wall.append((t1 - t0) * 1e3)
                kernel.append(lib.cpq_ir_minimum_phase_last_kernel_ms())
        host = []
        h = K.IrBuffer()
        for j in range(min(a.host_irs, irs)):
            t0 = time.perf_counter()
            rc = lib.cpq_ir_convert_to_minimum_phase(C.byref(bufs[j]), C.byref(h))
            t1 = time.perf_counter()
            assert rc == 0
            if j == 0:
                got = np.ctypeslib.as_array(h.data, shape=(ch, n))
                diff = float(np.abs(got - first).max())
            lib.cpq_ir_buffer_free(C.byref(h))
            host.append((t1 - t0) * 1e3)
        row = {"irs": irs, "channels": ch, "samples": n, "log2_fft": lg, "planned_bytes_per_row": per_row, "calls": a.calls,
               "host_cpus": len(os.sched_getaffinity(0)), "host_irs_timed": len(host), "device_minus_host_ir0": diff}
        for name, v in (("call_ms", wall), ("kernel_ms", kernel)):
            row[name] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        row["kernel_gb_per_s"] = per_row * irs * ch / (row["kernel_ms"]["median"] * 1e-3) / 1e9
        row["host_ms_per_ir"] = float(np.median(host))
        row["host_ms_batch_scaled"] = row["host_ms_per_ir"] * irs
        row["call_speedup_over_host"] = row["host_ms_batch_scaled"] / row["call_ms"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
