"""Times the host-pointer whole-chain call at the bench shape (256 streams x 524288 samples, block 512, FFT partition 4096,
conv + EQ) with fp64 rows and with packed PCM on the bus, pinned and pageable, in one process on one build:

    F64/F64   cpq_engine_process_block                          32 B per stereo sample over the bus
    F32/F32   cpq_engine_process_block_pcm, planar              16 B
    S24/F32   cpq_engine_process_block_pcm, interleaved         14 B

    python tools/pcm_io_bench.py [--streams 256] [--steps 3] [--warmup 1] [--out profiles/pcm_io_bench.json]

The yardstick of the packed modes is the F64/F64 line of the same run.  A second pass with the profiler on gives the time of
the converters per call (CPQ_K_PCM) and the bytes they move: unpack reads bps_in and writes 8 B per sample, pack reads 8 B and
writes bps_out."""
import argparse
import ctypes as C
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ir-len", type=int, default=131072)
    ap.add_argument("--blocks-per-call", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm_io_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import convopeq_amd as amd
    from convopeq_amd import _capi as K
    import oracle_lib as O

    S, B, T = a.streams, 512, a.blocks_per_call
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

    rng = np.random.default_rng(1)
    bps = {f: K.load().cpq_pcm_bytes_per_sample(f) for f in range(5)}
    modes = (("F64/F64", K.CPQ_PCM_F64, K.CPQ_PCM_F64, K.CPQ_PCM_PLANAR), ("F32/F32", K.CPQ_PCM_F32, K.CPQ_PCM_F32, K.CPQ_PCM_PLANAR),
             ("S24/F32 interleaved", K.CPQ_PCM_S24, K.CPQ_PCM_F32, K.CPQ_PCM_INTERLEAVED))

    def buffers(fi, fo):
        """(in, out) as uint8; the input holds noise at about -26 dB in the format's own coding"""
        count = 2 * S * n
        if fi == K.CPQ_PCM_F64:
            src = (0.05 * rng.standard_normal(count)).view(np.uint8)
        elif fi == K.CPQ_PCM_F32:
            src = (0.05 * rng.standard_normal(count, dtype=np.float32)).view(np.uint8)
        else:
            src = rng.integers(0, 256, count * 3, dtype=np.uint8)
            src[2::3] = (rng.integers(-6, 6, count, dtype=np.int8)).view(np.uint8)         # top byte: small signed values
        return src, np.empty(count * bps[fo], dtype=np.uint8)

    def call(fi, fo, layout, src, dst):
        if fi == K.CPQ_PCM_F64 and fo == K.CPQ_PCM_F64:
            dp = C.POINTER(C.c_double)
            return eng._lib.cpq_engine_process_block(eng._h, C.cast(src.ctypes.data, dp), C.cast(dst.ctypes.data, dp), n)
        return eng._lib.cpq_engine_process_block_pcm(eng._h, C.c_void_p(src.ctypes.data), fi, C.c_void_p(dst.ctypes.data), fo, layout, 0, n)

    result = {"streams": S, "samples_per_call": n, "block_size": B, "steps": a.steps, "warmup": a.warmup, "modes": []}
    for pinned in (True, False):
        for name, fi, fo, layout in modes:
            src, dst = buffers(fi, fo)
            if pinned:
                for buf in (src, dst):
                    assert eng._lib.cpq_host_register(C.c_void_p(buf.ctypes.data), buf.nbytes) == 0
            eng.profile_enable(False)
            for _ in range(a.warmup):
                eng._ck(call(fi, fo, layout, src, dst))
            times = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                eng._ck(call(fi, fo, layout, src, dst))           # the host-pointer call returns after its download
                times.append(time.perf_counter() - t0)
            eng.profile_enable(True)
            eng.profile_reset()
            eng._ck(call(fi, fo, layout, src, dst))
            prof = eng.profile_read()
            eng.profile_enable(False)
            if pinned:
                for buf in (src, dst):
                    assert eng._lib.cpq_host_unregister(C.c_void_p(buf.ctypes.data)) == 0
            best = min(times)
            row = {"mode": name, "pinned": pinned, "seconds_best": best, "seconds_all": times,
                   "stereo_samples_per_s": S * n / best, "bus_bytes_per_stereo_sample": 2 * (bps[fi] + bps[fo]),
                   "profile_ms": {k: v[1] for k, v in prof.items()}, "profile_launches": {k: v[0] for k, v in prof.items()}}
            if "k_pcm" in prof:
                moved = 2 * S * n * (bps[fi] + 8 + 8 + bps[fo])
                row["k_pcm_bytes_moved"] = moved
                row["k_pcm_bytes_per_s"] = moved / (prof["k_pcm"][1] * 1e-3)
            result["modes"].append(row)
            print(json.dumps(row), flush=True)
            del src, dst
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
