"""The output stage at the bench shape (256 streams x 524288 samples, block 512, FFT partition 4096, conv + EQ, device entry
point): the step with the stage off and on, and the stage's kernels alone on the rows the chain delivers, timed by cpq_profile_*.

    python tools/out_stage_bench.py          # writes profiles/out_stage_bench.json

k_out_pre moves 16 B per sample and channel (4.29 GB at this shape); k_out_post is run on the bench rows, which never limit,
and on the same rows scaled and offset so that every sample lies above the threshold (the sequential worst case)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np, torch
import convopeq_amd as amd
import oracle_lib as O

S, B, T, L = 256, 512, 1024, 131072
n = B * T
eng = amd.BatchedEngine(S, block_size=B, max_ir_len=L, max_blocks_per_call=T, partition_size=4096)
ir_l, ir_r = O.gen_ir(L, stream=0, channel=0), O.gen_ir(L, stream=0, channel=1)
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
res = {}

def step_times(steps=5, warm=2):
    for _ in range(warm):
        eng.process_device(d_in.data_ptr(), d_out.data_ptr(), n)
    eng.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        eng.process_device(d_in.data_ptr(), d_out.data_ptr(), n)
        eng.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts

def prof_stage(rows, flags, reps=3):
    """the stage alone on device rows (in place on a copy), per launch group"""
    eng.set_output_stage(flags)
    buf = rows.clone()
    torch.cuda.synchronize()
    eng.out_process_device(buf.data_ptr(), buf.data_ptr(), n)   # warm
    eng.synchronize()
    out = []
    for _ in range(reps):
        buf.copy_(rows)
        eng.out_reset()
        torch.cuda.synchronize()
        eng.profile_enable(True); eng.profile_reset()
        eng.out_process_device(buf.data_ptr(), buf.data_ptr(), n)
        out.append(eng.profile_read()["k_out"][1])
        eng.profile_enable(False)
    return out, [eng.out_read_envelope(s) for s in (0, S - 1)]

for name, flags in (("off", 0), ("all", amd.CPQ_OUT_ALL)):
    eng.set_output_stage(flags)
    res["step_ms_" + name] = step_times()
    eng.profile_enable(True); eng.profile_reset()
    eng.process_device(d_in.data_ptr(), d_out.data_ptr(), n)
    res["kernels_ms_" + name] = {k: v for k, v in eng.profile_read().items() if v[0]}
    eng.profile_enable(False)
eng.set_output_stage(0)
eng.process_device(d_in.data_ptr(), d_out.data_ptr(), n)
eng.synchronize()
rows = d_out.clone()
res["rows_peak"] = float(rows.abs().max())
res["k_out_pre_ms(dc+headroom)"], _ = prof_stage(rows, amd.CPQ_OUT_DC_BLOCK | amd.CPQ_OUT_HEADROOM)
res["k_out_headroom_ms"], _ = prof_stage(rows, amd.CPQ_OUT_HEADROOM)
res["k_out_post_ms(never limits)"], res["env_quiet"] = prof_stage(rows, amd.CPQ_OUT_LIMITER | amd.CPQ_OUT_CLAMP)
res["k_out_post_ms(clamp only)"], _ = prof_stage(rows, amd.CPQ_OUT_CLAMP)
loud = rows * (4.0 / res["rows_peak"]) + 1.0        # every sample above the threshold: limits continuously
res["k_out_post_ms(limits continuously)"], res["env_loud"] = prof_stage(loud, amd.CPQ_OUT_LIMITER | amd.CPQ_OUT_CLAMP, reps=2)
eng.set_output_stage(0)
eng.profile_enable(True); eng.profile_reset()
eng.process_device(d_in.data_ptr(), d_out.data_ptr(), n)
pr = eng.profile_read()
res["fdl_mac_ms"] = pr["k_fdl_mac"]
res["bytes_pre"] = 16 * 2 * S * n
eng.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
json.dump(res, open(os.path.join(ROOT, "profiles", "out_stage_bench.json"), "w"), indent=1)
print(json.dumps(res))
