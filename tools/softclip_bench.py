"""The soft clipper at the bench shape (256 streams x 524288 samples, block 512): k_soft_clip alone on device rows, beside
k_out_headroom on the same rows (both read and write every sample once: 16 B per sample and channel), and inside the whole-chain
call at factor 1 (with its local 2x pair, whose k_os_halfband time is the pair's alone there) and at factor 2.  Timed by
cpq_profile_* (HIP events around the launches), every repetition listed.

    python tools/softclip_bench.py          # writes profiles/softclip_bench.json

The chain around the stage is kept out of the way: convolver bypassed, the EQ's default parameters.  Rows: noise at +-2 (most
samples clip, on both streams' curves) and noise at +-0.05 (every sample below the clip start: the kernel only moves them)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import convopeq_amd as amd

S, B, T = 256, 512, 1024
n = B * T
res = {"streams": S, "n": n}


def make_engine(factor, block):
    # sized for 2 n samples per call: the clipper's rows at factor 1 (the local pair's block) and at factor 2
    eng = amd.BatchedEngine(S, block_size=block, max_ir_len=1024, max_blocks_per_call=2 * n // block, sample_rate=48000.0 * factor)
    eng.set_conv_bypass(True)
    eng.set_eq_params(amd.CPQ_ALL_STREAMS, amd.eq_params_default())
    if factor > 1:
        eng.set_oversampling(factor)
    for s in range(S):
        eng.set_soft_clip(s, True, 0.2 if s % 2 == 0 else 1.0)
    return eng


def profiled(eng, key, fn, reps=3):
    fn()
    eng.synchronize()
    out = []
    for _ in range(reps):
        eng.profile_enable(True); eng.profile_reset()
        fn()
        out.append({k: v for k, v in eng.profile_read().items() if v[0] and k in key})
        eng.profile_enable(False)
    return out


g = torch.Generator(device="cuda").manual_seed(1)
loud = 4.0 * torch.rand((2 * S, 2 * n), dtype=torch.float64, device="cuda", generator=g) - 2.0
quiet = loud * 0.025
buf = torch.empty_like(loud)
torch.cuda.synchronize()

eng = make_engine(1, B)
for name, rows in (("loud", loud), ("quiet", quiet)):
    for m, cb in ((n, B), (2 * n, 2 * B), (2 * n, 2 * B + 2)):          # the last: callbacks with a two-sample scalar tail
        view = rows[:, :m].contiguous()
        tgt = buf[:, :m].contiguous()
        tgt.copy_(view)
        torch.cuda.synchronize()
        r = profiled(eng, ("k_soft_clip",), lambda: eng.soft_clip_process_device(tgt.data_ptr(), tgt.data_ptr(), m, cb))
        ms = [x["k_soft_clip"][1] for x in r]
        res[f"k_soft_clip_ms({name}, {m} samples, callback {cb})"] = ms
        res[f"k_soft_clip_TBps({name}, {m} samples, callback {cb})"] = [16.0 * 2 * S * m / (t * 1e-3) / 1e12 for t in ms]
# the yardstick on the same rows: k_out_headroom, also one read and one write of every sample
eng.set_output_stage(amd.CPQ_OUT_HEADROOM)
view = loud[:, :n].contiguous()
r = profiled(eng, ("k_out",), lambda: eng.out_process_device(view.data_ptr(), buf.data_ptr(), n))
ms = [x["k_out"][1] for x in r]
res["k_out_headroom_ms"] = ms
res["k_out_headroom_TBps"] = [16.0 * 2 * S * n / (t * 1e-3) / 1e12 for t in ms]
eng.set_output_stage(0)
# whole chain at factor 1: the local 2x pair (k_os_halfband: up and down of the 31-tap stage) and the clipper on 2 n samples
d_in, d_out = view, buf[:, :n].contiguous()
res["chain_factor1"] = profiled(eng, ("k_soft_clip", "k_os_halfband"), lambda: eng.process_device(d_in.data_ptr(), d_out.data_ptr(), n))
eng.close()
# whole chain at factor 2: the clipper in place on the oversampled block of 2 n samples
eng = make_engine(2, 2 * B)
res["chain_factor2"] = profiled(eng, ("k_soft_clip", "k_os_halfband"), lambda: eng.process_device(d_in.data_ptr(), d_out.data_ptr(), n))
eng.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
json.dump(res, open(os.path.join(ROOT, "profiles", "softclip_bench.json"), "w"), indent=1)
print(json.dumps(res, indent=1))
