"""GPU tests of the half-band oversampler kernels at their decision points, against the exact reference of
tests/os_exact.py: guard thresholds (2^53), flush sites (1e-20), the silence test, large magnitudes, tile and lane edges
(kOsTile = 2048 outputs per workgroup, 8 per lane), ragged calls against one call bit for bit, the bench shape through
the device entry points, and engine state.  The inputs come from tests/os_edge_inputs.py; test_os_exact_cpu.py checks on
the CPU that every decision in them is determined.  Each test prints its worst error as a fraction of the bound E."""
import numpy as np
import pytest

import os_edge_inputs as I
import os_exact as X
import os_model as M

pytestmark = pytest.mark.gpu

SCEN = {s[0]: s for s in I.all_scenarios()}


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def engine(amd, S, F, os_type, max_base):
    eng = amd.BatchedEngine(S, block_size=480, max_ir_len=1024, max_blocks_per_call=(max_base * F + 479) // 480,
                            call_mode=amd.CPQ_CALLS_ANY, sample_rate=48000.0 * F)
    eng.set_oversampling(F, os_type)
    return eng


def run_op(eng, kind, x):
    return eng.os_up(x) if kind == "up" else eng.os_down(x)


@pytest.mark.parametrize("name", list(SCEN))
def test_scenario_matches_exact_reference(amd, name):
    """Every output within E of the exact sum (bit-equal where E = 0: the impulse cases), and the event counters,
    auto-clears, corruption_pending, hard fallback and consecutive auto-clears equal to the model's after every call."""
    _, F, T, ops = SCEN[name]
    nmax = max(x.shape[1] // (F if kind == "down" else 1) for kind, x in ops)
    eng = engine(amd, 1, F, T, nmax)
    ref, mod = X.ExactOversampler(F, T), M.Oversampler(F, T)
    worst = max_e = 0.0
    for k, (kind, x) in enumerate(ops):
        y = run_op(eng, kind, x)
        r = getattr(ref, kind)(x)
        getattr(mod, kind)(x)
        assert ref.undetermined == 0, (k, ref.undetermined)
        ratio = X.error_ratio(y, r)
        worst = max(worst, ratio)
        max_e = max(max_e, float(np.max(r.E)))
        assert ratio <= 1.0, (k, kind, ratio)
        tel = X.gpu_telemetry(eng.os_telemetry(0))
        assert tel == X.model_telemetry(mod) == ref.telemetry(), (k, kind, tel, X.model_telemetry(mod))
    print(f"[{name}] worst |err| / E = {worst:.3g} over {len(ops)} calls, largest E = {max_e:.3g}")
    eng.close()


@pytest.mark.parametrize("F,os_type", I.PAIRS)
def test_ragged_calls_equal_one_call_bit_for_bit(amd, F, os_type):
    """More than `keep` consecutive 1..7-sample calls (every history rebuilt only from call inputs) equal one call of the
    same samples exactly.  Condition: no call takes the silence path (checked on the model) and no sample lies in
    (0, 1e-19)."""
    rng = np.random.default_rng(100 + 10 * F + os_type)
    stages = [M.design_stage(i, os_type) for i in range(I.up_stage(F) + 1)]
    keep = max(max(s["history_up_keep"], s["history_down_keep"]) for s in stages)
    lens = rng.integers(1, 8, keep + 8)
    n = int(lens.sum())
    x = rng.uniform(-1.0, 1.0, (2, n))
    y = rng.uniform(-1.0, 1.0, (2, n * F))
    assert np.all(np.abs(x) >= 1e-19) and np.all(np.abs(y) >= 1e-19)
    split, whole = engine(amd, 1, F, os_type, 7), engine(amd, 1, F, os_type, n)
    mod = M.Oversampler(F, os_type)
    ups, downs, o = [], [], 0
    for m in lens:
        ups.append(split.os_up(x[:, o:o + m]))
        downs.append(split.os_down(y[:, o * F:(o + m) * F]))
        mod.down(y[:, o * F:(o + m) * F])
        o += m
    assert mod.silent_paths == 0 and mod.events == 0
    u1, d1 = whole.os_up(x), whole.os_down(y)
    assert np.array_equal(np.concatenate(ups, axis=1), u1)
    assert np.array_equal(np.concatenate(downs, axis=1), d1)
    print(f"[ragged F={F} T={os_type}] {len(lens)} calls ({n} base samples) bit-equal to one call")
    split.close()
    whole.close()


BENCH_GROUPS = 6
NAN_STREAMS = (253, 254, 255)


def _bench_inputs(S, nb, calls, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(nb * calls)
    base = np.empty((BENCH_GROUPS, 2, nb * calls))
    for g in range(BENCH_GROUPS):
        for ch in range(2):
            if g % 3 == 0:
                v = rng.uniform(-1.0, 1.0, nb * calls)
            elif g % 3 == 1:
                v = 0.4 * np.sin(2 * np.pi * 0.0031 * (g + 1 + ch) * t) + 0.3 * np.sin(2 * np.pi * 0.27 * t + g)
            else:
                v = rng.uniform(-0.5, 0.5, nb * calls) * (np.sin(2 * np.pi * t / (1900.0 + 97 * g)) > 0)
            base[g, ch] = v * (1.0 + 0.25 * g)
    group = np.arange(S) % BENCH_GROUPS
    sign = np.where((np.arange(S) // BENCH_GROUPS) % 2 == 0, 1.0, -1.0)
    x = (base[group] * sign[:, None, None]).reshape(2 * S, nb * calls)
    dirty = x.copy()
    for j, s in enumerate(NAN_STREAMS):                  # NaN bursts in call j % calls, at different offsets
        o = (j % calls) * nb + 1000 + 7919 * j
        dirty[2 * s + j % 2, o:o + 64] = np.nan
    if calls > 1:
        dirty[2 * NAN_STREAMS[2], nb + 50:nb + 60] = np.nan
    return x, dirty, group, sign


@pytest.mark.parametrize("F,os_type", I.PAIRS)
def test_bench_shape_device_entry_points(amd, F, os_type):
    """256 streams x 65536 base samples through os_up_device / os_down_device (torch tensors), two calls: one
    representative per group of streams against os_model within 2 E (E = gamma_C sum |c| |x|, chained through the
    stages), every other stream bit-equal or exactly negated on the device, the NaN-burst streams' telemetry equal to
    the model's and every other stream bit-equal to a run without them."""
    import torch
    S, nb, calls = 256, 65536, 2
    x, dirty, group, sign = _bench_inputs(S, nb, calls, seed=F * 7 + os_type)
    dev = torch.device("cuda")

    def run(inp):
        eng = amd.BatchedEngine(S, block_size=4096, max_ir_len=4096, max_blocks_per_call=nb * F // 4096,
                                sample_rate=48000.0 * F)
        eng.set_oversampling(F, os_type)
        ups, downs, tels = [], [], []
        for k in range(calls):
            xi = torch.from_numpy(np.ascontiguousarray(inp[:, k * nb:(k + 1) * nb])).to(dev)
            u = torch.empty((2 * S, nb * F), dtype=torch.float64, device=dev)
            d = torch.empty((2 * S, nb), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            eng.os_up_device(xi.data_ptr(), u.data_ptr(), nb)
            eng.os_down_device(u.data_ptr(), d.data_ptr(), nb)
            eng.synchronize()
            ups.append(u)
            downs.append(d)
            tels.append([X.gpu_telemetry(eng.os_telemetry(s)) for s in NAN_STREAMS])
        eng.close()
        return ups, downs, tels

    ups, downs, tels = run(dirty)
    cups, cdowns, _ = run(x)
    keep = torch.ones(S, dtype=torch.bool)
    keep[list(NAN_STREAMS)] = False
    kc = keep.repeat_interleave(2).to(dev)
    rep = torch.as_tensor(group).to(dev)
    sg = torch.as_tensor(sign).to(dev)
    worst = 0.0
    for k in range(calls):
        for a, b in ((ups[k], cups[k]), (downs[k], cdowns[k])):
            assert torch.equal(a[kc], b[kc])                 # NaN streams leave every other stream untouched
            v = b.view(S, 2, -1)
            assert torch.equal(v, sg[:, None, None] * v[rep])   # groups: identical or exactly negated
    # os_exact in cheap mode computes os_model's own np.convolve values (test_os_exact_cpu checks they are equal) and
    # carries the 2 E allowance through the stages
    refs = [X.ExactOversampler(F, os_type, cheap=True) for _ in range(BENCH_GROUPS)]
    mods = [M.Oversampler(F, os_type) for _ in NAN_STREAMS]
    for k in range(calls):
        hu = cups[k][:2 * BENCH_GROUPS].cpu().numpy()
        hd = cdowns[k][:2 * BENCH_GROUPS].cpu().numpy()
        for g in range(BENCH_GROUPS):
            ru = refs[g].up(x[2 * g:2 * g + 2, k * nb:(k + 1) * nb])
            rd = refs[g].down(hu[2 * g:2 * g + 2])
            assert refs[g].undetermined == 0
            for got, r in ((hu[2 * g:2 * g + 2], ru), (hd[2 * g:2 * g + 2], rd)):
                ratio = X.error_ratio(got, r)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (k, g, ratio)
        for j, s in enumerate(NAN_STREAMS):
            mods[j].down(mods[j].up(dirty[2 * s:2 * s + 2, k * nb:(k + 1) * nb]))
            assert tels[k][j] == X.model_telemetry(mods[j]), (k, s, tels[k][j], X.model_telemetry(mods[j]))
    assert all(m.events > 0 for m in mods)
    print(f"[bench shape F={F} T={os_type}] worst |kernel - model| / E = {2 * worst:.3g} (allowed 2)")


def test_corruption_pending_set_by_up_and_cleared_by_down(amd):
    F, T, n = 4, M.IIR, 600
    rng = np.random.default_rng(5)
    eng = engine(amd, 2, F, T, n)
    x = rng.uniform(-1.0, 1.0, (4, n))
    x[2, 300] = 1e300                                   # stream 1: a bad centre
    eng.os_up(x)
    t0, t1 = eng.os_telemetry(0), eng.os_telemetry(1)
    assert t0["corruption_pending"] == 0 and t1["corruption_pending"] == 1 and t1["corruption_events"] >= 1
    y = eng.os_down(rng.uniform(-1.0, 1.0, (4, n * F)))
    t1 = eng.os_telemetry(1)
    assert t1["corruption_pending"] == 0 and t1["auto_clears"] == 1 and np.all(y[2:4] == 0.0)
    eng.os_up(rng.uniform(-1.0, 1.0, (4, n)))
    assert eng.os_telemetry(1)["corruption_pending"] == 0
    eng.close()


def test_switching_factor_and_type_on_a_live_engine(amd):
    """set_oversampling 8 -> 2 -> 4 (IIR) -> 4 (LinearPhase) with dirty histories and flags: the next calls are
    bit-equal to a fresh engine's."""
    rng = np.random.default_rng(17)
    n = 1000
    live = engine(amd, 2, 8, M.IIR, n)
    x = rng.uniform(-1.0, 1.0, (4, n))
    x[0, 10] = np.nan
    live.os_down(live.os_up(x))
    live.os_up(x)                                        # leaves corruption_pending set
    for F, T in ((2, M.IIR), (4, M.IIR), (4, M.LINEAR_PHASE)):
        live.set_oversampling(F, T)
        fresh = engine(amd, 2, F, T, n)
        for k in range(3):
            xi = rng.uniform(-1.0, 1.0, (4, n))
            yi = rng.uniform(-1.0, 1.0, (4, n * F))
            assert np.array_equal(live.os_up(xi), fresh.os_up(xi)), (F, T, k)
            assert np.array_equal(live.os_down(yi), fresh.os_down(yi)), (F, T, k)
            for s in range(2):
                assert live.os_telemetry(s) == fresh.os_telemetry(s)
        fresh.close()
        x = rng.uniform(-1.0, 1.0, (4, n))
        x[1, 5] = np.inf
        live.os_up(x)                                    # dirty again before the next switch
    live.close()
