"""CPU tests (no GPU) of the oversampler edge inputs: tests/os_exact.py against exact rational arithmetic, then
os_model.Oversampler against os_exact on every input of test_gpu_oversampling_edges.py -- within E of the exact sum,
with identical telemetry and silence paths, every guard / flush / silence decision determined, and each scenario
constructing the edge it is named for."""
from fractions import Fraction

import numpy as np
import pytest

import os_edge_inputs as I
import os_exact as X
import os_model as M

LIMIT = 2.0 ** 53
D = M.DENORM


def test_two_prod_and_sums_are_exact():
    rng = np.random.default_rng(3)
    a = rng.uniform(-1, 1, 4000) * 2.0 ** rng.uniform(-70, 54, 4000)
    b = rng.uniform(-1, 1, 4000)
    p, e = X.two_prod(a, b)
    for i in range(0, 4000, 7):
        assert Fraction(p[i]) + Fraction(e[i]) == Fraction(a[i]) * Fraction(b[i])
    c = M.design_stage(2, M.LINEAR_PHASE)["conv"]
    C = len(c)
    x = rng.uniform(-1, 1, 50 + C - 1) * 2.0 ** rng.uniform(-66, 53, 50 + C - 1)
    cen = rng.uniform(-1, 1, 50) * 2.0 ** 40
    v, nf = X._window_sums(x, np.zeros_like(x), c, C - 1, 50, cen, np.zeros(50))
    assert not nf.any()
    for i in range(50):
        W = x[i:i + C][::-1]
        S = Fraction(cen[i]) + sum(Fraction(float(cr)) * Fraction(float(w)) for cr, w in zip(c, W))
        assert Fraction(v.hi[i]) == Fraction(float(S)) and abs(S - Fraction(v.hi[i]) - Fraction(v.lo[i])) <= \
            abs(Fraction(v.lo[i])) * Fraction(2.0 ** -52)
        naive = float(cen[i] + W @ c)
        assert abs(Fraction(naive) - S) <= Fraction(v.E[i])


def _run(F, T, ops):
    """(ref, model, per-op records) with every check of B applied after each op"""
    ref, mod = X.ExactOversampler(F, T), M.Oversampler(F, T)
    recs = []
    for k, (kind, x) in enumerate(ops):
        r = getattr(ref, kind)(x)
        y = getattr(mod, kind)(x)
        ratio = X.error_ratio(y, r)
        assert ref.undetermined == 0, (k, kind, ref.undetermined)
        assert ratio <= 1.0, (k, kind, ratio)
        assert X.model_telemetry(mod) == ref.telemetry(), (k, kind)
        assert mod.silent_paths == ref.silent_paths, (k, kind)
        recs.append((kind, r, list(ref.trace), set(ref.last_silent), ref.telemetry()))
    return ref, mod, recs


SCEN = {s[0]: s for s in I.all_scenarios()}


def has(v, value, ch):
    return bool(np.any(v.hi[ch] == value))


@pytest.mark.parametrize("name", list(SCEN))
def test_model_within_exact_bound_and_decisions_determined(name):
    _, F, T, ops = SCEN[name]
    ref, _, recs = _run(F, T, ops)
    assert ref.decisions > 0
    top = I.up_stage(F)
    nst = top + 1
    if name.startswith(("up_", "down_")):
        for kind, r, *_ in recs:            # impulses: every output is one rounded product -> bit-equal required
            assert np.all(r.E == 0.0) and np.all(r.lo == 0.0), kind
    ev = [rec[4][0] for rec in recs]
    if name.startswith("up_centre"):
        assert has(recs[0][1], LIMIT, 0) and has(recs[0][1], -LIMIT, 1) and ev[0] == 0
        assert recs[2][4][2] == 1 and ev[2] == 2 and recs[3][4][1] == 1 and recs[3][4][2] == 0
    elif name.startswith("up_flush"):
        assert has(recs[0][1], 2 * D, 0) and not has(recs[0][1], -2 * np.nextafter(D, 0), 1)
        assert has(recs[1][1], D, 0) and not has(recs[1][1], -np.nextafter(D, 0), 1)
    elif name.startswith("up_conv"):
        assert has(recs[0][1], 2 * LIMIT, 0) and not has(recs[0][1], -2 * np.nextafter(LIMIT, np.inf), 1)
        assert ev[0] == 2                   # the bad centres; the zeroed convolution sum is not an event
    elif name.startswith("down_centre"):
        assert has(recs[0][1], LIMIT, 0) and has(recs[0][1], -LIMIT, 1) and ev[0] == 0 and ev[1] == 2
        assert recs[2][4][1] == 1 and np.all(recs[2][1].hi == 0)
    elif name.startswith("down_sum"):
        assert has(recs[0][1], LIMIT - 1, 0) and has(recs[0][1], -(LIMIT - 1), 1) and ev[0] == 0
        assert has(recs[2][1], LIMIT, 0) and has(recs[2][1], -LIMIT, 1) and ev[2] == 0
        assert ev[4] == 2
    elif name.startswith("down_product"):
        assert has(recs[0][1], -LIMIT, 1) and ev[0] >= 1
    elif name.startswith("down_flush"):
        assert has(recs[0][1], D, 0) and not has(recs[0][1], -np.nextafter(D, 0), 1)
        assert has(recs[1][1], D, 0) and not has(recs[1][1], -np.nextafter(D, 0), 1)
    elif name.startswith("block_max_eq"):
        assert recs[0][3] == {(i, ch) for i in range(nst) for ch in (0, 1)} and not recs[1][3]
    elif name.startswith("block_max_above"):
        assert (top, 1) in recs[0][3] and (top, 0) not in recs[0][3]
    elif name.startswith("history_max_eq"):
        assert (top, 0) not in recs[0][3] and (top, 0) in recs[1][3] and (top, 1) in recs[1][3]
    elif name.startswith("history_max_above"):
        assert (top, 0) not in recs[1][3] and (top, 1) in recs[1][3]
    elif name.startswith("nan_block"):
        assert len(recs[0][3]) == 2 * nst and ev[0] == 0 and ev[1] == 0 and np.all(recs[0][1].hi == 0)
    elif name.startswith("stage_below_silent"):
        outs = {(i, ch): v for d, i, ch, v in recs[0][2]}
        assert outs[(top, 0)].hi.max() == D and outs[(top, 1)].hi.max() == np.nextafter(D, np.inf)
        assert (top - 1, 0) in recs[0][3] and (top - 1, 1) not in recs[0][3] and (top, 0) not in recs[0][3]
    elif name.startswith("large"):
        s0 = [v for kind, r, tr, *_ in recs if kind == "up" for d, i, ch, v in tr if i == 0]
        assert any(np.any((np.abs(v.hi[0::2]) > LIMIT) & (np.abs(v.hi[0::2]) <= 2 * LIMIT)) for v in s0)
        assert max(rec[4][0] for rec in recs) > 0 and recs[-1][4][1] > 0   # events and auto-clears happen


@pytest.mark.parametrize("name", ["tiles_F8_T1", "large_F4_T0", "nan_block_F8_T0"])
def test_cheap_reference_is_the_model(name):
    """cheap mode (the bench-shape test) holds os_model's own values, with a bound of 2 E"""
    _, F, T, ops = SCEN[name]
    ref, mod = X.ExactOversampler(F, T, cheap=True), M.Oversampler(F, T)
    for kind, x in ops:
        r = getattr(ref, kind)(x)
        assert np.array_equal(r.hi, getattr(mod, kind)(x)) and np.all(r.lo == 0.0)
        assert ref.telemetry() == X.model_telemetry(mod) and ref.undetermined == 0
