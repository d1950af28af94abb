"""The inputs of tests/minphase_edge_inputs.py really reach the edges they are named for, on the CPU: the intermediate spectra are
recomputed with numpy as oracle/ir_ingest_oracle.py computes them and the bins at the 1e-300 floor, beyond the +-50 clamp (either
part, either side) and the outputs below the 1e-18 flush are counted; the host path (cpq_ir_convert_to_minimum_phase) and the
oracle must both show the outcome.  tests/test_gpu_ir_minphase_edges.py runs the same inputs on the device, so an edit that makes
an input miss its edge fails here first.

The yardstick's cap: the GPU file allows the device max(8 d_ref, 8 * 2^-52 peak) from the host path, d_ref = max |host - oracle|.
That is only as sharp as the two CPU implementations agree, so d_ref <= 1e-10 * peak(host) is required of every input and size
the GPU file uses that has a non-zero output (measured: 6e-17 ... 3e-15 of the peak)."""
import importlib.util
import os

import numpy as np
import pytest

import convopeq_amd as amd
import minphase_edge_inputs as E

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 1.0e-10


@pytest.fixture(scope="module")
def O():
    spec = importlib.util.spec_from_file_location("ir_ingest_oracle", os.path.join(os.path.dirname(HERE), "oracle", "ir_ingest_oracle.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def check_cap(label, host, d_ref):
    for r in range(host.shape[0]):
        peak = float(np.abs(host[r]).max())
        print(f"{label} row {r}: peak {peak:.3e}  d_ref {d_ref[r]:.3e}  d_ref / peak {d_ref[r] / peak if peak else 0.0:.3e}")
        if peak > 0.0:
            assert d_ref[r] <= CAP * peak
        else:
            assert d_ref[r] == 0.0


@pytest.mark.parametrize("n", E.EDGE_SIZES)
@pytest.mark.parametrize("name", list(E.INPUTS))
def test_the_edge_is_reached(O, name, n):
    x, host, orc, d_ref = E.reference((name, n), E.INPUTS[name](n), amd.ir_convert_to_minimum_phase, O.convert_to_minimum_phase)
    assert np.array_equal(x, E.INPUTS[name](n))                    # deterministic
    assert host.shape == x.shape and orc.shape == x.shape and np.all(np.isfinite(host)) and np.all(np.isfinite(orc))
    cnt = [E.edge_counts(x[r]) for r in range(x.shape[0])]
    print(name, n, cnt)
    c, N = cnt[0], cnt[0]["N"]
    assert N == E.fft_size(n) and N == (4096 if n == 700 else 8192)
    both = (host, orc)
    if name == "huge":
        assert c["re_hi"] == N and c["re_lo"] == 0 and c["floored"] == 0
        assert all(np.abs(y).max() > 1e18 for y in both)
    elif name == "tiny":
        assert c["re_lo"] == N and c["re_hi"] == 0 and c["floored"] == 0 and c["flushed"] == n
        assert c["near"] == n                                       # not zero before the flush: the flush is what zeroes them
        assert all(not y.any() for y in both)
    elif name == "silence":
        assert c["floored"] == N and c["re_lo"] == N and c["flushed"] == n
        assert all(not y.any() for y in both)
    elif name == "half_silent":
        assert x.shape == (2, n) and not x[1].any() and x[0].any()
        assert c["floored"] == 0 and c["re_hi"] == 0 and c["re_lo"] == 0 and c["flushed"] == 0
        assert cnt[1]["floored"] == N and cnt[1]["re_lo"] == N and cnt[1]["flushed"] == n
        assert all(y[0].all() and not y[1].any() for y in both)
    elif name == "flush":
        assert c["floored"] == 0 and c["re_hi"] == 0 and c["re_lo"] == 0
        assert c["flushed"] >= 24 and c["near"] - c["flushed"] >= 24          # dozens on either side of 1e-18
        for y in both:
            assert int((y == 0.0).sum()) >= 24 and int(((y != 0.0) & (np.abs(y) < 4e-18)).sum()) >= 24
            assert not np.any((y != 0.0) & (np.abs(y) < E.FLUSH))
    elif name == "comb":
        assert c["floored"] == 1 and c["re_lo"] == 1 and c["re_hi"] == 0
        assert c["im_hi"] > 0 and c["im_lo"] > 0
        assert all(y.all() for y in both)
    else:
        assert name == "late_impulse"
        assert c["floored"] == 0 and c["re_hi"] == 0 and c["re_lo"] == 0 and c["flushed"] >= 100 and c["kept"] >= 1
        for y in both:
            assert y[0, 0] == 1.0 and int((y == 0.0).sum()) >= 100
            assert not np.any((y != 0.0) & (np.abs(y) < E.FLUSH))
    check_cap(f"{name} n {n}", host, d_ref)


@pytest.mark.parametrize("n", E.BOUNDARY_SIZES)
@pytest.mark.parametrize("name", E.BOUNDARY_INPUTS)
def test_the_cap_at_the_path_boundary(O, name, n):
    x, host, orc, d_ref = E.reference((name, n), E.INPUTS[name](n), amd.ir_convert_to_minimum_phase, O.convert_to_minimum_phase)
    c = E.edge_counts(x[0])
    print(name, n, c)
    assert c["N"] == (4096 if n == 1024 else 8192)
    if name == "comb":
        assert c["floored"] > 0 and c["re_lo"] > 0 and c["im_hi"] > 0 and c["im_lo"] > 0 and host.any()
    elif name == "silence":
        assert c["floored"] == c["N"] and not host.any() and not orc.any()
    else:
        assert c["flushed"] >= 24 and c["near"] - c["flushed"] >= 24
    check_cap(f"{name} n {n}", host, d_ref)


@pytest.mark.parametrize("n", E.LARGE_SIZES)
def test_the_cap_at_the_large_sizes(O, n):
    x, host, orc, d_ref = E.reference(("large", n), E.large_row(n), amd.ir_convert_to_minimum_phase, O.convert_to_minimum_phase)
    assert host.shape == (1, n) and host.any()
    check_cap(f"large n {n}", host, d_ref)


def test_the_rule():
    """the pointwise rule on made-up rows: the flush clause excuses a value below 1e-18 + limit against an exact 0 and nothing
    else, and a row of zeros admits no difference at all"""
    host = np.array([1.0, 0.0, 1.2e-18, 0.0, 5e-19])
    limit = E.limit_of(host, 0.0)
    assert limit == 8 * 2.0 ** -52
    ok = host.copy()
    ok[1] = 0.9e-18                 # the other side kept what the host flushed
    ok[2] = 0.0                     # and flushed what it kept
    assert E.worst_ratio(ok, host, 0.0)[2] <= 1.0
    bad = host.copy()
    bad[0] = 1.0 + 9 * 2.0 ** -52
    assert E.worst_ratio(bad, host, 0.0)[2] > 1.0
    bad = host.copy()
    bad[3] = 1e-18 + 2 * limit      # too large to have been a flush decision
    assert E.worst_ratio(bad, host, 0.0)[2] > 1.0
    bad = host.copy()
    bad[0] = np.nan
    assert not E.worst_ratio(bad, host, 0.0)[2] <= 1.0
    zeros = np.zeros(4)
    assert E.worst_ratio(zeros, zeros, 0.0) == (0.0, 0.0, 0.0)
    assert E.worst_ratio(np.array([0.0, 1e-22, 0.0, 0.0]), zeros, 0.0)[2] <= 1.0      # excused: what an unflushed kernel leaves
    assert E.worst_ratio(np.array([0.0, 2e-18, 0.0, 0.0]), zeros, 0.0)[2] == float("inf")
    # d_ref leaves out the elements on which only the flush decision differs
    a = np.array([1.0, 0.0, 3e-18])
    b = np.array([1.0 + 2.0 ** -52, 0.99e-18 + 1e-18 * 0.02, 3e-18])
    assert E.yardstick(a, b) == 2.0 ** -52
