"""cpq_src (CPQ_SRC_HOST, no GPU): the streaming sample-rate converter against the one-shot definition.

The concatenated output of a stream is, bit for bit, cpq::resampleRowHost of the concatenated input -- reached here through
amd.ir_resample(..., host=True) -- for every split into calls.  Rows are undamped uniform noise, so the IR path's tail trim
takes at most the last 8 samples; those are held to the np.longdouble model.  "Same" is equal shape and equal uint64 views."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import convopeq_amd as amd
import resample_model as M
from convopeq_amd import _capi as K

HERE = os.path.dirname(os.path.abspath(__file__))
RATIOS = [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000), (88200, 48000), (96000, 44100), (8000, 96000), (96000, 8000)]


def noise(shape, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, size=shape)


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def cuts(sizes, n):
    """call lengths: the sizes given, then the rest of n"""
    assert sum(sizes) <= n
    return list(sizes) + [n - sum(sizes)]


def ragged(n, seed, most=400):
    rng, sizes = np.random.default_rng(seed), []
    while sum(sizes) < n:
        sizes.append(int(min(rng.integers(0, most + 1), n - sum(sizes))))
    return sizes


def stream(src, x, sizes, flush_alone=False):
    """x through src in calls of `sizes`, the last one (or a call of no samples behind them) with flush.  Returns the concatenated
    output; every call's n_out is checked against cpq_src_out_count."""
    out, at = [], 0
    calls = [(s, i == len(sizes) - 1 and not flush_alone) for i, s in enumerate(sizes)] + ([(0, True)] if flush_alone else [])
    for size, flush in calls:
        expect = src.out_count(size, flush)
        y = src.process(x[:, at:at + size], flush=flush)
        assert y.shape == (x.shape[0], expect)
        out.append(y)
        at += size
    assert at == x.shape[1]
    return np.concatenate(out, axis=1), [o.shape[1] for o in out]


def splits(T, n):
    return {"whole": [n], "forty singles": cuts([1] * 40, n), "around the latency": cuts([T // 2 - 1, 1, 1, T], n),
            "ragged": ragged(n, 5)}


@pytest.fixture(scope="module")
def case():
    """2 channels x 2 T + 37 samples at 44100 -> 48000: the rows, the one-shot rows, the design, the whole-stream output"""
    a, b = 44100, 48000
    d = amd.resample_design(a, b)
    assert d["T"] == 600
    x = noise((2, 2 * d["T"] + 37), 1)
    x.setflags(write=False)
    one = amd.ir_resample(x, a, b, host=True)
    whole, _ = stream(amd.StreamResampler(2, a, b, 4096, host=True), x, [x.shape[1]])
    whole.setflags(write=False)
    return {"a": a, "b": b, "d": d, "x": x, "one": one, "whole": whole}


def test_bits_against_the_one_shot_definition(case):
    d, x, one, whole = case["d"], case["x"], case["one"], case["whole"]
    n_out = M.out_len(x.shape[1], case["a"], case["b"])
    assert whole.shape == (2, n_out)
    assert n_out - 8 <= one.shape[1] <= n_out               # undamped: the IR path trims at most the last 8 samples
    assert same(np.ascontiguousarray(whole[:, :one.shape[1]]), one)
    # what the trim took is held to the longdouble model, with the bound of test_ratios
    idx = np.arange(one.shape[1] - 1, n_out)
    u = 2.0 ** -53
    for ch in range(2):
        model, bound = M.resample_rows(d, x[ch], outputs=idx)
        limit = (d["T"] * u / (1 - d["T"] * u) + d["T"] * 2.0 ** -63) * bound
        assert np.all(np.abs(whole[ch, idx].astype(np.longdouble) - model) <= limit)


def test_call_splits_and_out_count(case):
    a, b, x, T = case["a"], case["b"], case["x"], case["d"]["T"]
    n = x.shape[1]
    for name, sizes in splits(T, n).items():
        src = amd.StreamResampler(2, a, b, 4096, host=True)
        assert src.latency == T // 2
        got, counts = stream(src, x, sizes)
        assert same(got, case["whole"]), name
        assert sum(counts) == M.out_len(n, a, b)
        if name == "around the latency":
            assert counts[:2] == [0, 0] and counts[2] > 0        # nothing before sample T / 2 has arrived
    got, counts = stream(amd.StreamResampler(2, a, b, 4096, host=True), x, ragged(n, 6), flush_alone=True)
    assert same(got, case["whole"]) and counts[-1] > 0


def test_stream_lifecycle(case):
    a, b, x, d = case["a"], case["b"], case["x"], case["d"]
    n = x.shape[1]
    for p in (1, 2 ** 40 // d["L"]):
        got, _ = stream(amd.StreamResampler(2, a, b, 4096, host=True, start_period=p), x, ragged(n, 7))
        assert same(got, case["whole"]), p
    src = amd.StreamResampler(2, a, b, 4096, host=True)
    src.process(noise((2, 777), 8))
    src.reset()
    got, _ = stream(src, x, ragged(n, 9))
    assert same(got, case["whole"])
    # two streams separated by a flush: each as from a fresh object
    x2 = noise((2, 901), 10)
    want2, _ = stream(amd.StreamResampler(2, a, b, 4096, host=True), x2, [901])
    got2, _ = stream(src, x2, ragged(901, 11))
    got3, _ = stream(src, x, [n])
    assert same(got2, want2) and same(got3, case["whole"])


@pytest.mark.parametrize("pair", RATIOS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_ratios(pair):
    a, b = pair
    d = amd.resample_design(a, b)
    x = noise((2, 2 * d["T"] + 37), a % 1000 + b % 999)
    one = amd.ir_resample(x, a, b, host=True)
    src = amd.StreamResampler(2, a, b, 700, host=True)
    assert src.latency == d["T"] // 2
    got, _ = stream(src, x, ragged(x.shape[1], a % 97, most=700))
    n_out = M.out_len(x.shape[1], a, b)
    assert got.shape == (2, n_out) and n_out - 8 <= one.shape[1]
    assert same(np.ascontiguousarray(got[:, :one.shape[1]]), one)


def test_stream_shorter_than_its_filter():
    a, b = 768000, 8000
    x = noise((2, 2500), 3)
    src = amd.StreamResampler(2, a, b, 1000, host=True)
    assert src.latency == amd.resample_design(a, b)["T"] // 2 > 2500
    got, counts = stream(src, x, [1000, 1000, 500])
    assert counts == [0, 0, M.out_len(2500, a, b)]           # all of it at the flush
    one = amd.ir_resample(x, a, b, host=True)
    assert same(np.ascontiguousarray(got[:, :one.shape[1]]), one) and one.shape[1] >= got.shape[1] - 8


def test_equal_rates_are_a_copy():
    x = noise((3, 500), 4)
    src = amd.StreamResampler(3, 48000, 48000.0000001, 256, host=True)
    assert src.latency == 0 and src.max_out == 256
    got, counts = stream(src, x, [256, 0, 244])
    assert same(got, x) and counts == [256, 0, 244]


def test_non_finite_samples(case):
    a, b, d = case["a"], case["b"], case["d"]
    L, Mm, T = d["L"], d["M"], d["T"]
    x = np.array(case["x"])
    n = x.shape[1]
    at = {0: (400, np.nan), 1: (900, np.inf)}
    for ch, (i, v) in at.items():
        x[ch, i] = v
    got, _ = stream(amd.StreamResampler(2, a, b, 4096, host=True), x, ragged(n, 12))
    j = np.arange(got.shape[1])
    centre = j * Mm // L + T // 2
    for ch, (i, _) in at.items():
        covered = (centre - (T - 1) <= i) & (i <= centre)           # the window of output j: centre - T + 1 ... centre
        assert np.array_equal(~np.isfinite(got[ch]), covered)
        assert np.array_equal(got[ch, ~covered].view(np.uint64), case["whole"][ch, ~covered].view(np.uint64))


def _raw(src, rows, n_in, in_stride, out, out_stride, cap, flush=0, null_in=False, null_out=False, null_n=False):
    n = C.c_int32(-7)
    rc = K.load().cpq_src_process(src._h, None if null_in else rows.ctypes.data, in_stride, n_in, None if null_out else out.ctypes.data, out_stride,
                                  cap, flush, None if null_n else C.byref(n))
    return rc, n.value


def test_refusals(case):
    a, b, x = case["a"], case["b"], case["x"]
    lib = K.load()
    h = C.c_void_p()
    for desc, status in ((K.SrcDesc(0, a, b, 64, 0, K.CPQ_SRC_HOST, 0), K.CPQ_ERR_INVALID_ARG),
                         (K.SrcDesc(2, a, b, 0, 0, K.CPQ_SRC_HOST, 0), K.CPQ_ERR_INVALID_ARG),
                         (K.SrcDesc(2, a, b, 64, 0, K.CPQ_SRC_HOST, -1), K.CPQ_ERR_INVALID_ARG),
                         (K.SrcDesc(2, a, b, 64, K.CPQ_RESAMPLE_MINIMUM_PHASE, K.CPQ_SRC_HOST, 0), K.CPQ_ERR_UNSUPPORTED),
                         (K.SrcDesc(2, 44100.5, b, 64, 0, K.CPQ_SRC_HOST, 0), K.CPQ_ERR_UNSUPPORTED),
                         (K.SrcDesc(2, 44101, b, 64, 0, K.CPQ_SRC_HOST, 0), K.CPQ_ERR_UNSUPPORTED),
                         (K.SrcDesc(2, 7999, b, 64, 0, K.CPQ_SRC_HOST, 0), K.CPQ_ERR_UNSUPPORTED)):
        assert lib.cpq_src_create(C.byref(desc), C.byref(h)) == status and not h.value
        assert lib.cpq_src_last_error(None)
    assert lib.cpq_src_create(None, C.byref(h)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_src_create(C.byref(K.SrcDesc(2, a, b, 64, 0, K.CPQ_SRC_HOST, 0)), None) == K.CPQ_ERR_INVALID_ARG

    n = x.shape[1]
    src = amd.StreamResampler(2, a, b, 1000, host=True)
    first = src.process(x[:, :700])
    count = src.out_count(537)
    assert count > 8
    rows = np.ascontiguousarray(x[:, 700:])
    both = np.zeros(2 * 2000)                          # rows of in and out inside one array
    out = np.zeros((2, count))
    bad = [_raw(src, rows, 537, 537, out, count, count, null_in=True), _raw(src, rows, 537, 537, out, count, count, null_out=True),
           _raw(src, rows, 537, 537, out, count, count, null_n=True), _raw(src, rows, 1001, 1001, out, count, count),
           _raw(src, rows, -1, 537, out, count, count), _raw(src, rows, 537, 536, out, count, count),
           _raw(src, rows, 537, 537, out, count - 1, count), _raw(src, rows, 537, 537, out, count, count - 1),
           _raw(src, both, 537, 537, both[600:], count, count), _raw(src, both[count:], 537, 537, both, count, count)]
    assert [rc for rc, _ in bad] == [K.CPQ_ERR_INVALID_ARG] * len(bad)
    assert all(n_out == -7 for _, n_out in bad)                 # a refused call writes neither *n_out ...
    assert not out.any() and not both.any()                     # ... nor a sample
    assert lib.cpq_src_last_error(src._h)
    assert lib.cpq_src_process(None, rows.ctypes.data, 537, 537, out.ctypes.data, count, count, 0, None) == K.CPQ_ERR_INVALID_ARG
    assert src.out_count(537) == count                          # nothing moved
    with pytest.raises(amd.CpqError):
        src.out_count(1001)
    rest = src.process(rows, flush=True)
    assert same(np.concatenate([first, rest], axis=1), case["whole"])


def test_the_device_object_is_refused_not_replaced():
    with pytest.raises(amd.CpqError) as e:
        amd.StreamResampler(2, 44100, 48000, 64)
    assert e.value.status == K.CPQ_ERR_UNSUPPORTED


def test_plan_and_host_object_under_sanitizers(tmp_path):
    """tests/sanitize/src_plan_check.cpp: src_plan.hpp and resample_design.cpp as a program of their own under ASan and UBSan --
    positions beyond 2^40, the rebasing identity, calls that tile the outputs, reads within the kept history, the history bound"""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "convopeq_amd", "csrc")
    exe = tmp_path / "src_plan_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + csrc, "-I" + os.path.join(root, "include"),
                    os.path.join(HERE, "sanitize", "src_plan_check.cpp"), os.path.join(csrc, "resample_design.cpp"),
                    os.path.join(csrc, "ir_ingest.cpp"), "-o", str(exe), "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failed checks" in r.stdout and "FAILED" not in r.stdout
