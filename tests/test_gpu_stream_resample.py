"""k_src_resample and k_src_keep through the device object of cpq_src (StreamResampler(device=True)).

The reference of every case is the host object (host=True) fed the same calls.  Device and host read one table and add in one
order, so every comparison of samples is for equal shape and equal bits (uint64 views): there is no tolerance.  The one exception
is a non-finite sample, whose spread is compared output for output and whose NaN payload is not.  Shapes follow the kernels:
T = 600 taps at 44100 -> 48000, tiles of 256 outputs (64 once M > 8 L), the virtual row staged 256 taps at a time, the kept
history moved 256 samples at a time."""
import ctypes as C

import numpy as np
import pytest
import torch

import convopeq_amd as amd
import resample_model as M
from convopeq_amd import _capi as K

pytestmark = pytest.mark.gpu

A, B, T = 44100, 48000, 600
PAIRS = [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000), (96000, 8000), (8000, 96000), (768000, 8000)]
PAIR_IDS = ["160:147", "147:160", "2:1", "1:2", "1:12 (tile 64)", "12:1", "1:96 (tile 64)"]
SENTINEL = 1234.5


def noise(shape, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, size=shape)


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def run(src, x, calls):
    """x through src.process in calls of (size, flush); every call's count is checked against out_count.  Returns the pieces."""
    out, at = [], 0
    for size, flush in calls:
        expect = src.out_count(size, flush)
        y = src.process(x[:, at:at + size], flush=flush)
        assert y.shape == (x.shape[0], expect)
        out.append(y)
        at += size
    assert at == x.shape[1]
    return out


def cat(pieces):
    return np.ascontiguousarray(np.concatenate(pieces, axis=1))


def plain(sizes, n):
    """call lengths `sizes`, then the rest of n with the flush"""
    assert sum(sizes) <= n
    return [(s, False) for s in sizes] + [(n - sum(sizes), True)]


def both(x, calls, a=A, b=B, max_in=5000, **kw):
    """the same calls through a fresh device object and a fresh host object: every piece equal; returns the host's pieces"""
    n_ch = x.shape[0]
    got = run(amd.StreamResampler(n_ch, a, b, max_in, device=True, **kw), x, calls)
    want = run(amd.StreamResampler(n_ch, a, b, max_in, host=True, **kw), x, calls)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), f"call {i} of {calls[i]}"
    return want


def length_for(src, count):
    """the call length that makes the next call emit `count` samples, or None where no length does (a ratio above 1 emits two
    samples for some inputs)"""
    n = 0
    while src.out_count(n) < count:
        n += 1
    return n if src.out_count(n) == count else None


@pytest.fixture(scope="module")
def case():
    """3 channels x 5000 samples at 44100 -> 48000, and the host object's output for the whole stream in one call"""
    assert amd.resample_design(A, B)["T"] == T
    x = noise((3, 5000), 1)
    x.setflags(write=False)
    whole = cat(run(amd.StreamResampler(3, A, B, 5000, host=True), x, [(5000, True)]))
    whole.setflags(write=False)
    assert whole.shape == (3, M.out_len(5000, A, B))
    return {"x": x, "whole": whole}


def tile_counts_split(n):
    probe = amd.StreamResampler(1, A, B, 5000, host=True)
    z, sizes = np.zeros((1, 5000)), [T]
    probe.process(z[:, :T])
    for count in (255, 256, 257, 513):
        while length_for(probe, count) is None:         # a call of one sample moves the stream to where the count exists
            sizes.append(1)
            probe.process(z[:, :1])
        sizes.append(length_for(probe, count))
        assert probe.process(z[:, :sizes[-1]]).shape[1] == count
    return plain(sizes, n)


def random_split(n, seed, calls=40):
    at = np.sort(np.random.default_rng(seed).integers(0, n + 1, size=calls - 1))
    sizes = np.diff(np.concatenate([[0], at])).tolist()
    return plain(sizes, n)


SPLITS = {"one call": lambda n: [(n, True)],
          "700 singles": lambda n: plain([1] * 700, n),
          "calls of nothing between others": lambda n: [(0, False), (300, False), (0, False), (0, False), (1000, False), (0, False), (n - 1300, False), (0, True)],
          "around the latency": lambda n: plain([T // 2 - 1, T // 2, T // 2 + 1], n),
          "around the tile": tile_counts_split,
          "random 40": lambda n: random_split(n, 5)}


@pytest.mark.parametrize("name", list(SPLITS))
def test_call_splits(case, name):
    x = case["x"]
    calls = SPLITS[name](x.shape[1])
    want = both(x, calls)
    assert same(cat(want), case["whole"])               # and so the device's concatenation is the one-call stream


def test_one_shot_parity(case):
    x, whole = case["x"], case["whole"]
    got = cat(run(amd.StreamResampler(3, A, B, 5000, device=True), x, random_split(5000, 6, calls=9)))
    assert same(got, whole)
    one = amd.ir_resample(x, A, B, host=True)
    n_out = whole.shape[1]
    assert n_out - 8 <= one.shape[1] <= n_out           # undamped noise: the IR path trims at most the last 8 samples
    assert same(np.ascontiguousarray(got[:, :one.shape[1]]), one)
    d = amd.resample_design(A, B)
    idx = np.arange(one.shape[1] - 1, n_out)            # what the trim took: held to the longdouble model
    u = 2.0 ** -53
    for ch in range(3):
        model, bound = M.resample_rows(d, x[ch], outputs=idx)
        limit = (T * u / (1 - T * u) + T * 2.0 ** -63) * bound
        assert np.all(np.abs(got[ch, idx].astype(np.longdouble) - model) <= limit)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_ratios(pair):
    a, b = pair
    t = amd.resample_design(a, b)["T"]
    n = 2 * t + 37 if t < 4000 else 2500
    max_in = 1000 if t >= 4000 else t + 100
    x = noise((2, n), a % 1000 + b % 999)
    first, second = n // 5, min(max_in, n - n // 5 - 3)
    calls = [(first, False), (second, False), (n - first - second, False), (0, True)]
    assert all(s <= max_in for s, _ in calls)
    want = cat(both(x, calls, a, b, max_in))
    assert want.shape == (2, M.out_len(n, a, b))
    dev = amd.StreamResampler(2, a, b, max_in, device=True)
    assert dev.latency == t // 2 and dev.max_out == amd.StreamResampler(2, a, b, max_in, host=True).max_out


@pytest.mark.parametrize("n_ch", [1, 2, 65, 300])
def test_channel_counts(n_ch):
    x = noise((n_ch, 10 * 64), 20 + n_ch)
    calls = [(64, False)] * 9 + [(64, True)]
    want = cat(both(x, calls, max_in=64))
    assert n_ch == 1 or not same(want[:1], want[1:2])          # the channels differ
    perm = np.random.default_rng(n_ch).permutation(n_ch)       # a channel's output does not depend on its neighbours
    got = cat(run(amd.StreamResampler(n_ch, A, B, 64, device=True), np.ascontiguousarray(x[perm]), calls))
    assert same(got, np.ascontiguousarray(want[perm]))


def test_flush_in_mid_stream_and_reset(case):
    x = case["x"]
    calls = [(700, False), (900, True), (1, False), (1400, False), (0, True), (1999, True)]
    both(x, calls)
    dev, ref = amd.StreamResampler(3, A, B, 5000, device=True), amd.StreamResampler(3, A, B, 5000, host=True)
    for src in (dev, ref):
        src.process(noise((3, 777), 8))
        src.reset()
    assert same(cat(run(dev, x, random_split(5000, 9, calls=7))), case["whole"])
    assert same(cat(run(ref, x, [(5000, True)])), case["whole"])


@pytest.mark.parametrize("period", [3, 2 ** 40])
def test_start_period(case, period):
    x = case["x"]
    got = cat(run(amd.StreamResampler(3, A, B, 5000, device=True, start_period=period), x, random_split(5000, 7, calls=6)))
    assert same(got, case["whole"])


def test_two_objects_called_alternately(case):
    x = case["x"][:2, :3000]
    pairs = [(A, B), (96000, 8000)]
    devs = [amd.StreamResampler(2, a, b, 500, device=True) for a, b in pairs]
    refs = [amd.StreamResampler(2, a, b, 500, host=True) for a, b in pairs]
    for i, at in enumerate(range(0, 3000, 500)):
        for dev, ref in zip(devs, refs):
            flush = at + 500 == 3000
            g, w = dev.process(x[:, at:at + 500], flush=flush), ref.process(x[:, at:at + 500], flush=flush)
            assert same(g, w), (i, at)


# ---- the device-pointer entry

def dev_call(src, t_in, n_in, t_out, cap, flush=False, in_stride=None, out_stride=None, null_in=False, null_out=False, null_n=False):
    n = C.c_int32(-7)
    rc = K.load().cpq_src_process_device(src._h, None if null_in else C.c_void_p(t_in.data_ptr()), t_in.stride(0) if in_stride is None else in_stride,
                                         n_in, None if null_out else C.c_void_p(t_out.data_ptr()), t_out.stride(0) if out_stride is None else out_stride,
                                         cap, int(flush), None if null_n else C.byref(n))
    return rc, n.value


def test_device_rows_with_strides_and_a_sentinel(case):
    x, whole = case["x"], case["whole"]
    dev = amd.StreamResampler(3, A, B, 5000, device=True)
    wide_in = torch.full((3, 5000 + 13), SENTINEL, dtype=torch.float64, device="cuda")
    wide_in[:, :5000] = torch.from_numpy(np.array(x))
    at, col = 0, 0
    wide_out = torch.full((3, whole.shape[1] + 29), SENTINEL, dtype=torch.float64, device="cuda")
    for size, flush in [(1700, False), (0, False), (2300, False), (1000, True)]:
        count = dev.out_count(size, flush)
        rc, n = dev_call(dev, wide_in[:, at:], size, wide_out[:, col:], count, flush)       # out_capacity exactly out_count
        assert rc == K.CPQ_OK and n == count
        at, col = at + size, col + count
    torch.cuda.synchronize()
    got = wide_out.cpu().numpy()
    assert same(np.ascontiguousarray(got[:, :whole.shape[1]]), whole)
    assert np.all(got[:, whole.shape[1]:] == SENTINEL)                                       # beyond n_out, and the rows' padding
    assert np.all(wide_in[:, 5000:].cpu().numpy() == SENTINEL)
    # a call that writes fewer samples than the row holds leaves the rest
    dev2 = amd.StreamResampler(3, A, B, 5000, device=True)
    out = torch.full((3, 4000), SENTINEL, dtype=torch.float64, device="cuda")
    count = dev2.out_count(1700)
    rc, n = dev_call(dev2, wide_in, 1700, out, count)
    torch.cuda.synchronize()
    assert rc == K.CPQ_OK and n == count and same(np.ascontiguousarray(out.cpu().numpy()[:, :count]), np.ascontiguousarray(whole[:, :count]))
    assert np.all(out.cpu().numpy()[:, count:] == SENTINEL)


def test_process_device_tensors_on_a_stream(case):
    x, whole = case["x"], case["whole"]
    dev = amd.StreamResampler(3, A, B, 5000, device=True)
    stream = torch.cuda.Stream()
    t = torch.from_numpy(np.array(x)).cuda()
    torch.cuda.synchronize()
    dev.set_stream(stream)
    with torch.cuda.stream(stream):
        pieces = [dev.process_device(t[:, :1234]), dev.process_device(t[:, 1234:1234]), dev.process_device(t[:, 1234:], flush=True)]
    stream.synchronize()
    assert pieces[1].shape == (3, 0)
    assert same(cat([p.cpu().numpy() for p in pieces]), whole)
    dev.set_stream(None)                                # back on the null stream: the next stream starts from the flush
    assert same(dev.process(x, flush=True), whole)


def test_back_to_back_calls_without_synchronisation():
    """each call's hist was last written by the call before it, on the same stream, and nothing waits in between"""
    n_calls, size = 200, 7
    x = noise((2, n_calls * size), 30)
    want = cat(run(amd.StreamResampler(2, A, B, size, host=True), x, [(size, False)] * (n_calls - 1) + [(size, True)]))
    dev = amd.StreamResampler(2, A, B, size, device=True)
    t = torch.from_numpy(x).cuda()
    out = torch.full((2, want.shape[1] + 5), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    col = 0
    for i in range(n_calls):
        flush = i == n_calls - 1
        count = dev.out_count(size, flush)
        rc, n = dev_call(dev, t[:, i * size:], size, out[:, col:], count, flush)
        assert rc == K.CPQ_OK and n == count
        col += count
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert col == want.shape[1] and same(np.ascontiguousarray(got[:, :col]), want) and np.all(got[:, col:] == SENTINEL)


# ---- values

def test_non_finite_samples_spread_as_on_the_host(case):
    x = np.array(case["x"][:2])
    at = {0: (2400, np.nan), 1: (2900, np.inf)}
    for ch, (i, v) in at.items():
        x[ch, i] = v
    calls = random_split(5000, 12, calls=8)
    got = cat(run(amd.StreamResampler(2, A, B, 5000, device=True), x, calls))
    want = cat(run(amd.StreamResampler(2, A, B, 5000, host=True), x, calls))
    d = amd.resample_design(A, B)
    centre = np.arange(got.shape[1]) * d["M"] // d["L"] + T // 2
    for ch, (i, _) in at.items():
        covered = (centre - (T - 1) <= i) & (i <= centre)
        assert np.array_equal(~np.isfinite(got[ch]), ~np.isfinite(want[ch])) and np.array_equal(np.isnan(got[ch]), np.isnan(want[ch]))
        assert np.array_equal(~np.isfinite(want[ch]), covered) and covered.sum() > T
        assert np.array_equal(got[ch, ~covered].view(np.uint64), case["whole"][ch, ~covered].view(np.uint64))
        inf = np.isinf(want[ch])
        assert np.array_equal(got[ch, inf], want[ch, inf])


def test_denormals_and_zeros():
    rng = np.random.default_rng(40)
    tiny = np.float64(5e-324)
    x = np.empty((2, 2000))
    x[0] = rng.integers(1, 4, size=2000) * tiny * rng.choice([-1.0, 1.0], size=2000)       # sums that underflow to +-0 from the first output on
    x[1] = rng.uniform(-1.0, 1.0, size=2000) * 2.0 ** -1040                                # denormal products and sums
    calls = plain([T // 2 + 40, 3, 700], 2000)
    want = cat(both(x, calls, max_in=2000))
    assert np.any(want[1] != 0.0) and np.all(np.abs(want) < 2.0 ** -1000)
    zeros = cat(both(np.zeros((2, 2000)), calls, max_in=2000))
    assert not zeros.view(np.uint64).any()              # +0.0, never -0.0


def test_equal_rates_are_a_copy_with_strides():
    x = noise((3, 500), 4)
    dev = amd.StreamResampler(3, 48000, 48000.0000001, 256, device=True)
    assert dev.latency == 0 and dev.max_out == 256
    got = run(dev, x, [(256, False), (0, False), (244, True)])
    assert same(cat(got), x) and [g.shape[1] for g in got] == [256, 0, 244]
    t = torch.full((3, 300), SENTINEL, dtype=torch.float64, device="cuda")
    t[:, :256] = torch.from_numpy(x[:, :256])
    out = torch.full((3, 270), SENTINEL, dtype=torch.float64, device="cuda")
    rc, n = dev_call(dev, t, 256, out, 256)
    torch.cuda.synchronize()
    assert rc == K.CPQ_OK and n == 256
    got = out.cpu().numpy()
    assert same(np.ascontiguousarray(got[:, :256]), np.ascontiguousarray(x[:, :256])) and np.all(got[:, 256:] == SENTINEL)


# ---- refusals

def _raw(src, rows, n_in, in_stride, out, out_stride, cap, flush=0, null_in=False, null_out=False, null_n=False):
    n = C.c_int32(-7)
    rc = K.load().cpq_src_process(src._h, None if null_in else rows.ctypes.data, in_stride, n_in, None if null_out else out.ctypes.data, out_stride,
                                  cap, flush, None if null_n else C.byref(n))
    return rc, n.value


def test_refusals_leave_the_device_object_as_it_was(case):
    """test_stream_resample_cpu.py's call refusals on the device object, through both entry points, each with nothing moved"""
    x, whole = case["x"][:2], case["whole"][:2]
    lib = K.load()
    src = amd.StreamResampler(2, A, B, 1000, device=True)
    first = src.process(x[:, :700])
    count = src.out_count(537)
    assert count > 8
    rows = np.ascontiguousarray(x[:, 700:1237])
    both_ = np.zeros(2 * 2000)
    out = np.zeros((2, count))
    t_rows = torch.from_numpy(rows).cuda()
    t_both = torch.zeros(2 * 2000, dtype=torch.float64, device="cuda")
    t_out = torch.zeros((2, count), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    host_rows = [lambda: _raw(src, rows, 537, 537, out, count, count, null_in=True), lambda: _raw(src, rows, 537, 537, out, count, count, null_out=True),
                 lambda: _raw(src, rows, 537, 537, out, count, count, null_n=True), lambda: _raw(src, rows, 1001, 1001, out, count, count),
                 lambda: _raw(src, rows, -1, 537, out, count, count), lambda: _raw(src, rows, 537, 536, out, count, count),
                 lambda: _raw(src, rows, 537, 537, out, count - 1, count), lambda: _raw(src, rows, 537, 537, out, count, count - 1),
                 lambda: _raw(src, both_, 537, 537, both_[600:], count, count), lambda: _raw(src, both_[count:], 537, 537, both_, count, count)]
    device_rows = [lambda: dev_call(src, t_rows, 537, t_out, count, null_in=True), lambda: dev_call(src, t_rows, 537, t_out, count, null_out=True),
                   lambda: dev_call(src, t_rows, 537, t_out, count, null_n=True), lambda: dev_call(src, t_rows, 1001, t_out, count, in_stride=1001),
                   lambda: dev_call(src, t_rows, -1, t_out, count), lambda: dev_call(src, t_rows, 537, t_out, count, in_stride=536),
                   lambda: dev_call(src, t_rows, 537, t_out, count, out_stride=count - 1), lambda: dev_call(src, t_rows, 537, t_out, count - 1),
                   lambda: dev_call(src, t_both, 537, t_both[600:], count, in_stride=537, out_stride=count),
                   lambda: dev_call(src, t_both[count:], 537, t_both, count, in_stride=537, out_stride=count)]
    for i, refused in enumerate(host_rows + device_rows):
        rc, n_out = refused()
        assert rc == K.CPQ_ERR_INVALID_ARG and n_out == -7, i       # a refused call writes neither *n_out ...
        assert lib.cpq_src_last_error(src._h)
        assert src.out_count(537) == count, i                       # ... nor moves the state
    torch.cuda.synchronize()
    assert not out.any() and not both_.any() and not t_out.cpu().numpy().any() and not t_both.cpu().numpy().any()       # ... nor a sample
    assert lib.cpq_src_process_device(None, None, 537, 537, None, count, count, 0, None) == K.CPQ_ERR_INVALID_ARG
    with pytest.raises(amd.CpqError):
        src.out_count(1001)
    # the object gives the bits of one that was never refused
    middle = src.process(rows)
    rest = src.process(x[:, 1237:2237])
    assert same(cat([first, middle, rest]), np.ascontiguousarray(whole[:, :first.shape[1] + middle.shape[1] + rest.shape[1]]))


def test_last_kernel_ms(case):
    x = case["x"]
    dev, ref = amd.StreamResampler(3, A, B, 5000, device=True), amd.StreamResampler(3, A, B, 5000, host=True)
    assert dev.last_kernel_ms == -1.0                   # no host-row call yet
    dev.process(x[:, :3000])
    ref.process(x[:, :3000])
    assert dev.last_kernel_ms > 0.0 and ref.last_kernel_ms == -1.0
