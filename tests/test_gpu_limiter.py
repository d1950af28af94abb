"""k_lim_apply and k_lim_keep through the device object of cpq_limiter (TruePeakLimiter(device=True)).

The reference of every case is the host object (host=True) fed the same calls.  Device and host evaluate one definition in one
order (csrc/lim_plan.hpp), so every comparison is for equal shape and equal bits (uint64 views): there is no tolerance.  Shapes
follow the kernels: tiles of 1024 outputs, a halo of 2 W + 21 samples, r in rounds of 256, the kept history moved 256 samples at
a time; no row is longer than 5 tiles.  The windows at which one of those rules changes, and rows of more than 256 tiles, are
tests/test_gpu_limiter_windows.py's; the numpy helpers both files use are tests/limiter_window_cases.py's."""
import numpy as np
import pytest
import torch

import convopeq_amd as amd
from limiter_window_cases import CEIL_DB, RATE, TILE, gains, host_pieces, noise, plant, same

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
WINDOWS = (8, 72, 1024)


def pair(n_streams, W, rate=RATE):
    dev = amd.TruePeakLimiter(n_streams, rate, CEIL_DB, W, device=True)
    host = amd.TruePeakLimiter(n_streams, rate, CEIL_DB, W, host=True)
    for lim in (dev, host):
        lim.set_gains(gains(n_streams))
    return dev, host


def device_pieces(dev, x, lengths, stride_pad=0, in_place=False, sync_each=True):
    """the same calls on device rows: every call's rows lie inside a wider buffer filled with a sentinel, which must survive"""
    t = torch.from_numpy(x).cuda()
    out, at, bufs = [], 0, []
    for k in lengths:
        stride = k + stride_pad
        if in_place:
            buf = torch.full((x.shape[0], stride), SENTINEL, dtype=torch.float64, device="cuda")
            buf[:, :k] = t[:, at:at + k]
            y = dev.process_device(buf[:, :k], buf[:, :k])
            src = None
        else:
            src = torch.full((x.shape[0], stride), SENTINEL, dtype=torch.float64, device="cuda")
            src[:, :k] = t[:, at:at + k]
            buf = torch.full((x.shape[0], stride), SENTINEL, dtype=torch.float64, device="cuda")
            y = dev.process_device(src[:, :k], buf[:, :k])
        assert y.shape == (x.shape[0], k)
        bufs.append((buf, src, k))
        at += k
    D = dev.latency
    fl = torch.full((x.shape[0], ((D + 1) & ~1) + stride_pad), SENTINEL, dtype=torch.float64, device="cuda")
    dev.flush_device(fl)
    torch.cuda.synchronize()
    for buf, src, k in bufs:
        b = buf.cpu().numpy()
        assert (b[:, k:] == SENTINEL).all()
        if src is not None:
            assert (src.cpu().numpy()[:, k:] == SENTINEL).all()
        out.append(b[:, :k])
    f = fl.cpu().numpy()
    assert (f[:, D:] == SENTINEL).all()
    out.append(f[:, :D])
    return out


def check(dev, host, x, lengths, **kw):
    got = device_pieces(dev, x, lengths, **kw)
    want = host_pieces(host, x, lengths)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), f"call {i} of {lengths}: {int((g.view(np.uint64) != w.view(np.uint64)).sum())} doubles differ"
    td, th = dev.telemetry(), host.telemetry()
    assert td == th
    return th


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("n_streams", (1, 3, 65))
def test_call_lengths_around_the_latency_and_the_tile(W, n_streams):
    D = W + 11
    lengths = [1, 7, D, D + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
    if n_streams == 65:
        lengths = [7, D + 1, TILE + 1, 2 * TILE + 5]
    n = sum(lengths)
    x = noise(n_streams, n, 10 * W + n_streams)
    starts = np.cumsum([0] + lengths)
    last = int(starts[-2])                      # the long call's first sample
    plant(x, 0)                                 # sample 0 of the programme
    plant(x, int(starts[4]) - 1)                # the last sample of a call: the reduction spans a call boundary
    plant(x, last + TILE - 1)                   # the last sample of a tile
    plant(x, last + 2 * TILE)                   # the first sample of a tile
    dev, host = pair(n_streams, W)
    tel = check(dev, host, x, lengths, stride_pad=2 if n_streams != 3 else 3)      # 3: odd strides, the scalar path
    assert all(t["limited_samples"] > 0 and t["min_gain"] < 1.0 for t in tel)


@pytest.mark.parametrize("W", WINDOWS)
def test_peaks_closer_than_the_window_and_further_apart_than_both(W):
    M = W + 12
    n = 4 * TILE + 5
    x = noise(2, n, W, level=0.05)
    a = TILE - W // 2
    plant(x, a)
    plant(x, a + W - 1, amp=1.9)                # closer than W: one dip
    plant(x, a + W - 1 + M + W + 40, amp=3.1)   # further apart than M + W: the envelope returns to 1.0 in between
    dev, host = pair(2, W)
    check(dev, host, x, [n])
    y = np.concatenate(host_pieces(host, x, [n]), axis=1)
    lim = amd.TruePeakLimiter(2, RATE, CEIL_DB, W, host=True)
    assert np.abs(y).max() <= lim.ceiling + (W + 3) * np.spacing(lim.ceiling)


@pytest.mark.parametrize("W", (8, 1024))
def test_in_place(W):
    lengths = [TILE + 1, 7, 2 * TILE + 5]
    x = plant(plant(noise(3, sum(lengths), 5 + W), TILE), TILE + 9)
    dev, host = pair(3, W)
    check(dev, host, x, lengths, in_place=True, stride_pad=4)


def test_overlapping_rows_are_refused_and_move_nothing():
    dev, host = pair(1, 8)
    buf = torch.zeros((2, 64), dtype=torch.float64, device="cuda")
    flat = buf.view(-1)
    with pytest.raises(amd.CpqError):
        dev.process_device(flat[0:64].view(2, 32), flat[16:80].view(2, 32))
    with pytest.raises(amd.CpqError):
        dev.process_device(flat[1:65].view(2, 32), buf[:, :32].clone())         # not 16-byte aligned
    x = plant(noise(1, 300, 1), 100)
    check(dev, host, x, [300])


def test_a_non_default_stream_and_calls_without_a_synchronisation():
    W, k, calls = 72, 200, 100
    x = noise(2, k * calls, 77)
    for at in range(150, k * calls, 997):
        plant(x, at)
    plant(x, 5 * k - 1)
    plant(x, 5 * k)
    dev, host = pair(2, W)
    stream = torch.cuda.Stream()
    t = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    dev.set_stream(stream)
    with torch.cuda.stream(stream):
        out = torch.empty_like(t)
        for i in range(calls):
            dev.process_device(t[:, i * k:(i + 1) * k], out[:, i * k:(i + 1) * k])
        tail = dev.flush_device()
    stream.synchronize()
    want = host_pieces(host, x, [k] * calls)
    assert same(out.cpu().numpy(), np.concatenate(want[:-1], axis=1))
    assert same(tail.cpu().numpy(), want[-1])
    assert dev.telemetry() == host.telemetry()
    assert dev.last_kernel_ms > 0.0
    dev.set_stream(None)


def test_flush_then_a_second_programme_and_reset():
    W = 72
    dev, host = pair(3, W)
    x1 = plant(noise(3, 2 * TILE + 5, 1), TILE - 1)
    x2 = plant(noise(3, TILE + 40, 2), 3)
    t1 = check(dev, host, x1, [TILE, TILE + 5])
    t2 = check(dev, host, x2, [TILE + 40])
    assert t1 != t2
    for lim in (dev, host):
        lim.process(x1[:, :500])
        with pytest.raises(amd.CpqError):
            lim.set_gains(np.ones(3))           # a programme has started
        lim.reset()
        assert lim.telemetry() == [{"min_gain": 1.0, "limited_samples": 0}] * 3
    assert check(dev, host, x2, [40, TILE]) == t2


def test_host_rows_through_the_device_object():
    W = 8
    dev, host = pair(2, W)
    x = plant(noise(2, TILE + 77, 9), TILE)
    got = [dev.process(x[:, :TILE]), dev.process(x[:, TILE:]), dev.flush()]
    want = host_pieces(host, x, [TILE, 77])
    assert all(same(g, w) for g, w in zip(got, want))
    assert dev.telemetry() == host.telemetry()


def test_host_rows_that_grow_around_a_call_in_place():
    """host rows of 7, TILE + 1 and 2 TILE + 5 samples: the object's row buffers are replaced before the second and the third
    call.  Between those two a call in place on device rows of TILE + 3 samples, whose copy lies in the buffer the host rows go
    through, and replaces it as well."""
    W = 8
    lengths = [7, TILE + 1, TILE + 3, 2 * TILE + 5]
    starts = np.cumsum([0] + lengths)
    x = noise(2, sum(lengths), 31)
    plant(x, TILE)
    plant(x, int(starts[2]) - 1)                # the last sample of the second call
    dev, host = pair(2, W)
    got = [dev.process(x[:, starts[0]:starts[1]]), dev.process(x[:, starts[1]:starts[2]])]
    buf = torch.from_numpy(np.ascontiguousarray(x[:, starts[2]:starts[3]])).cuda()
    assert dev.process_device(buf, buf) is buf
    got += [buf.cpu().numpy(), dev.process(x[:, starts[3]:starts[4]]), dev.flush()]
    want = host_pieces(host, x, lengths)
    assert len(got) == len(want) == 5
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), f"piece {i}: {int((np.ascontiguousarray(g).view(np.uint64) != w.view(np.uint64)).sum())} doubles differ"
    tel = dev.telemetry()
    assert tel == host.telemetry() and all(t["limited_samples"] > 0 and t["min_gain"] < 1.0 for t in tel)


def test_a_sample_that_is_not_finite():
    W = 72
    x = plant(noise(2, TILE + 300, 4), 700)
    x[0, TILE - 1] = np.nan
    x[1, TILE] = np.inf
    x[3, 5] = -np.inf
    x[2, TILE + 299] = 1.0e300
    dev, host = pair(2, W)
    check(dev, host, x, [TILE + 300])
    y = np.concatenate(host_pieces(host, x, [TILE + 300]), axis=1)
    assert np.isfinite(y).all() and y[0, TILE - 1 + W + 11] == 0.0 and y[1, TILE + W + 11] == 0.0


@pytest.mark.parametrize("rate", (96000, 192000), ids=("phases 0 and 2", "no phase"))
def test_the_other_phase_rules(rate):
    W = 72
    x = plant(plant(noise(2, TILE + 300, rate), TILE - 1), TILE)
    dev, host = pair(2, W, rate)
    check(dev, host, x, [TILE + 300])
