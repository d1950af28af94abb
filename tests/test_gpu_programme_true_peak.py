"""GPU tests of the true peak per programme and the normalisation of cpq_loudness (k_prog_peak and k_prog_apply in
convopeq_amd/csrc/prog_kernels.hip) through the C ABI.  Every comparison of peaks is bit for bit against the numpy model
tests/prog_peak_model.py: a maximum does not depend on order, and the 12-term sum has one order.  The rate is 8000 Hz unless
said otherwise; rows are a few thousand samples."""
import ctypes as C
import math

import numpy as np
import pytest

import prog_peak_model as PK

pytestmark = pytest.mark.gpu

RATE = 8000
TILE = 4096


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def splits(n, piece):
    return [piece] * (n // piece) + ([n % piece] if n % piece else [])


def device_peaks(amd, x, calls=None, rate=RATE, obj=None):
    """(true_peak, sample_peak) per row of x [2 S, n], fed through cpq_loudness_process in `calls`"""
    own = obj is None
    if own:
        obj = amd.ProgrammeLoudness(x.shape[0] // 2, rate, x.shape[1] / rate + 1, true_peak=True)
    o = 0
    for n in [x.shape[1]] if calls is None else calls:
        obj.process(x[:, o:o + n])
        o += n
    assert o == x.shape[1]
    pk = obj.peaks()
    if own:
        obj.close()
    return (np.array([v for p in pk for v in p["true_peak"]]), np.array([v for p in pk for v in p["sample_peak"]]))


def check(got, x, rate, label):
    want = PK.peaks(x, rate)
    for g, w, what in zip(got, want, ("true peak", "sample peak")):
        bad = np.nonzero(bits(g) != bits(w))[0]
        assert len(bad) == 0, (label, what, "rows", bad[:8], g[bad[:8]], w[bad[:8]])
    return want


def planted(S, n, seed):
    """quiet noise, and one sample per stream that towers over it where a kernel can lose it: the programme's first and last
    sample and the 11 samples on either side of every tile seam; a different place, size and sign per stream, in the right
    channel only for every third stream"""
    rng = np.random.default_rng(seed)
    x = 0.01 * rng.standard_normal((2 * S, n))
    places = [0, n - 1] + [p for seam in range(TILE, n + 12, TILE) for p in range(seam - 11, seam + 11) if 0 < p < n - 1]
    for s in range(S):
        ch = 1 if s % 3 == 0 else (s // 3) % 2
        x[2 * s + ch, places[(s + (n % 7 if s > 1 else 0)) % len(places)]] = (1.0 + 0.01 * s) * (-1.0 if s % 2 else 1.0)
    return x


@pytest.mark.parametrize("S", (1, 3, 65))
@pytest.mark.parametrize("n", (4095, 4096, 4097, 8193))
def test_a_maximum_planted_where_the_kernel_can_lose_it(amd, S, n):
    x = planted(S, n, 100 * S + n)
    tp, sp = check(device_peaks(amd, x), x, RATE, f"{S} streams of {n}")
    spikes = np.abs(x).max(axis=1) >= 1.0
    assert spikes.sum() == S and np.all(sp[spikes] >= 1.0) and np.all(tp[~spikes] < 0.1)
    # ... and the same programme cut at the seam and one sample to either side of it
    for cut in (TILE - 1, TILE, TILE + 1):
        if cut < n:
            check(device_peaks(amd, x, [cut, n - cut]), x, RATE, f"{S} streams of {n} cut at {cut}")


@pytest.mark.parametrize("S", (1, 3))
def test_an_inter_sample_peak_whose_window_straddles_two_calls(amd, S):
    n, k = 600, 300
    rng = np.random.default_rng(4)
    x = 0.001 * rng.standard_normal((2 * S, n))
    for s in range(S):
        x[2 * s + s % 2, k - 1 - s:k + 1 - s] = -0.9 if s % 2 else 0.9        # two equal neighbours: the peak lies between them
    tp, sp = check(device_peaks(amd, x, [k, n - k]), x, RATE, "straddling")
    for s in range(S):
        r = 2 * s + s % 2
        assert tp[r] > 1.05 * sp[r] and sp[r] == 0.9
        y = np.concatenate([PK.interpolated(x[r:r + 1], p) for p in range(4)])
        at = int(np.unravel_index(y.argmax(), y.shape)[1])
        assert at >= k and at - 11 < k              # the window of the maximum holds samples of both calls
    check(device_peaks(amd, x, [k - 1, 1, 1, n - k - 1]), x, RATE, "straddling, calls of one sample at the peak")


@pytest.mark.parametrize("piece", (1, 10, 11, 12))
def test_calls_shorter_than_and_around_the_history(amd, piece):
    S, n = 3, 61
    rng = np.random.default_rng(piece)
    x = rng.uniform(-1.0, 1.0, (2 * S, n))
    check(device_peaks(amd, x, splits(n, piece)), x, RATE, f"calls of {piece}")
    if piece == 1:                                  # the first sample alone: zero history
        check(device_peaks(amd, x[:, :1]), x[:, :1], RATE, "one sample")


@pytest.mark.parametrize("S", (1, 3, 65))
def test_random_calls_against_one_call(amd, S):
    n = 9000
    rng = np.random.default_rng(S)
    x = 0.3 * rng.standard_normal((2 * S, n))
    calls = []
    while sum(calls) < n:
        calls.append(int(min(n - sum(calls), rng.integers(1, 30) if len(calls) % 3 == 0 else rng.integers(1, 5000))))
    one = device_peaks(amd, x)
    cut = device_peaks(amd, x, calls)
    check(one, x, RATE, "one call")
    assert np.array_equal(bits(one[0]), bits(cut[0])) and np.array_equal(bits(one[1]), bits(cut[1]))


@pytest.mark.parametrize("extra", (1, 2, 7, 24))
def test_row_strides_above_n_and_odd_ones(amd, extra):
    """device rows with sentinels of 50.0 between them: a kernel that reads past a row reads a peak of 50"""
    import torch
    S, n = 3, 4097
    stride = n + extra
    x = planted(S, n, extra)
    flat = torch.full((2 * S * stride + 8,), 50.0, dtype=torch.float64, device="cuda")
    rows = flat[2:2 + 2 * S * stride].view(2 * S, stride)       # 16 bytes in: still aligned
    rows[:, :n] = torch.from_numpy(x).cuda()
    before = flat.clone()
    obj = amd.ProgrammeLoudness(S, RATE, 10, true_peak=True)
    torch.cuda.synchronize()
    obj.process_device(rows[:, :n])
    pk = obj.peaks()
    obj.close()
    assert torch.equal(flat, before)                # the rows are read, never written
    got = (np.array([v for p in pk for v in p["true_peak"]]), np.array([v for p in pk for v in p["sample_peak"]]))
    check(got, x, RATE, f"stride n + {extra}")


def test_nan_inf_and_huge_values_are_scrubbed(amd):
    S, n = 3, 4200
    rng = np.random.default_rng(8)
    x = 0.2 * rng.standard_normal((2 * S, n))
    clean = x.copy()
    for r, (at, v) in enumerate(((0, np.nan), (n - 1, np.inf), (4095, -np.inf), (4096, 1e300), (17, -1e300), (4107, np.nan))):
        x[r, at] = v
        clean[r, at] = 0.0
    x[0, 100:130] = np.nan
    clean[0, 100:130] = 0.0
    got = device_peaks(amd, x, [4090, 110])
    check(got, x, RATE, "scrubbed")
    check(got, clean, RATE, "the peak of the rest")
    assert np.all(np.isfinite(got[0])) and np.all(got[1] < 2.0)
    big = np.full((2, 40), 9.9e299)                 # just below the scrub: taken, and the sum does not overflow
    check(device_peaks(amd, big), big, RATE, "9.9e299")


def test_denormals_and_zeros(amd):
    rng = np.random.default_rng(9)
    x = rng.standard_normal((4, 500)) * 1e-310
    x[2:] = 0.0
    x[3, 7] = -0.0
    tp, sp = check(device_peaks(amd, x, [250, 250]), x, RATE, "denormals")
    assert np.all(tp[:2] > 0.0) and np.all(tp[:2] < 1e-307)
    assert bits(tp[2:]).tolist() == [0, 0] and bits(sp[2:]).tolist() == [0, 0]


@pytest.mark.parametrize("rate", (48000, 88200, 96000, 176400, 192000))
def test_phases_by_rate(amd, rate):
    n = 5000
    x = np.zeros((2, n))
    x[0] = 0.5 * np.sin(2.0 * np.pi * np.arange(n) / 4.0 + math.pi / 4.0)      # fs / 4 at 45 degrees: the peaks lie between samples
    x[1] = -0.5 * x[0]
    tp, sp = check(device_peaks(amd, x, rate=rate), x, rate, f"{rate} Hz")
    if rate >= 176400:
        assert np.array_equal(bits(tp), bits(sp))
    else:
        assert np.all(tp > 1.2 * sp)


def test_reset_the_switch_and_the_hop_sums(amd):
    lib, K = amd._capi.load(), amd._capi
    S, n = 3, 8193
    x = planted(S, n, 1)
    plain = amd.ProgrammeLoudness(S, RATE, 10)
    res = (K.LoudnessPeaks * S)()
    assert lib.cpq_loudness_read_peaks(plain._h, res) == K.CPQ_ERR_NOT_READY and lib.cpq_loudness_last_error(plain._h)
    assert lib.cpq_loudness_read_peaks(plain._h, None) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_set_true_peak(plain._h, 2) == K.CPQ_ERR_INVALID_ARG
    plain.process(x[:, :5000])
    # the switch is refused in mid-programme, and nothing has moved
    assert lib.cpq_loudness_set_true_peak(plain._h, 1) == K.CPQ_ERR_NOT_READY
    assert b"start of a programme" in lib.cpq_loudness_last_error(plain._h)
    assert lib.cpq_loudness_read_peaks(plain._h, res) == K.CPQ_ERR_NOT_READY
    plain.process(x[:, 5000:])
    on = amd.ProgrammeLoudness(S, RATE, 10, true_peak=True)
    on.process(x[:, :5000])
    assert lib.cpq_loudness_set_true_peak(on._h, 0) == K.CPQ_ERR_NOT_READY
    on.process(x[:, 5000:])
    # the hop sums do not know of the switch
    for s in range(S):
        a, b = plain.read_hops(s), on.read_hops(s)
        assert len(a) == n // 800 and np.array_equal(bits(a), bits(b)), s
    assert plain.finish() == on.finish()
    first = device_peaks(amd, x[:, :0], [], obj=on)
    check(first, x, RATE, "before the reset")
    # reset clears the peak state: a quieter programme reads its own peaks, from a zero history
    on.reset()
    zero = device_peaks(amd, x[:, :0], [], obj=on)
    assert not zero[0].any() and not zero[1].any()
    y = 0.25 * x[:, 100:5000]
    check(device_peaks(amd, y, [3000, 1900], obj=on), y, RATE, "after the reset")
    # after a reset the switch may go off and on again; on again starts from cleared peaks
    plain.reset()
    plain.set_true_peak(True)
    check(device_peaks(amd, y, obj=plain), y, RATE, "switched on after a reset")
    plain.reset()
    plain.set_true_peak(False)
    assert lib.cpq_loudness_read_peaks(plain._h, res) == K.CPQ_ERR_NOT_READY
    plain.set_true_peak(True)
    assert not device_peaks(amd, x[:, :0], [], obj=plain)[0].any()
    plain.close()
    on.close()


def strided(torch, x, stride, fill=7.0):
    flat = torch.full((x.shape[0] * stride + 8,), fill, dtype=torch.float64, device="cuda")
    rows = flat[2:2 + x.shape[0] * stride].view(x.shape[0], stride)
    rows[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return flat, rows[:, :x.shape[1]]


def apply_case(amd, S, n, extra_in, extra_out):
    import torch
    rng = np.random.default_rng(n + S)
    x = rng.standard_normal((2 * S, n))
    x[0, n // 2] = np.nan                           # nothing is scrubbed: a NaN stays a NaN
    x[-1, 0] = np.inf
    gains = rng.uniform(0.05, 3.0, S)
    want = x * np.repeat(gains, 2)[:, None]
    obj = amd.ProgrammeLoudness(S, RATE, 1)
    flat_in, t_in = strided(torch, x, n + extra_in)
    flat_out, t_out = strided(torch, np.zeros_like(x), n + extra_out, fill=9.0)
    keep_in = flat_in.clone()
    obj.apply_device(gains, t_in, t_out)
    torch.cuda.synchronize()
    got = t_out.cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    assert torch.equal(flat_in.view(torch.int64), keep_in.view(torch.int64))
    gaps = torch.ones_like(flat_out, dtype=torch.bool)
    gaps[2:2 + 2 * S * (n + extra_out)].view(2 * S, n + extra_out)[:, :n] = False
    assert bool((flat_out[gaps] == 9.0).all())      # what lies between the rows is as it was
    if extra_in == extra_out:                       # in place
        obj.apply_device(gains, t_in)
        torch.cuda.synchronize()
        assert np.array_equal(bits(t_in.cpu().numpy()), bits(want))
        gaps_in = torch.ones_like(flat_in, dtype=torch.bool)
        gaps_in[2:2 + 2 * S * (n + extra_in)].view(2 * S, n + extra_in)[:, :n] = False
        assert bool((flat_in[gaps_in] == 7.0).all())
    assert obj.finish()[0]["n_hops"] == 0           # the programme is not touched
    obj.close()


@pytest.mark.parametrize("S", (1, 3, 65))
@pytest.mark.parametrize("n,extra_in,extra_out", ((1, 1, 1), (2, 0, 0), (1001, 0, 0), (1001, 1, 1), (1001, 1, 3), (1000, 0, 2), (1000, 1, 2),
                                                  (4097, 3, 3)))
def test_apply_against_numpy_bit_for_bit(amd, S, n, extra_in, extra_out):
    apply_case(amd, S, n, extra_in, extra_out)


@pytest.mark.parametrize("n", (524288 + 6, 524288 + 7))
def test_apply_where_the_lanes_stride_over_a_row(amd, n):
    """more than kApplyMaxBlocks blocks' worth of samples in a row (1024 blocks of 256 lanes, two samples a lane)"""
    apply_case(amd, 1, n, 0, 0)
    apply_case(amd, 1, n, 1, 1)


def test_apply_refusals_move_nothing(amd):
    import torch
    lib, K = amd._capi.load(), amd._capi
    S, n = 2, 100
    obj = amd.ProgrammeLoudness(S, RATE, 1)
    t = torch.ones((2 * S, n), dtype=torch.float64, device="cuda")
    out = torch.zeros_like(t)
    g = np.ones(S)
    gp = g.ctypes.data_as(K.c_double_p)
    a, b = t.data_ptr(), out.data_ptr()
    call = lambda *args: lib.cpq_loudness_apply_device(obj._h, *args)
    assert call(gp, C.c_void_p(a), n, C.c_void_p(b), n, n) == K.CPQ_OK
    torch.cuda.synchronize()
    out.zero_()
    for args in ((None, a, n, b, n, n), (gp, None, n, b, n, n), (gp, a, n, None, n, n), (gp, a, n, b, n, 0), (gp, a, n, b, n, -1),
                 (gp, a, n - 1, b, n, n), (gp, a, n, b, n - 1, n), (gp, a + 8, n, b, n, n - 1), (gp, a, n, b + 8, n, n - 1),
                 (gp, a, n, a + 16, n, n - 2),      # out begins inside in's first row
                 (gp, a, n, a, n - 10, n - 10),     # the same pointer, another stride
                 (gp, a + 16 * n, n, a, n, n)):     # in two rows behind out
        assert call(args[0], C.c_void_p(args[1]), args[2], C.c_void_p(args[3]), *args[4:]) == K.CPQ_ERR_INVALID_ARG, args[1:]
        assert lib.cpq_loudness_last_error(obj._h)
    for bad in (np.nan, np.inf, -np.inf):
        g2 = np.array([1.0, bad])
        assert call(g2.ctypes.data_as(K.c_double_p), C.c_void_p(a), n, C.c_void_p(b), n, n) == K.CPQ_ERR_INVALID_ARG
        assert b"gain" in lib.cpq_loudness_last_error(obj._h)
    torch.cuda.synchronize()
    assert bool((t == 1.0).all()) and bool((out == 0.0).all())
    obj.close()


def test_normalise_on_a_device_tensor_end_to_end(amd):
    """three programmes to -23 LUFS under -1 dBTP: the loudness gain wins, the ceiling wins, silence stays"""
    import torch
    S, n = 3, 16000
    rng = np.random.default_rng(21)
    x = np.zeros((2 * S, n))
    x[0:2] = 0.1 * rng.standard_normal((2, n))
    x[2:4] = 0.004 * rng.standard_normal((2, n))
    x[3, 9000:9002] = -0.8
    t = torch.from_numpy(x).cuda()
    obj = amd.ProgrammeLoudness(S, RATE, 3, true_peak=True)
    obj.process_device(t)
    res, pks = obj.finish(), obj.peaks()
    gains, limited = obj.normalise_device(t, -23.0, -1.0)
    torch.cuda.synchronize()
    assert limited == [False, True, False] and gains[2] == 1.0 and res[2]["integrated"] == -math.inf
    assert gains[0] == 10.0 ** ((-23.0 - res[0]["integrated"]) / 20.0) and gains[0] == obj.gain(res[0], -23.0)
    ceiling = 10.0 ** (-1.0 / 20.0)
    assert gains[1] == ceiling / pks[1]["true_peak"][1] and pks[1]["true_peak"][1] == max(pks[1]["true_peak"] + pks[1]["sample_peak"])
    assert gains[1] < 10.0 ** ((-23.0 - res[1]["integrated"]) / 20.0)
    assert pks[1]["max_dbtp"] == 20.0 * math.log10(pks[1]["true_peak"][1]) and pks[2]["max_dbtp"] == -math.inf
    y = t.cpu().numpy()
    assert np.array_equal(bits(y), bits(x * np.repeat(gains, 2)[:, None]))
    # a second object on the written rows: the model's peaks on the same rows, bit for bit
    second = amd.ProgrammeLoudness(S, RATE, 3, true_peak=True)
    second.process_device(t)
    after, got = second.finish(), second.peaks()
    tp, sp = PK.peaks(y, RATE)
    for s in range(S):
        assert np.array_equal(bits(got[s]["true_peak"]), bits(tp[2 * s:2 * s + 2])), s
        assert np.array_equal(bits(got[s]["sample_peak"]), bits(sp[2 * s:2 * s + 2])), s
    # no peak passes the ceiling by more than the scaling bound
    bound = PK.scaling_bound(x, RATE, np.repeat(gains, 2))
    for r in range(2 * S):
        print(f"row {r}: true peak {tp[r]!r} ({float(PK.dbtp(tp[r])) if tp[r] else -math.inf:.4f} dBTP), over the ceiling {tp[r] - ceiling:.3e}, bound {bound[r]:.3e}")
        assert max(tp[r], sp[r]) <= ceiling + bound[r]
    assert abs(after[0]["integrated"] + 23.0) < 0.01 and after[1]["integrated"] < -23.0 and after[2]["integrated"] == -math.inf
    assert abs(float(PK.dbtp(tp[3])) + 1.0) < 1e-9
    obj.close()
    second.close()
