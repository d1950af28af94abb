"""GPU tests of cpq_loudness (gated programme loudness, EBU R 128; kernels in convopeq_amd/csrc/prog_kernels.hip) through the C
ABI, against tests/prog_model.py on the programmes of tests/prog_inputs.py.

Hop sums.  read_hops against the fp64 sequential model within max(8 d_ref, 4 H 2^-52 E) per hop: d_ref is the distance of that
model from its np.longdouble run on the same input (the loudness bar of test_gpu_metering.py), the second term what adding H
positive terms in another order may cost.  Where a call's 2048-sample spans fall decides how the K-weighting scan associates, so
another split of the same programme is held to the bar, not to equal bits; the same split twice gives equal bits.

Finish.  The device's figures against the numpy finish run on the device's own hop sums: mean squares differ only in the order
n_blocks positive terms are added in, n_blocks 2^-52 relative, which is (10 / ln 10) n_blocks 2^-52 LU on a loudness; counts are
equal.  tests/test_prog_model_cpu.py asserts that no block of these inputs lies within 0.5 LU of a gate."""
import ctypes as C
import math

import numpy as np
import pytest

import prog_inputs as I
import prog_model as P

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52
FIGURES = ("integrated", "relative_gate", "momentary_max", "short_term_max")
COUNTS = ("n_hops", "n_blocks", "n_abs", "n_rel", "n_short_kept")


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def feed(obj, x, calls=None):
    o = 0
    for n in calls or [x.shape[1]]:
        obj.process(x[:, o:o + n])
        o += n
    assert o == x.shape[1]


def run(amd, x, calls=None, rate=I.RATE, seconds=70):
    obj = amd.ProgrammeLoudness(x.shape[0] // 2, rate, seconds)
    feed(obj, x, calls)
    hops = [obj.read_hops(s) for s in range(x.shape[0] // 2)]
    res = obj.finish()
    obj.close()
    return hops, res


def check_hops(got, ref, hop_len, label):
    assert got.shape == ref["E"].shape, label
    bar = I.hop_bar(ref, hop_len)
    diff = np.abs(got - ref["E"])
    worst = int(np.argmax(diff / np.maximum(bar, 1e-300))) if len(diff) else 0
    if len(diff):
        print(f"{label}: {len(got)} hops, worst hop {worst}: |dev - model| {diff[worst]:.3e}, bar {bar[worst]:.3e} (d_ref {ref['d_ref']:.3e})")
    assert np.all(diff <= bar), (label, worst)


def splits(n, piece):
    return [piece] * (n // piece) + ([n % piece] if n % piece else [])


def test_hop_sums_one_call_of_60_s(amd):
    ref = I.reference()["main60"]
    hops, _ = run(amd, ref["x"])
    check_hops(hops[0], ref, I.H, "60 s in one call")


@pytest.mark.parametrize("piece", (799, 800, 801, 2047, 2048, 2049, 4801))
def test_hop_sums_split_into_equal_calls(amd, piece):
    ref = I.reference()["main60"]
    hops, _ = run(amd, ref["x"], splits(ref["x"].shape[1], piece))
    check_hops(hops[0], ref, I.H, f"calls of {piece}")


def test_hop_sums_calls_of_one_sample_and_random_splits(amd):
    """calls of 1 sample over the first two hops and a bit (1700 calls), then random lengths; the same split twice: equal bits"""
    ref = I.reference()["main60"]
    n = ref["x"].shape[1]
    rng = np.random.default_rng(77)
    calls = [1] * 1700
    while sum(calls) < n:
        calls.append(int(min(n - sum(calls), rng.integers(1, 9000))))
    first, res1 = run(amd, ref["x"], calls)
    check_hops(first[0], ref, I.H, "1-sample calls, then random")
    again, res2 = run(amd, ref["x"], calls)
    assert np.array_equal(bits(first[0]), bits(again[0])) and res1 == res2


@pytest.mark.parametrize("rate", (44100, 48000))
def test_hop_sums_at_other_rates(amd, rate):
    ref = I.rate_reference(rate)
    hops, _ = run(amd, ref["x"], rate=rate, seconds=3)
    check_hops(hops[0], ref, rate // 10, f"{rate} Hz, one call")
    hops, _ = run(amd, ref["x"], splits(ref["x"].shape[1], 5000), rate=rate, seconds=3)
    check_hops(hops[0], ref, rate // 10, f"{rate} Hz, calls of 5000")


@pytest.mark.parametrize("rate", tuple(I.GRID_RATES))
def test_hop_sums_where_the_hop_grid_meets_the_span_grid(amd, rate):
    """10240 Hz: H = 1024, every second hop ends exactly on the end of a 2048-sample span (nothing is handed over to the next
    span); 20480 Hz: a hop is a span; 768000 Hz: H = 76800, a hop lies across 38 spans and is handed over 37 times"""
    ref = I.rate_reference(rate)
    n, seconds = ref["x"].shape[1], 3 if rate < 100000 else 1
    assert n == I.GRID_RATES[rate] and len(ref["E"]) == n // (rate // 10) >= 2
    hops, _ = run(amd, ref["x"], rate=rate, seconds=seconds)
    check_hops(hops[0], ref, rate // 10, f"{rate} Hz, one call")
    for piece in (1023, 1024, 1025, 2048) if rate < 100000 else (5000,):
        hops, _ = run(amd, ref["x"], splits(n, piece), rate=rate, seconds=seconds)
        check_hops(hops[0], ref, rate // 10, f"{rate} Hz, calls of {piece}")


def test_a_sample_whose_square_overflows(amd):
    """9.9e299 passes the scrub; its K-weighted square does not fit: that hop sum is +inf on the device as in the model, and so
    are those behind it while the filters ring down through 1e154.  Every finite hop meets the bar, taken per hop here (the ring
    spans 300 decades: max(8 d, 4 H 2^-52 E) with d that hop's own distance between the fp64 and the long-double model).  The
    finish on such hop sums is the host's, bit for bit: nothing passes the relative gate of an infinite mean"""
    ref = I.spiked_reference()
    hops, res = run(amd, ref["x"])
    got, want = hops[0], ref["E"]
    print("device", got.tolist())
    print("model ", want.tolist())
    assert got.shape == want.shape and np.isinf(want[1]) and want[1] > 0 and not np.isnan(got).any()
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.all(got[np.isinf(got)] > 0)
    fin = np.isfinite(want)
    assert fin[0] and fin[16:].all() and np.count_nonzero(fin) >= 35
    bar = I.hop_bar(dict(d_ref=ref["d"][fin], E=want[fin]), I.H)
    diff = np.abs(got[fin] - want[fin])
    print("diff / bar", (diff / bar).tolist())
    assert np.all(diff <= bar), np.flatnonzero(fin)[diff > bar]
    host = amd.loudness_finish_host(got, I.RATE)
    assert host == res[0], (host, res[0])
    assert res[0]["n_abs"] == 47 and res[0]["n_rel"] == 0 and res[0]["integrated"] == -math.inf and res[0]["relative_gate"] == math.inf
    assert res[0]["momentary_max"] == math.inf and res[0]["short_term_max"] == math.inf and res[0]["n_short_kept"] == 0


def check_finish(res, E, label):
    """the device's figures of one stream against the numpy finish on its own hop sums E"""
    want = P.finish(E, I.H)
    for key in COUNTS:
        assert res[key] == want[key], (label, key, res[key], want[key])
    tol = 10.0 / math.log(10.0) * max(want["n_blocks"], 1) * U52
    for key in FIGURES:
        print(f"{label} {key}: device {res[key]!r}, numpy {want[key]!r}, bar {tol:.3e}")
        if math.isinf(want[key]):
            assert res[key] == want[key], (label, key)
        else:
            assert abs(res[key] - want[key]) <= tol, (label, key)
    # the range's two picks: each within the bar, so the range within twice that
    print(f"{label} range: device {res['range']!r}, numpy {want['range']!r}")
    assert abs(res["range"] - want["range"]) <= 2.0 * tol, label
    return want


@pytest.mark.parametrize("name", ("ebu_3341_1", "ebu_3341_3", "ebu_3342_1", "short_399ms", "silence", "tone_minus80", "hops_4",
                                  "hops_30", "ramp40", "scrub", "main60"))
def test_finish_against_numpy_on_the_device_hop_sums(amd, name):
    ref = I.reference()[name]
    hops, res = run(amd, ref["x"])
    check_hops(hops[0], ref, I.H, name)
    want = check_finish(res[0], hops[0], name)
    if name == "short_399ms":
        assert res[0]["n_hops"] == 3 and res[0]["n_blocks"] == 0 and res[0]["integrated"] == -math.inf and res[0]["range"] == 0.0
    if name in ("silence", "tone_minus80"):
        assert res[0]["n_blocks"] == 47 and res[0]["n_abs"] == 0 and res[0]["integrated"] == -math.inf
        with pytest.raises(amd.CpqError) as e:
            _gain(amd, res[0])
        assert e.value.status == amd._capi.CPQ_ERR_NOT_READY
    if name == "silence":
        assert not hops[0].any()
    if name == "hops_4":
        assert res[0]["n_blocks"] == 1 and res[0]["n_short_kept"] == 0
    if name == "hops_30":
        assert res[0]["n_blocks"] == 27 and res[0]["n_short_kept"] == 1 and res[0]["range"] == 0.0
    if name == "ramp40":
        assert res[0]["n_short_kept"] == 40 and res[0]["range"] > 7.0
    if name == "ebu_3342_1":
        assert abs(res[0]["range"] - 10.0) <= 1.0
    if name == "ebu_3341_1":
        assert abs(_gain(amd, res[0]) - 10.0 ** ((-23.0 - res[0]["integrated"]) / 20.0)) <= 1e-15
    # the host finish of the library is the device's, operation for operation
    host = amd.loudness_finish_host(hops[0], I.RATE)
    assert host == res[0], (host, res[0])
    assert want["n_hops"] == len(hops[0])


def _gain(amd, result, target=-23.0):
    obj = amd.ProgrammeLoudness(1, I.RATE, 1)
    try:
        return obj.gain(result, target)
    finally:
        obj.close()


@pytest.fixture(scope="module")
def alone(amd):
    """hop sums and figures of each of 300 programmes run alone, through one object that is reset in between"""
    obj = amd.ProgrammeLoudness(1, I.RATE, 4)
    out = []
    for s in range(300):
        obj.reset()
        obj.process(I.stream_programme(s))
        out.append((obj.read_hops(0), obj.finish()[0]))
    obj.close()
    return out


@pytest.mark.parametrize("S", (1, 3, 64, 300))
def test_every_stream_as_if_alone(amd, alone, S):
    x = np.concatenate([I.stream_programme(s) for s in range(S)])
    hops, res = run(amd, x, seconds=4)
    for s in range(S):
        assert np.array_equal(bits(hops[s]), bits(alone[s][0])), s
        assert res[s] == alone[s][1], s
    assert len({r["integrated"] for r in res}) == S     # the programmes differ
    # ... and in two calls that cut hops and spans
    hops2, _ = run(amd, x, [2049, x.shape[1] - 2049], seconds=4)
    one = amd.ProgrammeLoudness(1, I.RATE, 4)
    feed(one, x[2 * (S - 1):2 * S], [2049, x.shape[1] - 2049])
    assert np.array_equal(bits(hops2[S - 1]), bits(one.read_hops(0)))
    one.close()


def test_row_stride_sentinels_and_a_stream_of_its_own(amd):
    """device rows with a stride above n_samples and NaN sentinels around every row, on a non-default stream"""
    import torch
    S, n, stride = 3, 28000, 28000 + 24
    x = np.concatenate([I.stream_programme(s) for s in range(S)])
    flat = torch.full((2 * S * stride + 16,), float("nan"), dtype=torch.float64, device="cuda")
    rows = flat[8:8 + 2 * S * stride].view(2 * S, stride)       # 64-byte offset: still 16-byte aligned
    rows[:, :n] = torch.from_numpy(x).cuda()
    before = flat.clone()
    stream = torch.cuda.Stream()
    obj = amd.ProgrammeLoudness(S, I.RATE, 4)
    obj.set_stream(stream)
    torch.cuda.synchronize()
    obj.process_device(rows[:, :n])
    res = obj.finish()
    hops = [obj.read_hops(s) for s in range(S)]
    obj.set_stream(None)
    obj.close()
    assert torch.equal(flat.view(torch.int64), before.view(torch.int64))        # the rows are read, never written
    want_h, want_r = run(amd, x, seconds=4)
    for s in range(S):
        assert np.array_equal(bits(hops[s]), bits(want_h[s])) and res[s] == want_r[s]
        assert np.isfinite(res[s]["integrated"])


def test_100_calls_back_to_back_then_finish(amd):
    import torch
    S, piece = 4, 280
    x = np.concatenate([I.stream_programme(s) for s in range(S)])
    t = torch.from_numpy(x).cuda()
    obj = amd.ProgrammeLoudness(S, I.RATE, 4)
    for i in range(100):
        obj.process_device(t[:, i * piece:(i + 1) * piece])     # odd offsets are 16-byte aligned: 280 doubles apart
    res = obj.finish()
    hops = [obj.read_hops(s) for s in range(S)]
    obj.close()
    want_h, want_r = run(amd, x[:, :100 * piece], [piece] * 100, seconds=4)
    for s in range(S):
        assert len(hops[s]) == 35 and np.array_equal(bits(hops[s]), bits(want_h[s])) and res[s] == want_r[s]


def test_host_rows_whose_calls_grow(amd):
    """process() on host rows in calls of 1, 4801 (a hop and a sample) and 9600 samples (two hops): the object's row buffer is
    replaced before the second and before the third call, its stride changing each time.  Bit for bit the hops of a second
    object given the same rows call by call through process_device, where nothing is staged.  (The calls are the same on both:
    another split of a programme is held to the bar above, not to equal bits.)"""
    import torch
    S, rate, calls = 2, 48000, [1, 4801, 9600]              # hops of 4800 samples
    t = np.arange(sum(calls))
    x = 0.1 * np.sin(2.0 * math.pi * 997.0 * t / rate + np.arange(2 * S)[:, None]) + 0.01 * np.random.default_rng(5).standard_normal((2 * S, len(t)))
    staged, direct = amd.ProgrammeLoudness(S, rate, 4), amd.ProgrammeLoudness(S, rate, 4)
    feed(staged, x, calls)
    o, pieces = 0, []
    for n in calls:
        pieces.append(torch.from_numpy(np.ascontiguousarray(x[:, o:o + n])).cuda())        # its own tensor: 16-byte aligned
        direct.process_device(pieces[-1])
        o += n
    for s in range(S):
        got, want = staged.read_hops(s), direct.read_hops(s)
        assert len(want) == 3 and np.all(want > 0.0)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), s
    assert staged.finish() == direct.finish()
    staged.close()
    direct.close()


def test_finish_in_mid_programme_reset_and_max_hops(amd):
    ref = I.reference()["ebu_3342_1"]
    x = ref["x"]
    n = x.shape[1]
    obj = amd.ProgrammeLoudness(1, I.RATE, n / I.RATE)          # max_hops is exactly the programme
    obj.process(x[:, :70001])
    mid = obj.finish()[0]
    assert mid["n_hops"] == 87 and mid == obj.finish()[0]
    check_finish(mid, obj.read_hops(0), "mid-programme")
    obj.process(x[:, 70001:n - 1])
    # a call that would pass max_hops is refused whole, and the state is as it was
    lib, K = amd._capi.load(), amd._capi
    two = np.ascontiguousarray(x[:, n - 2:])
    assert lib.cpq_loudness_process(obj._h, two.ctypes.data, 2, 2) == K.CPQ_ERR_UNSUPPORTED
    assert b"max_seconds" in lib.cpq_loudness_last_error(obj._h)
    obj.process(x[:, n - 1:])
    end, hops = obj.finish()[0], obj.read_hops(0)
    assert lib.cpq_loudness_process(obj._h, two.ctypes.data, 2, 1) == K.CPQ_ERR_UNSUPPORTED
    assert obj.finish()[0] == end
    want_h, want_r = run(amd, x, [70001, n - 70002, 1], seconds=n / I.RATE)
    assert np.array_equal(bits(hops), bits(want_h[0])) and end == want_r[0] and end["n_hops"] == 200
    check_hops(hops, ref, I.H, "finish in between")
    # reset: the object is as new
    obj.reset()
    assert obj.finish()[0]["n_hops"] == 0 and len(obj.read_hops(0)) == 0
    obj.process(x)
    fresh_h, fresh_r = run(amd, x, seconds=n / I.RATE)
    assert np.array_equal(bits(obj.read_hops(0)), bits(fresh_h[0])) and obj.finish()[0] == fresh_r[0]
    obj.close()


def test_call_refusals_move_nothing(amd):
    lib, K = amd._capi.load(), amd._capi
    x = I.stream_programme(0)
    obj = amd.ProgrammeLoudness(1, I.RATE, 4)
    obj.process(x[:, :1000])
    n = x.shape[1]
    for args, status in (((None, n, 10), K.CPQ_ERR_INVALID_ARG), ((x.ctypes.data, n, 0), K.CPQ_ERR_INVALID_ARG),
                         ((x.ctypes.data, n, -1), K.CPQ_ERR_INVALID_ARG), ((x.ctypes.data, 9, 10), K.CPQ_ERR_INVALID_ARG),
                         ((x.ctypes.data + 8, n, 10), K.CPQ_ERR_INVALID_ARG)):
        assert lib.cpq_loudness_process(obj._h, *args) == status, args
        assert lib.cpq_loudness_process_device(obj._h, *args) == status, args
        assert lib.cpq_loudness_last_error(obj._h)
    assert lib.cpq_loudness_process(None, x.ctypes.data, n, 10) == K.CPQ_ERR_INVALID_ARG
    n_hops = C.c_int64()
    assert lib.cpq_loudness_read_hops(obj._h, 1, None, 0, C.byref(n_hops)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_finish(obj._h, None) == K.CPQ_ERR_INVALID_ARG
    obj.process(x[:, 1000:])
    want_h, want_r = run(amd, x, [1000, n - 1000], seconds=4)
    assert np.array_equal(bits(obj.read_hops(0)), bits(want_h[0])) and obj.finish()[0] == want_r[0]
    obj.close()


def test_on_the_rows_an_engine_delivers(amd):
    """cpq_engine_process_block_device's output rows at 48 kHz, 4 streams, metered where they lie: the hop sums of the same rows
    downloaded and fed through cpq_loudness_process, bit for bit"""
    import torch
    S, B, T = 4, 512, 8
    rng = np.random.default_rng(9)
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=1024, max_blocks_per_call=T, sample_rate=48000.0)
    eng.prepare_to_play(48000.0, T * B)
    for s in range(S):
        ir = rng.standard_normal((2, 600)) * np.exp(-np.arange(600) / 80.0) * (0.2 + 0.1 * s)
        eng.set_impulse(s, ir[0], ir[1])
    eng.set_eq_params(amd.CPQ_ALL_STREAMS, amd.eq_params_default())
    dev, host = amd.ProgrammeLoudness(S, 48000, 2), amd.ProgrammeLoudness(S, 48000, 2)
    calls = 3
    x = 0.1 * rng.standard_normal((2 * S, calls * T * B))
    for k in range(calls):
        t_in = torch.from_numpy(np.ascontiguousarray(x[:, k * T * B:(k + 1) * T * B])).cuda()
        t_out = torch.empty_like(t_in)
        eng.process_device(t_in.data_ptr(), t_out.data_ptr(), T * B)
        torch.cuda.synchronize()                    # the engine has its own stream: its rows are written
        dev.process_device(t_out)
        torch.cuda.synchronize()
        host.process(t_out.cpu().numpy())
    for s in range(S):
        a, b = dev.read_hops(s), host.read_hops(s)
        assert len(a) == calls * T * B // 4800 and a.all() and np.array_equal(bits(a), bits(b)), s
    assert dev.finish() == host.finish()
    for o in (dev, host, eng):
        o.close()
