"""k_ir_resample through cpq_ir_resample / cpq_ir_resample_batch on the device.

The device and cpq_ir_resample_host read one table and add in one order, so every comparison with the host path is for equal
bits and equal lengths: any difference is a kernel bug.  Rows are undamped noise, so the tail trim keeps a row to its end (the
right-hand zero extension is compared too) unless the row has fewer than 8 outputs, where the reference's rule keeps one.
Shapes follow the kernel: T = 600 taps at 44100 -> 48000, tiles of 256 outputs (64 once M > 8 L), the row staged 256 taps at a time."""
import os

import numpy as np
import pytest

import convopeq_amd as amd
import resample_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 256


def noise(shape, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, size=shape)


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def host(ir, a, b):
    return amd.ir_resample(ir, a, b, host=True)


def rows_for_outputs(count, a, b):
    """the shortest row with `count` outputs"""
    n = (count - 1) * a // b
    while M.out_len(n, a, b) < count:
        n += 1
    assert M.out_len(n, a, b) == count
    return n


def test_row_lengths_around_the_filter_length():
    a, b = 44100, 48000
    T = amd.resample_design(a, b)["T"]
    assert T == 600
    for n in (1, 2, T // 2, T - 1, T, T + 1):
        ir = noise((1, n), n)
        got, want = amd.ir_resample(ir, a, b), host(ir, a, b)
        assert same(got, want), n
        assert n <= 2 or want.shape[1] >= M.out_len(n, a, b) - 8          # undamped: kept to the end, both zero extensions compared


def test_output_counts_around_the_tile():
    a, b = 44100, 48000
    lengths = [rows_for_outputs(c, a, b) for c in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)]
    irs = [(noise((1, n), 100 + n), a) for n in lengths]
    got = amd.ir_resample_batch(irs, b)
    for (ir, _), g, count in zip(irs, got, (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)):
        want = host(ir, a, b)
        assert same(g, want) and count - 8 <= want.shape[1] <= count
        assert same(amd.ir_resample(ir, a, b), want)


@pytest.mark.parametrize("pair", [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000), (88200, 48000), (96000, 44100),
                                  (96000, 8000), (8000, 96000), (768000, 8000)],
                         ids=["160:147", "147:160", "2:1", "1:2", "80:147", "147:320", "1:12 (tile 64)", "12:1", "1:96 (tile 64)"])
def test_ratios(pair):
    a, b = pair
    d = amd.resample_design(a, b)
    n = 2 * d["T"] + 37 if d["T"] < 4000 else 2500           # longer than the filter, or (the 64-output tiles) shorter
    ir = noise((2, n), a % 1000 + b % 999)
    want = host(ir, a, b)
    assert same(amd.ir_resample(ir, a, b), want)
    nOut = M.out_len(n, a, b)
    assert nOut >= 16 and want.shape[1] >= nOut - 8
    # the first and the last T outputs against the longdouble model: the zero extension on either side is the definition's
    idx = np.unique(np.concatenate([np.arange(min(d["T"], want.shape[1])), np.arange(max(0, want.shape[1] - d["T"]), want.shape[1])]))
    model, bound = M.resample_rows(d, ir[0], outputs=idx)
    u = 2.0 ** -53
    limit = (d["T"] * u / (1 - d["T"] * u) + d["T"] * 2.0 ** -63) * bound
    assert np.all(np.abs(want[0, idx].astype(np.longdouble) - model) <= limit)


def test_mono_and_stereo_in_one_batch():
    a, b = 48000, 44100
    mono, stereo = noise((1, 900), 1), noise((2, 1400), 2)
    got = amd.ir_resample_batch([(mono, a), (stereo, a)], b)
    assert same(got[0], host(mono, a, b)) and same(got[1], host(stereo, a, b))


def test_batch_of_five_lengths_and_two_source_rates():
    b = 48000
    irs = [(noise((2, 700), 11), 44100), (noise((1, 1301), 12), 96000), (noise((2, 64), 13), 44100), (noise((1, 2049), 14), 96000),
           (noise((2, 333), 15), 44100), (noise((1, 500), 16), 48000)]         # the last one is at the target rate: a copy
    got = amd.ir_resample_batch(irs, b)
    assert len(got) == len(irs)
    for (ir, rate), g in zip(irs, got):
        assert same(g, amd.ir_resample(ir, rate, b)) and same(g, host(ir, rate, b))
    assert same(got[5], irs[5][0])
    # a stereo IR whose channels end at different places: each cut at its own length, zero beyond
    ir = noise((2, 3000), 17)
    ir[1, 500:] = 0.0
    g = amd.ir_resample(ir, 44100, b)
    assert same(g, host(ir, 44100, b)) and not np.any(g[1, 1300:]) and np.any(g[0, 1300:])


def test_batch_is_all_or_nothing():
    good, silent = noise((1, 500), 21), np.zeros((1, 500))
    with pytest.raises(amd.CpqError) as e:
        amd.ir_resample_batch([(good, 44100), (silent, 44100)], 48000)
    assert e.value.status == amd._capi.CPQ_ERR_SILENT_IR and "IR 1" in str(e.value)
    with pytest.raises(amd.CpqError) as e:
        amd.ir_resample(good, 44100, 48000, phase=amd._capi.CPQ_RESAMPLE_MINIMUM_PHASE)
    assert e.value.status == amd._capi.CPQ_ERR_UNSUPPORTED
    assert amd.ir_resample_batch([], 48000) == []


def test_long_row():
    a, b = 44100, 48000
    ir = noise((1, 131072), 31)
    got, want = amd.ir_resample(ir, a, b), host(ir, a, b)
    assert want.shape[1] >= M.out_len(131072, a, b) - 8
    spread = np.linspace(0, want.shape[1] - 1, 4096).astype(np.int64)
    assert got.shape == want.shape and np.array_equal(got[0, spread].view(np.uint64), want[0, spread].view(np.uint64))
    assert same(got, want)
    assert amd._capi.load().cpq_ir_resample_last_kernel_ms() > 0.0


def test_fixture_pairs_on_the_device():
    golden = np.load(M.GOLDEN)
    for a, b in M.PAIRS:
        key = M.pair_key(a, b)
        x, d_ref = golden["x_" + key], float(golden["d_ref_" + key])
        got = amd.ir_resample(x, a, b)
        want = M.passband_signal(M.out_len(len(x), a, b), b)
        err = float(np.max(np.abs(got[0] - want[:got.shape[1]])))
        print(f"{key}: device {err:.3e}, 2 d_ref {2 * d_ref:.3e}")
        assert err <= max(2.0 * d_ref, 64 * 2.0 ** -52 * np.max(np.abs(want)))
        assert same(got, host(x, a, b))
    got = amd.ir_resample(golden["x_stop"], *M.STOP_PAIR)
    assert float(np.max(np.abs(got))) <= 2.0 * float(golden["leak_stop"])
    got = amd.ir_resample(golden["x_impulse"], *M.IMPULSE_PAIR)
    assert int(np.argmax(np.abs(got[0]))) == 109


def test_end_to_end_resampled_ir_on_a_stream(oracle):
    O = oracle
    B = 512
    ir, rate = amd.ir_load_wav(os.path.join(HERE, "golden", "impulse_room_correction_hpf_lpf.wav"))
    assert rate == 48000.0
    head = np.stack([ir[0, :4096], ir[-1, :4096]])
    with pytest.raises(amd.CpqError) as e:
        amd.ir_prepare(head, 48000.0, 44100.0, 0.5)
    assert e.value.status == amd._capi.CPQ_ERR_UNSUPPORTED
    res = amd.ir_resample(head, 48000.0, 44100.0)
    assert same(res, host(head, 48000.0, 44100.0))
    prep = amd.ir_prepare(res, 44100.0, 44100.0, 0.5)
    irs, scale = prep["ir"], prep["scale"]["scale_factor"]
    x = np.stack([O.gen_pcm(4 * B, stream=0, channel=ch) for ch in range(2)])
    ref = np.empty_like(x)
    for ch in range(2):
        nuc = O.Nuc()
        assert nuc.set_impulse(irs[ch] * scale, B)
        ref[ch] = nuc.run(x[ch], B)
        nuc.close()
    eng = amd.BatchedEngine(1, block_size=B, max_ir_len=irs.shape[1], max_blocks_per_call=1)
    eng.prepare_to_play(44100.0, B)
    eng.set_impulse(0, irs[0] * scale, irs[1] * scale)
    y = np.concatenate([eng.conv_process(x[:, i * B:(i + 1) * B]) for i in range(4)], axis=1)
    eng.close()
    err = float(np.sqrt(np.mean(np.square(y - ref))))
    print("resampled IR on a stream: rms err", err, "signal rms", float(np.sqrt(np.mean(np.square(ref)))))
    assert np.any(ref) and err <= 1e-13
