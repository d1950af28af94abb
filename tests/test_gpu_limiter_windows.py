"""k_lim_apply and k_lim_keep at every window where one of their rules changes, and on rows of more than 256 tiles.

As in test_gpu_limiter.py the reference is the host object (host=True) fed the same calls, the comparison is for equal shape,
equal bits and equal telemetry without a tolerance, and every device buffer keeps its sentinel columns.  The windows, the calls
and the signals are tests/limiter_window_cases.py's; test_limiter_window_cases_cpu.py shows without a GPU that every class of
windows has its property and that every signal limits.

What the window decides in the kernels (M = W + 12, D = W + 11, halo = 2 W + 21, nR = 1024 + 2 W + 10):
  the sliding minimum   doubling steps 1, 2, 4, ... and one remainder step of M - 2^k, swinging between two LDS stages.  No
                        remainder step (M = 2^k), a remainder of 1 (2^k + 1), the largest (2^k - 1); an even step count leaves
                        the result on the stage it started on, an odd one on the other (the three windows of test_gpu_limiter.py
                        are all odd)
  the r rounds          nR in rounds of 256: no idle lane in the last round (nR % 256 == 0), all but two idle (2), two idle (254)
  the keep step         up to halo samples in ascending chunks of 256: halo = 255, 257, 511, 513, 1023, 1025, and a history that
                        grows from 5 to halo - 1 samples in one call shorter than the halo
  the flush             D = 1023, 1024 and 1025 outputs: at 1025 a second tile of one output
  the fold              one trip of 256 lanes over the tile partials up to 256 tiles, a second above; part's stream stride is the
                        largest tile count seen, not the call's"""
import numpy as np
import pytest

import limiter_model as LM
import limiter_window_cases as LC
from test_gpu_limiter import check, device_pieces, pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W", LC.SWEEP_WINDOWS)
def test_window_sweep(W):
    """stride_pad 3: every call but the one of 2 samples has even strides and takes the 16-byte path; the flush is scalar"""
    classes = [name for name, (windows, has) in LC.CLASSES.items() if W in windows]
    assert classes and all(LC.CLASSES[name][1](W) for name in classes)
    lengths = LC.sweep_lengths(W)
    dev, host = pair(LC.SWEEP_STREAMS, W)
    assert dev.latency == LC.lim_d(W)
    tel = check(dev, host, LC.sweep_signal(W), lengths, stride_pad=3)
    assert all(t["limited_samples"] > 0 and t["min_gain"] < 1.0 for t in tel)


def test_both_parities_of_the_step_count_are_in_the_sweep():
    parity = {W: len(LC.min_steps(W)) % 2 for W in LC.SWEEP_WINDOWS}
    assert {W for W, odd in parity.items() if odd} == {8, 19, 20, 53, 115, 116, 245, 246, 251, 499, 500, 1013, 1014, 1024}
    assert sum(parity.values()) == 14 and len(parity) == 26        # 12 windows end on the stage the minimum started on


@pytest.mark.parametrize("n_streams", (1, 3))
def test_more_than_256_tiles_and_partials_that_grow(n_streams):
    """Calls of 3 samples (partials for 1 tile), 256 tiles (one whole trip of the fold), 257 tiles and one sample (the partials
    grow, a second trip, a last tile of one output) and 1500 samples (2 tiles at a stream stride of 258).  The smallest gain of
    the programme lies in tile 256 of the third call, which only the second trip reads."""
    x = LC.fold_signal(n_streams)
    want = LC.host_telemetry(n_streams, LC.FOLD_W, x, LC.FOLD_LENGTHS)
    less = LC.host_telemetry(n_streams, LC.FOLD_W, LC.fold_signal(n_streams, deepest=False), LC.FOLD_LENGTHS)
    assert all(b["min_gain"] > a["min_gain"] and b["limited_samples"] < a["limited_samples"] for a, b in zip(want, less))
    dev, host = pair(n_streams, LC.FOLD_W)
    tel = check(dev, host, x, LC.FOLD_LENGTHS, stride_pad=2 if n_streams == 1 else 3)
    assert tel == want and all(t["limited_samples"] > 0 for t in tel)


@pytest.mark.parametrize("W", LC.MODEL_WINDOWS)
def test_against_the_numpy_model(W):
    """one call of a tile and 300 samples and the flush, held to tests/limiter_model.py as well as to the host object"""
    n = LC.TILE + 300
    x = LC.noise(2, n, 40 + W)
    x[2:] *= 2.0
    for at in (0, LC.TILE - 1, LC.TILE, n - 1):
        LC.plant(x, at)
    LC.plant_in(x, 0, 100, 3.0)
    LC.plant_in(x, 0, 100 + LC.lim_m(W) - 1, 2.2)
    dev, host = pair(2, W)
    got = np.concatenate(device_pieces(dev, x, [n], stride_pad=2), axis=1)
    tel = dev.telemetry()
    for s in range(2):
        want = LM.limit(x[2 * s:2 * s + 2], LC.RATE, dev.ceiling, W, LC.gains(2)[s])
        assert LC.same(got[2 * s:2 * s + 2], want.y), f"stream {s}: {int((got[2 * s:2 * s + 2].view(np.uint64) != want.y.view(np.uint64)).sum())} doubles differ"
        assert tel[s] == {"min_gain": want.min_gain, "limited_samples": want.limited_samples}
        assert want.limited_samples > 0 and want.min_gain < 1.0
    check(dev, host, x, [n], stride_pad=2)              # the flush has started a new programme


@pytest.mark.parametrize("W", LC.IN_PLACE_WINDOWS)
@pytest.mark.parametrize("stride_pad,in_place", ((4, True), (3, True), (4, False)),
                         ids=("in place, scalar stores", "in place, 16-byte stores", "apart, scalar loads and stores"))
def test_in_place_and_odd_strides(W, stride_pad, in_place):
    """The sweep's calls.  All but one of their lengths are odd, so stride_pad 4 makes the caller's strides odd (the scalar path)
    and stride_pad 3 even.  In place the rows go through the object's stage, whose stride is even and which is replaced by a
    larger one before the calls of halo - 6, TILE + 1 and 2 TILE + 3 samples."""
    lengths = LC.sweep_lengths(W)
    assert LC.wide(lengths, stride_pad) == [stride_pad == 3] * 4 + [stride_pad != 3] + [stride_pad == 3]
    dev, host = pair(LC.SWEEP_STREAMS, W)
    tel = check(dev, host, LC.sweep_signal(W), lengths, stride_pad=stride_pad, in_place=in_place)
    assert all(t["limited_samples"] > 0 and t["min_gain"] < 1.0 for t in tel)
