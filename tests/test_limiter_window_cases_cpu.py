"""The cases of tests/test_gpu_limiter_windows.py without a GPU: tests/limiter_window_cases.py restates csrc/lim_plan.hpp with the
constants the headers have, every class of windows is non-empty and has the property it stands for, both parities of the
minimum's step count occur, and every signal limits on the host object alone, so that no device case can pass on rows the
limiter never touches."""
import os
import re

import numpy as np
import pytest

import convopeq_amd as amd
import limiter_model as LM
import limiter_window_cases as LC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "convopeq_amd", "csrc")


def header_constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"\b%s = (\d+)\b" % name, f.read())
    assert m, (header, name)
    return int(m.group(1))


def test_the_restated_constants_are_the_headers():
    assert LC.TILE == header_constant("lim_plan.hpp", "kLimTile")
    assert LC.ROUND == header_constant("lim_plan.hpp", "kLimThreads")
    assert LC.KEEP_CHUNK == header_constant("lim_plan.hpp", "kLimKeepBlock")
    assert LC.MIN_WINDOW == header_constant("lim_plan.hpp", "kLimMinWindow")
    assert LC.MAX_WINDOW == header_constant("lim_plan.hpp", "kLimMaxWindow")
    assert LC.PEAK_TAPS == header_constant("prog_plan.hpp", "kPeakTaps")
    for W in LC.SWEEP_WINDOWS:
        lim = amd.TruePeakLimiter(1, LC.RATE, LC.CEIL_DB, W, host=True)
        assert lim.window == W and lim.latency == LC.lim_d(W)
    assert (LC.lim_m(72), LC.lim_d(72), LC.lim_halo(1024), LC.lim_r_count(8)) == (84, 83, 2069, 1050)       # lim_plan_check.cpp's


def test_every_class_of_windows_is_non_empty_and_has_its_property():
    for name, (windows, has) in LC.CLASSES.items():
        assert windows, name
        for W in windows:
            assert LC.MIN_WINDOW <= W <= LC.MAX_WINDOW and has(W), (name, W)
    # the classes that are complete lists: no other window in range has the property
    every = range(LC.MIN_WINDOW, LC.MAX_WINDOW + 1)
    assert tuple(W for W in every if LC.is_pow2(LC.lim_m(W))) == LC.CLASSES["M a power of two: no remainder step"][0]
    assert [W for W in every if LC.lim_r_count(W) % LC.ROUND == 0][:2] == [123, 251]
    assert [W for W in every if LC.lim_halo(W) % LC.KEEP_CHUNK in (1, LC.KEEP_CHUNK - 1) and LC.lim_halo(W) <= 4 * LC.KEEP_CHUNK + 1] == [117, 118, 245, 246, 373, 374, 501, 502]
    assert len(LC.SWEEP_WINDOWS) == 26
    # what the three windows of test_gpu_limiter.py leave out: their remainder steps are 4, 20 and 12, never 0, 1 or the largest
    assert [LC.remainder_step(W) for W in LC.OLD_WINDOWS] == [4, 20, 12]
    assert all(LC.lim_r_count(W) % LC.ROUND not in (0, 2, LC.ROUND - 2) for W in LC.OLD_WINDOWS)
    assert all(abs(LC.lim_halo(W) - k * LC.KEEP_CHUNK) > 1 for W in LC.OLD_WINDOWS for k in (1, 2, 4))
    assert set(LC.MODEL_WINDOWS) <= set(LC.SWEEP_WINDOWS) and set(LC.IN_PLACE_WINDOWS) <= set(LC.SWEEP_WINDOWS)


def test_the_minimum_ends_on_either_stage_over_the_sweep():
    """The minimum starts on stage B and every step swaps the stages: an even step count leaves the result on B, an odd one on A.
    M = 2^k takes k steps, any other M below 2^(k+1) takes k + 1.  The three windows of test_gpu_limiter.py all take an odd count
    (5, 7, 11), so a kernel that read stage A whatever the count would pass there; the even count is this sweep's."""
    for W in LC.SWEEP_WINDOWS + LC.OLD_WINDOWS:
        steps, M = LC.min_steps(W), LC.lim_m(W)
        assert sum(steps) == M - 1 and all(1 <= s <= 1 + sum(steps[:i]) for i, s in enumerate(steps))
        assert len(steps) == (M - 1).bit_length()
    odd = tuple(W for W in LC.SWEEP_WINDOWS if len(LC.min_steps(W)) % 2)
    even = tuple(W for W in LC.SWEEP_WINDOWS if len(LC.min_steps(W)) % 2 == 0)
    assert odd == (8, 19, 20, 53, 115, 116, 245, 246, 251, 499, 500, 1013, 1014, 1024)
    assert even == (21, 52, 117, 118, 122, 123, 124, 244, 501, 502, 1011, 1012)
    assert [len(LC.min_steps(W)) for W in LC.OLD_WINDOWS] == [5, 7, 11]


def test_the_sweep_calls_grow_the_history_across_every_keep_chunk():
    for W in LC.SWEEP_WINDOWS:
        lengths, halo = LC.sweep_lengths(W), LC.lim_halo(W)
        assert all(k >= 1 for k in lengths) and lengths[1] < halo
        assert lengths[0] < LC.KEEP_CHUNK and lengths[0] + lengths[1] == halo - 1 and sum(lengths[:3]) == halo
        # stride_pad 3 puts every call but the one of 2 samples on the 16-byte path, stride_pad 4 on the scalar path
        assert LC.wide(lengths, 3) == [True, True, True, True, False, True]
        assert LC.wide(lengths, 4) == [False, False, False, False, True, False]
        n, start = sum(lengths), sum(lengths[:-1])
        for stream, first in ((0, LC.lim_m(W) - 1), (1, W - 1)):
            chain = [at for s, at, _ in LC.sweep_peaks(W) if s == stream]
            assert np.diff(chain).tolist() == [first, first + 1]
            assert start <= chain[2] < n - 1 and chain[1] >= start - 2


@pytest.mark.parametrize("W", LC.SWEEP_WINDOWS)
def test_every_sweep_signal_limits_on_the_host_object(W):
    tel = LC.host_telemetry(LC.SWEEP_STREAMS, W, LC.sweep_signal(W), LC.sweep_lengths(W))
    assert all(t["limited_samples"] > 0 and t["min_gain"] < 1.0 for t in tel)
    # the quiet stream is limited by the planted peaks only: take them out and it passes untouched
    x = LC.sweep_signal(W)
    for stream, at, _ in LC.sweep_peaks(W):
        x[:2, at] = 0.0
    assert LC.host_telemetry(LC.SWEEP_STREAMS, W, x, LC.sweep_lengths(W))[0] == {"min_gain": 1.0, "limited_samples": 0}


@pytest.fixture(scope="module")
def fold_envelope():
    """stream 0 of the one-stream case through the numpy model, which has the envelope itself"""
    x = LC.fold_signal(1)
    lim = amd.TruePeakLimiter(1, LC.RATE, LC.CEIL_DB, LC.FOLD_W, host=True)
    return LM.limit(x[:2], LC.RATE, lim.ceiling, LC.FOLD_W, LC.gains(1)[0])


def test_the_fold_case_limits_in_the_tiles_it_names(fold_envelope):
    a, starts = fold_envelope.a, LC.fold_call_starts()
    assert LC.FOLD_LENGTHS[1] == LC.KEEP_CHUNK * LC.TILE and LC.FOLD_LENGTHS[2] == (LC.KEEP_CHUNK + 1) * LC.TILE + 1

    def tile(call, t):
        lo = starts[call] + t * LC.TILE
        return a[lo:min(lo + LC.TILE, starts[call + 1])]

    for at, amp, call, t in LC.fold_peaks():
        assert starts[call] <= at < starts[call + 1] and (at - starts[call]) // LC.TILE == t
        assert (tile(call, t) < 1.0).sum() > 0, (call, t)
    last = tile(2, LC.KEEP_CHUNK + 1)
    assert last.shape == (1,) and last[0] < 1.0                 # the one-output tile of the second trip
    assert int(np.argmin(a)) - starts[2] in range(LC.KEEP_CHUNK * LC.TILE, (LC.KEEP_CHUNK + 1) * LC.TILE)
    assert tile(2, LC.KEEP_CHUNK).min() < min(a[:starts[2] + LC.KEEP_CHUNK * LC.TILE].min(), a[starts[2] + (LC.KEEP_CHUNK + 1) * LC.TILE:].min())


@pytest.mark.parametrize("n_streams", (1, 3))
def test_the_fold_case_on_the_host_object(n_streams, fold_envelope):
    tel = LC.host_telemetry(n_streams, LC.FOLD_W, LC.fold_signal(n_streams), LC.FOLD_LENGTHS)
    assert all(t["limited_samples"] > 0 and t["min_gain"] < 1.0 for t in tel)
    if n_streams == 1:
        assert tel[0] == {"min_gain": fold_envelope.min_gain, "limited_samples": fold_envelope.limited_samples}
    # every stream's smallest gain is the peak in tile 256 of the third call: without it the minimum is another
    less = LC.host_telemetry(n_streams, LC.FOLD_W, LC.fold_signal(n_streams, deepest=False), LC.FOLD_LENGTHS)
    assert all(b["min_gain"] > a["min_gain"] and b["limited_samples"] < a["limited_samples"] for a, b in zip(tel, less))
