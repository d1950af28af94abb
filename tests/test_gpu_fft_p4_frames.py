"""The frame loop of the P = 4096 transforms (k_rfft_fwd_ols_p4 / k_rfft_inv_ols_p4): one workgroup walks a contiguous range
of frames of one channel, the forward transform carrying the half frame that frames t and t + 1 share in registers -- and
any scheme that loads frame t + 1 while frame t computes has to pass here (the one that was built did, and was not kept
because it gained nothing: RESULTS.md).  cpq_diag_partition_fft_split sets the number of workgroups per channel, so that
small inputs give ranges of 1, 2, 3, 4 and 7 frames, a ragged last range and an empty one (n_blocks = 5, split = 4: ranges
2, 2, 1 and a workgroup that returns at once), on the first and the last channel.

Input: seeded noise, frame t of channel c scaled by 2^(t + 8 c): a block taken from the wrong t or c is off by a factor of
two at least.

Checks, per shape: forward spectra against numpy.fft.rfft of [previous block | block], inverse against numpy's irfft and
against the input, in the storage order and with the bounds of tests/test_gpu_fft.py (4e-15 forward and inverse, 2e-15 round
trip: log2(8192) = 13 butterfly levels of fp64 rounding).  That file normalises by the largest bin of the frame and by the
largest sample; here every frame has a scale of its own, so the inverse and the round trip are normalised per frame by the
largest sample of the frame [previous block | block] whose spectrum is inverted (the rounding of an inverse transform is
relative to its whole 2P-point result; with equal scales this is test_gpu_fft.py's normalisation).  Then bit equality with
split = n_blocks, where every workgroup has one frame and nothing is carried from frame to frame.

One case through an engine: 3 streams, P = 4096, two consecutive calls of 3 and 5 partitions, reference semantics of a
time-varying plan (1024-sample callbacks, 131072 taps), i.e. the layered path whose last inverse transform stores through
the delay-line reader (MODE 2), whose tail layers store plain rows (MODE 0) and whose forward transform carries histNew from
the first call into the second; against the oracle at 1e-13 RMS like tests/test_gpu_parity.py."""
import numpy as np
import pytest

import fft_layout
from fft_layout import dp
from mac_fft_calls import FFT_BAD, FFT_GOOD, FFT_VALID, INVALID_ARG, fft_split_call

pytestmark = pytest.mark.gpu

P = 4096
SHAPES = [(1, 1), (2, 1), (3, 1), (7, 1), (7, 2), (5, 4)]          # (n_blocks, split)


@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need a gfx950 device")
    from convopeq_amd import _capi
    return _capi.load()


def _bins():
    """storage element -> bin of the packed spectrum (element 0 = (DC, Nyquist)), as tests/test_gpu_fft.py"""
    return fft_layout.bins(P)


def _input(n_ch, T):
    rng = np.random.default_rng(4096 + 100 * n_ch + T)
    x = rng.standard_normal((n_ch, T, P))
    for c in range(n_ch):
        for t in range(T):
            x[c, t] *= 2.0 ** (t + 8 * c)
    return np.ascontiguousarray(x)


def _run(lib, x, split):
    n_ch, T, _ = x.shape
    spec = np.empty((n_ch, T, P, 2))
    out = np.empty((n_ch, T, P))
    assert lib.cpq_diag_partition_fft_split(P, n_ch, T, split, dp(x), dp(spec), dp(out)) == 0
    return spec, out


@pytest.mark.parametrize("n_blocks,split", SHAPES)
@pytest.mark.parametrize("n_ch", [1, 3])
def test_p4_frame_ranges(lib, n_ch, n_blocks, split):
    x = _input(n_ch, n_blocks)
    spec, out = _run(lib, x, split)
    bins = _bins()
    worst_f = worst_b = worst_rt = 0.0
    for c in range(n_ch):
        prev = np.zeros(P)
        for t in range(n_blocks):
            frame = np.concatenate([prev, x[c, t]])
            ref = np.fft.rfft(frame)
            got = spec[c, t, :, 0] + 1j * spec[c, t, :, 1]
            scale = np.abs(ref).max()
            assert abs(got[0].real - ref[0].real) <= 4e-15 * scale and abs(got[0].imag - ref[P].real) <= 4e-15 * scale, (c, t)
            err = np.abs(got[1:] - ref[bins[1:]]).max() / scale
            worst_f = max(worst_f, err)
            assert err <= 4e-15, (c, t, err)
            back = np.fft.irfft(ref, 2 * P)[P:]
            big = np.abs(frame).max()
            worst_b = max(worst_b, np.abs(out[c, t] - back).max() / big)
            worst_rt = max(worst_rt, np.abs(out[c, t] - x[c, t]).max() / big)
            prev = x[c, t]
    print(f"{n_ch} ch, {n_blocks} blocks, split {split}: forward {worst_f:.2e}, inverse {worst_b:.2e}, round trip {worst_rt:.2e}")
    assert worst_b <= 4e-15 and worst_rt <= 2e-15, (worst_b, worst_rt)
    # one frame per workgroup: nothing is carried from frame to frame
    spec1, out1 = _run(lib, x, n_blocks)
    assert np.array_equal(spec, spec1) and np.array_equal(out, out1)


def test_split_argument(lib):
    """split <= 0 is the engine's own choice (the result of cpq_diag_partition_fft); more workgroups than frames are refused;
    other partitions ignore the argument.  The argument sets: tests/mac_fft_calls.py, walked without a device too"""
    n_ch, T = FFT_GOOD["n_ch"], FFT_GOOD["T"]
    x = _input(n_ch, T)
    spec0, out0 = np.empty((n_ch, T, P, 2)), np.empty((n_ch, T, P))
    assert lib.cpq_diag_partition_fft(P, n_ch, T, dp(x), dp(spec0), dp(out0)) == 0
    y = np.ascontiguousarray(x[:, :, :512])
    a = np.empty((n_ch, T, 512, 2)), np.empty((n_ch, T, 512))
    assert lib.cpq_diag_partition_fft(512, n_ch, T, dp(y), dp(a[0]), dp(a[1])) == 0
    for what, override in FFT_VALID.items():
        v = dict(FFT_GOOD, **override)
        rc, spec, out = fft_split_call(lib, v, x if v["P"] == P else y)
        assert rc == 0, what
        want = (spec0, out0) if v["P"] == P else a
        assert np.array_equal(spec, want[0]) and np.array_equal(out, want[1]), what
    assert fft_split_call(lib, dict(FFT_GOOD, **FFT_BAD["split = T + 1"]), x)[0] == INVALID_ARG
    rc, spec, out = fft_split_call(lib, dict(FFT_GOOD, P=512, split=4), y)
    assert rc == 0 and np.array_equal(spec, a[0]) and np.array_equal(out, a[1])


def test_engine_two_calls_of_3_and_5_partitions(lib, oracle):
    import convopeq_amd as amd
    O = oracle
    S, block, L = 3, 1024, 131072
    irs = [O.gen_ir(L, stream=c // 2, channel=c % 2) for c in range(2 * S)]
    n = 8 * P
    x = np.empty((2 * S, n))
    for s in range(S):
        for ch in range(2):
            x[2 * s + ch] = O.gen_pcm(n, stream=s, channel=ch)
    ref = np.empty_like(x)
    for c in range(2 * S):
        nuc = O.Nuc()
        assert nuc.set_impulse(irs[c], block)
        ref[c] = nuc.run(x[c], block)
        nuc.close()
    assert O.plan(L, block).ltiValid == 0            # the layered path
    eng = amd.BatchedEngine(S, block_size=block, max_ir_len=L, max_blocks_per_call=5 * P // block, partition_size=P)
    assert eng.partition_size() == P
    for s in range(S):
        eng.set_impulse(s, irs[2 * s], irs[2 * s + 1])
    y = np.concatenate([eng.conv_process(x[:, :3 * P]), eng.conv_process(x[:, 3 * P:])], axis=1)
    err = float(np.sqrt(np.mean(np.square(y - ref))))
    print(f"engine, P = 4096, calls of 3 and 5 partitions: rms err {err:.3e}, signal rms {float(np.sqrt(np.mean(ref * ref))):.3f}")
    assert err <= 1e-13
    eng.close()
