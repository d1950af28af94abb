"""The host object of cpq_quantizer (Quantizer(host=True)) against tests/quant_model.py and against the reference's recorded
shaper outputs (tests/golden/dither_ref.npz).  Every comparison is equality of bytes: there is no tolerance."""
import os

import numpy as np
import pytest

import convopeq_amd as amd
import dither_model as D
import quant_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
RATE = 48000.0
GUARD = 0xA5
# bit depth x container: every depth the container is wide enough for
DEPTHS = [(8, M.S16), (8, M.S24), (8, M.S32), (16, M.S16), (16, M.S24), (16, M.S32), (24, M.S24), (24, M.S32)]


def signal(n_streams, n, seed, level=0.4):
    return level * np.random.default_rng(seed).standard_normal((2 * n_streams, n))


def pair(n_streams, shaper, bits, fmt, rate=RATE, gains=None):
    host = amd.Quantizer(n_streams, rate, shaper, bits, fmt, host=True)
    model = M.Quantizer(rate, n_streams, shaper, bits, fmt)
    if gains is not None:
        host.set_gains(gains)
        model.set_gains(gains)
    return host, model


def guarded(q, layout, n, gap):
    """a packed buffer with `gap` guard bytes after every row and a guard row before and after: (whole, the rows [R, pitch])"""
    r, width = q.packed_shape(layout, n)
    whole = np.full((r + 2, width + gap), GUARD, dtype=np.uint8)
    return whole, whole[1:r + 1]


def guards_intact(whole, width):
    return (whole[0] == GUARD).all() and (whole[-1] == GUARD).all() and (whole[1:-1, width:] == GUARD).all()


@pytest.mark.parametrize("layout", (M.PLANAR, M.INTERLEAVED), ids=("planar", "interleaved"))
@pytest.mark.parametrize("bits,fmt", DEPTHS)
@pytest.mark.parametrize("shaper", M.SHAPERS)
def test_host_object_equals_the_model(shaper, bits, fmt, layout):
    S, n = 2, 150
    gains = [0.9, 1.3]
    x = signal(S, n, 100 * shaper + bits)
    host, model = pair(S, shaper, bits, fmt, gains=gains)
    gap = 4 * (1 + layout)                                      # a pitch wider than the row, a multiple of every element
    whole, rows = guarded(host, layout, n, gap)
    got = host.process(x, layout, out=rows)
    want = model.process(x, layout)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert guards_intact(whole, want.shape[1])
    codes = M.decode(got, fmt, layout, S)
    step = 1 << (M.WIDTH[fmt] - bits)
    top = (1 << (M.WIDTH[fmt] - 1)) - 1                         # the 4-tap shaper's +1.0, saturated: the one code off the grid
    off = codes % step != 0
    assert codes.any() and (codes[off] == top).all() and (shaper == M.FIXED4 or not off.any())
    # a second call carries the state: the tight pitch this time
    x2 = signal(S, 70, 7)
    assert np.array_equal(host.process(x2, layout), model.process(x2, layout))


@pytest.mark.parametrize("rate", (44100.0, 48000.0, 64000.0, 1.0e6))
@pytest.mark.parametrize("shaper", (M.FIXED4, M.FIXED15))
def test_sixteen_bit_bytes_equal_the_reference_recorded_outputs(shaper, rate):
    fx = np.load(os.path.join(HERE, "golden", "dither_ref.npz"))
    x, (n1, n2), h = fx["input"], fx["calls"], float(fx["headroom"])
    want = D.encode16(D.recorded(fx, shaper, 16, rate)).astype(np.int64)        # recorded * 2^15, saturated, NaN -> 0
    with np.errstate(invalid="ignore"):
        xh = x * h                                               # the reference's x = in * headroom, one rounding
    for gain, rows in ((1.0, xh), (h, x)):
        q = amd.Quantizer(1, rate, shaper, 16, M.S16, host=True)
        q.set_gains([gain])
        got = np.concatenate([q.process(rows[:, :n1]), q.process(rows[:, n1:])], axis=1)
        assert np.array_equal(M.decode(got, M.S16, M.PLANAR, 1), want), gain
    assert (want == 32767).any() and (want == -32768).any()


@pytest.mark.parametrize("shaper", M.SHAPERS)
def test_every_split_into_calls_gives_the_same_bytes(shaper):
    S = 2
    pieces = [1, 63, 64, 65, 1, 7, 300, 4096, 4097, 29]        # tile seams, the host object's chunk of 4096 and ragged ends
    n = sum(pieces)
    x = signal(S, n, shaper)
    for fmt, layout in ((M.S16, M.PLANAR), (M.S24, M.INTERLEAVED)):
        whole = amd.Quantizer(S, RATE, shaper, 16, fmt, host=True)
        split = amd.Quantizer(S, RATE, shaper, 16, fmt, host=True)
        for q in (whole, split):
            q.set_gains([0.7, 1.1])
        one = whole.process(x, layout)
        parts, at = [], 0
        for k in pieces:
            parts.append(M.decode(split.process(x[:, at:at + k], layout), fmt, layout, S))
            at += k
        assert np.array_equal(np.concatenate(parts, axis=1), M.decode(one, fmt, layout, S))
        # reset: the first run again
        whole.reset()
        assert np.array_equal(M.decode(whole.process(x[:, :500], layout), fmt, layout, S), np.concatenate(parts, axis=1)[:, :500])


def test_the_rails_and_the_saturation_of_the_four_tap_shaper():
    """input at and above +-1.0 at bit_depth == width: the 4-tap shaper does not clamp its code and emits +1.0 and
    -1 - 2^-15, which the pack saturates; the other two clamp the code themselves"""
    n = 240
    x = np.empty((2, n))
    x[0, :80], x[0, 80:160], x[0, 160:] = 1.0, 1.5, -1.5
    x[1, :80], x[1, 80:160], x[1, 160:] = -1.0, -3.0, 1.0 - 2.0 ** -15
    for shaper in M.SHAPERS:
        host, model = pair(1, shaper, 16, M.S16)
        yq = M.Quantizer(RATE, 1, shaper, 16, M.S16).shaped(x)
        got = host.process(x)
        assert np.array_equal(got, model.process(x))
        codes = M.decode(got, M.S16, M.PLANAR, 1)
        if shaper == M.FIXED4:
            assert (yq == 1.0).any() and (yq == -1.0 - 2.0 ** -15).any()          # the input reaches both
            assert (codes[yq == 1.0] == 32767).all() and (codes[yq == -1.0 - 2.0 ** -15] == -32768).all()
        else:
            assert yq.max() == 1.0 - 2.0 ** -15 and yq.min() == -1.0
        assert codes.max() == 32767 and codes.min() == -32768


@pytest.mark.parametrize("shaper", M.SHAPERS)
def test_samples_that_are_not_finite(shaper):
    n = 200
    x = signal(1, n, 5, level=0.2)
    x[0, 50], x[1, 51], x[0, 120], x[1, 64] = np.nan, np.inf, -np.inf, np.nan
    for fmt in (M.S16, M.S24):
        host, model = pair(1, shaper, 16, fmt)
        got = host.process(x, M.INTERLEAVED)
        assert np.array_equal(got, model.process(x, M.INTERLEAVED))
        codes = M.decode(got, fmt, M.INTERLEAVED, 1) >> (M.WIDTH[fmt] - 16)
        if shaper == M.FIXED4:
            # a y that is not finite reads as 0 before the clamp: the sample is the dither of a zero
            assert all(abs(int(codes[c, i])) <= 1 for c, i in ((0, 50), (1, 51), (0, 120), (1, 64)))
        else:
            # a NaN in is a NaN out for that sample, which packs to 0; an infinity clamps to the rail it points at
            assert codes[0, 50] == 0 and codes[1, 64] == 0
            assert codes[1, 51] in (32766, 32767) and codes[0, 120] in (-32768, -32767)
        # the neighbours go on as the model says (compared above) and stay small: the stored error of such a sample is finite
        assert np.abs(codes[:, 52:60]).max() < 32768 // 2 and np.abs(codes[:, 121:130]).max() < 32768 // 2


@pytest.mark.parametrize("shaper", M.SHAPERS)
def test_gain_zero_is_the_dither_of_silence(shaper):
    x = signal(2, 130, 3)
    zero = amd.Quantizer(2, RATE, shaper, 16, M.S16, host=True)
    zero.set_gains([0.0, 1.0])
    ones = amd.Quantizer(2, RATE, shaper, 16, M.S16, host=True)
    silent = x.copy()
    silent[:2] = 0.0
    got, want = zero.process(x), ones.process(silent)
    assert np.array_equal(got, want)
    model = M.Quantizer(RATE, 2, shaper, 16, M.S16)
    model.set_gains([0.0, 1.0])
    assert np.array_equal(got, model.process(x))
    codes = M.decode(got, M.S16, M.PLANAR, 2)
    assert codes[:2].any() and np.abs(codes[:2]).max() <= 8


def test_adaptive_coefficients_set_in_the_middle_of_a_programme():
    S = 3
    x = signal(S, 180, 11)
    host, model = pair(S, M.ADAPTIVE9, 16, M.S24, gains=[1.0, 0.5, 1.5])
    k1 = [0.5, -0.3, 0.2, 2.0, np.nan, -9.0]                     # clamped to +-0.85, not finite -> 0, the missing ones 0
    k2 = np.linspace(-0.4, 0.4, 9)
    out, want = [], []
    for step, (a, b) in enumerate(((0, 60), (60, 120), (120, 180))):
        if step == 1:
            host.set_adaptive_coeffs(1, k1)
            model.set_adaptive_coeffs(1, k1)
        if step == 2:
            host.set_adaptive_coeffs(amd.CPQ_ALL_STREAMS, k2)
            model.set_adaptive_coeffs(-1, k2)
        out.append(host.process(x[:, a:b]))
        want.append(model.process(x[:, a:b]))
        if step == 1:
            assert np.array_equal(host.adaptive_coeffs(1), [0.5, -0.3, 0.2, 0.85, 0.0, -0.85, 0.0, 0.0, 0.0])
            assert np.array_equal(host.adaptive_coeffs(0), host.adaptive_coeffs(2)) and host.adaptive_coeffs(0)[0] == -0.003796
    for g, w in zip(out, want):
        assert np.array_equal(g, w)
    assert np.array_equal(host.adaptive_coeffs(2), k2)
    # reset keeps the coefficients and the gains
    host.reset()
    model.reset()
    assert np.array_equal(host.adaptive_coeffs(0), k2)
    assert np.array_equal(host.process(x[:, :50]), model.process(x[:, :50]))
