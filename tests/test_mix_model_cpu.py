"""tests/mix_model.py checked without a GPU: the models of the direct head, the block RMS and the gain ramp against exact
rational arithmetic within bounds derived from their operation counts (u = 2^-53), and against the oracle where it exposes
the same step.

Bounds.  Direct head: nt products accumulated in at most nt / 8 + 3 rounded additions per path plus the scalar tail's two
roundings per tap; every rounding is relative to a partial sum bounded by S = sum |h| |x|, so |y - exact| <= (nt + 2) u S.
Mean square: B / 4 fused steps per lane, three lane additions, B % 4 <= 3 unfused steps of two roundings less one shared, the
divide: (B / 4 + 5) u relative (all terms are non-negative, so partial sums are bounded by the total).  Ramp: sample i is
reached by at most i / 16 + 3 + 1 rounded additions (or 1 + i % 4 in the remainder) of values bounded by |g|, plus the rounded
3 * inc: |g_i - (start + i * inc)| <= (i / 4 + 3) u max|g|.

The tail schedule model is pinned to oracle_lib.Nuc through its output (test_tail_schedule_against_the_oracle): an IR that is
one tap at a tail layer's offset turns the layer's delay line into the input itself, a ramp input x[n] = n + 1 makes every
output sample name the delay-line position it was read from, and a silent callback is one the reader skipped.  The write lag D
comes from the oracle's plan (doneCallback), not from the engine's formula.  A replay of the reference's two cursors
(test_tail_schedule_against_a_cursor_replay) covers parameter sets no plan produces."""
from fractions import Fraction

import numpy as np
import pytest

import mix_model as M

U = 2.0 ** -53


def test_fma_is_rounded_once():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30            # a * b = 1 - 2^-60: rounds to 1, the fused sum keeps -2^-60
    assert M.fma(a, b, -1.0) == -2.0 ** -60 and a * b - 1.0 == 0.0
    assert M.fma(3.0, 4.0, 5.0) == 17.0 and M.fma(np.inf, 1.0, 1.0) == np.inf and np.isnan(M.fma(np.inf, 0.0, 1.0))
    rng = np.random.default_rng(0)
    for a, b, c in rng.standard_normal((200, 3)):
        assert M.fma(a, b, c) == float(Fraction(a) * Fraction(b) + Fraction(c))


@pytest.mark.parametrize("nt", [0, 1, 3, 7, 8, 9, 15, 16, 17, 24, 31, 32])
def test_direct_head_against_exact_and_oracle(oracle, nt):
    rng = np.random.default_rng(nt)
    n = 40
    x, hist, h = rng.standard_normal((1, n)), rng.standard_normal((1, 32)), rng.standard_normal(32)
    ir_rev = np.zeros((1, 32))
    ir_rev[0, :nt] = h[:nt][::-1]                       # reversed taps: ir_rev[k] multiplies the sample nt - 1 - k back
    dout, hist_new = M.direct_head(x, ir_rev, [nt], [0], hist)
    full = np.concatenate([hist[0], x[0]])
    assert np.array_equal(hist_new[0], full[-32:])
    for s in range(n):
        exact = sum(Fraction(h[k]) * Fraction(full[32 + s - k]) for k in range(nt))
        S = sum(abs(h[k]) * abs(full[32 + s - k]) for k in range(nt))
        assert abs(Fraction(dout[0, s]) - exact) <= (nt + 2) * U * S, (s, dout[0, s])
    if nt:
        ref = oracle.direct_conv_at(full, h[:nt], np.arange(32, 32 + n))
        S = np.convolve(np.abs(full), np.abs(h[:nt]))[32:32 + n]
        assert (np.abs(dout[0] - ref) <= 2 * (nt + 2) * U * S).all()


def test_direct_head_exact_model_agrees_on_integers():
    rng = np.random.default_rng(1)
    x, hist = rng.integers(-8, 9, (4, 70)).astype(float), rng.integers(-8, 9, (4, 32)).astype(float)
    ir, taps, slot = rng.integers(-8, 9, (3, 32)).astype(float), [32, 9, 0], [0, 1, 2, 1]
    assert np.array_equal(M.direct_head(x, ir, taps, slot, hist)[0], M.direct_head_exact(x, ir, taps, slot, hist))


@pytest.mark.parametrize("B", [1, 3, 4, 5, 63, 64, 66, 441, 512])
def test_block_rms_against_exact(B):
    d = np.random.default_rng(B).standard_normal(B)
    exact = sum(Fraction(v) ** 2 for v in d) / B
    ms = M.block_mean_square(d)
    assert abs(Fraction(ms) - exact) <= Fraction(B // 4 + 5) * Fraction(U) * exact
    assert M.block_rms(d) == float(np.sqrt(np.float64(ms)))                # one more correctly rounded operation
    assert M.block_rms(np.zeros(B)) == 0.0


@pytest.mark.parametrize("B", [1, 3, 4, 17, 64, 441, 512])
def test_ramp_against_the_line(B):
    rng = np.random.default_rng(B)
    for start, inc in [(1.0, 0.0), (0.5, 2.0 ** -10), (1.0 + 0.1 * rng.standard_normal(), 1e-3 * rng.standard_normal())]:
        g = M.ramp_gains(start, inc, B)
        line = [Fraction(start) + i * Fraction(inc) for i in range(B)]
        top = max(abs(start), abs(start + B * inc))
        for i in range(B):
            assert abs(Fraction(g[i]) - line[i]) <= (i // 4 + 3) * U * top, (B, i)
        if inc in (0.0, 2.0 ** -10):
            assert np.array_equal(g, start + np.arange(B) * inc)         # exact steps: no rounding anywhere


def test_linear_ramp_values_are_what_the_blend_and_the_mix_consume(oracle):
    """LinearRamp values as x_gains / bypass gains: the models use them as given; the equal-power gains of the mix ramp are
    orc_equal_power_sin of them"""
    r = oracle.LinearRamp(0.0, 48000.0, 0.001)
    r.set_target(1.0)
    g = np.array([r.next() for _ in range(60)])
    assert g[47] == 1.0 and g[-1] == 1.0 and (np.diff(g[:48]) > 0).all()
    ring = np.arange(64.0)[None, :].repeat(2, 0)
    wet = np.ones((2, 60))
    out = M.convproc_mix(wet, 60, np.array([[0.0, 1.0]]), ring, 64, [3], [10], x_len=[48], x_gains=g[None, :48])
    stream = oracle.ConvProcStream.__new__(oracle.ConvProcStream)
    stream.hist = [np.concatenate([ring[0], ring[0]])] * 2               # absolute position p holds p % 64
    for i in range(60):
        new, old = stream._dry(0, 64 + i, 3), stream._dry(0, 64 + i, 10)
        want = new * g[i] + old * (1.0 - g[i]) if i < 48 else new
        assert out[0, i] == want
    eps = oracle.lib().orc_equal_power_sin
    rg = np.array([[[eps(v), eps(1.0 - v)] for v in g]])
    mixed = M.convproc_mix(wet, 60, np.array([[eps(1.0), eps(0.0)]]), ring, 64, [0], [0], ramp_len=[50], ramp_gains=rg)
    for i in range(60):
        wg, dg = (rg[0, i, 0], rg[0, i, 1]) if i < 50 else (eps(1.0), eps(0.0))
        assert mixed[1, i] == 1.0 * wg + ring[1, i % 64] * dg


TAIL_PLANS = [(20000, {}), (131072, {}), (131072, dict(tailMode=0)), (300000, dict(tailStartSeconds=0.3, tailL1L2Multiplier=4))]


@pytest.mark.parametrize("ir_len,spec", TAIL_PLANS, ids=["20000", "131072", "131072-mode0", "300000-late-tail"])
def test_tail_schedule_against_the_oracle(oracle, ir_len, spec):
    """B = 1024, plans whose tail layer has PL = 8192 with outputDelay below PL (layered: the reader skips callbacks) and above
    it.  h = one tap at the layer's offset: the layer's natural-time output is x, so with x[n] = n + 1 callback c of the
    oracle's output is gain * (start(c) + j + 1), j < B, or silence when the reader skipped.  The values are integers below
    2^17 times the gain, carried through fp64 FFTs of 16384 points: the recovered start is within 1e-6 of an integer (1e-11
    observed), so rounding it is safe."""
    B, n_cb = 1024, 60
    sp = oracle.FilterSpec.defaults(**spec) if spec else None
    p = oracle.plan(ir_len, B, spec=sp)
    assert p.numLayers >= 2
    x = np.arange(1.0, n_cb * B + 1)
    for l in range(1, p.numLayers):
        PL, oL = p.partSize[l], p.outputDelay[l]
        D = p.doneCallback[l] - PL // B + 1            # the first block is complete after PL / B callbacks and readable D later
        h = np.zeros(ir_len)
        h[p.offset[l]] = 1.0
        nuc = oracle.Nuc()
        assert nuc.set_impulse(h, B, spec=sp)
        y = nuc.run(x, B).reshape(n_cb, B)
        nuc.close()
        seen = []
        for c in range(n_cb):
            if not y[c].any():
                seen.append(-1)
                continue
            s = y[c] / p.gain[l] - np.arange(B) - 1.0
            assert np.abs(s - np.round(s[0])).max() < 1.0e-6, (l, c)
            seen.append(int(np.round(s[0])))
        st, sched = M.tail_schedule([0, 0, 0, 0], n_cb, B, [(PL, oL, D)])
        assert sched[0] == seen, (PL, oL, D)
        assert sum(v >= 0 for v in seen) > 10 and (oL >= PL or -1 in seen[p.doneCallback[l]:])
        st1, a = M.tail_schedule([0, 0, 0, 0], 23, B, [(PL, oL, D)])           # the same over two calls
        _, b = M.tail_schedule(st1, n_cb - 23, B, [(PL, oL, D)])
        assert a[0] + b[0] == seen


def test_tail_schedule_against_a_cursor_replay():
    """delayLineWrite / delayLineReadAdd replayed with two plain cursors per layer, sample by sample in callbacks"""
    for B, PL, oL, D in [(64, 64, 32, 0), (64, 256, 64, 1), (64, 256, 256, 1), (64, 512, 704, 3), (1024, 4096, 2048, 0)]:
        write = read = 0
        pending, filled, want = [], 0, []
        for c in range(40):
            filled += B
            if filled == PL:                       # a partition filled up in callback c: its block reaches the delay line D later
                pending.append(c + D)
                filled = 0
            write += PL * sum(1 for p in pending if p == c)
            start = max(read, max(write - oL, 0))
            if start + B > write:
                want.append(-1)
            else:
                want.append(start)
                read = start + B
        st, sched = M.tail_schedule([0, 0, 0, 0], 40, B, [(PL, oL, D)])
        assert sched[0] == want and st == [40, read, 0, 0]
        st1, a = M.tail_schedule([0, 0, 0, 0], 13, B, [(PL, oL, D)])
        st2, b = M.tail_schedule(st1, 27, B, [(PL, oL, D)])
        assert a[0] + b[0] == want and st2[:3] == st[:3] and st2[3] == 13 * B


def test_small_models():
    ring = np.arange(8.0)[None, :]
    assert list(M.ring_get_chunks(np.full((1, 6), 9.0), [0], 6, 4, ring, [6, 1], [3, 2])[0]) == [6, 7, 0, 0, 1, 2]
    assert list(M.ring_add_chunks(np.ones((1, 6)), [0], 6, 4, ring, [-1, 7], 2.0)[0]) == [1, 1, 1, 1, 15, 1]
    assert list(M.ring_regrow(np.array([[4.0, 5, 6, 7]]), 8, 6)[0]) == [0, 0, 6, 7, 4, 5, 0, 0]
    assert list(M.ring_put(np.zeros((1, 4)), np.array([[1.0, 2, 3]]), 3, 3)[0]) == [2, 3, 0, 1]
    assert M.block_silence(np.array([[1e-8, 0], [0, -2e-8]]), 1, 1, 2).tolist() == [[1, 0]]
    out = M.tail_append(np.zeros((1, 1, 4)), np.arange(1.0, 7.0).reshape(1, 1, 6), [0, 9, 0, 8], 1)
    assert list(out[0, 0]) == [5, 6, 3, 4]                    # from = max(9 - 8, 6 - 4, 0) = 2: samples 2 .. 5 at (8 + i) % 4
