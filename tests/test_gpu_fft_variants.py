"""The launch variants of the partition transforms (convopeq_amd/csrc/fft_kernels.hip) in isolation, through the diagnostic
entries cpq_diag_fft_forward, cpq_diag_fft_inverse_store and cpq_diag_ir_spectra: what an engine launches around the plain rows
that cpq_diag_partition_fft (tests/test_gpu_fft.py) covers --

  forward        launch_rfft_fwd_ols with a moving head, a ring that wraps and a history carried in from the call before
  side carry     launch_rfft_fwd_ols_side (P = 512): blocks copied to one or two other rows, a table stored, a tail moved
  ring store     launch_rfft_inv_ols_ring (store_block2 MODE 1) at even, odd, wrapping, 2^40-range and tabled positions
  tail store     launch_rfft_inv_ols_tail (MODE 2): the replayed delay-line reader added to the rows as they are stored
  add store      launch_rfft_inv_ols_add  (MODE 3, P = 512): one or two delay-line rings added to the rows
  IR spectra     launch_ir_spectra at the edges of h_eff's length, launch_spectrum_gain with a factor of its own per bin

per kernel family: P = 64, 256 radix-2 Stockham in LDS; 512 wave-level; 1024, 2048 mixed radix in LDS; 4096 four-step in a workgroup; 8192 four-step
through scratch with 16-point columns; 65536, 131072 the 128- and 256-point column variants.  3 channels x 5 blocks up to
P = 4096, 2 x 2 above.

Expectations.  The library is built with -ffp-contract=off, the transform in front of a store is the same code in every MODE
instantiation of a family and does not depend on head, position or history source.  So what a variant stores is, BIT FOR BIT,
what cpq_diag_partition_fft (MODE 0) gives for the same frame or spectrum, followed -- for MODE 2 and 3 -- by the roundings
written in store_block2, restated here in numpy fp64 (numpy contracts nothing either): y + x when |g - 1| < 1e-12, else
y + x * g (two roundings), layer 1 / ring A before layer 2 / ring B.  Copies (side rows, table, tail, histNew, XDN / HDN) and
the one multiply of k_spectrum_gain are exact as well.  Only the comparison with numpy.fft.rfft carries a tolerance, the one of
tests/test_gpu_fft.py: 4e-15 of the largest bin of the frame.  Every buffer comes back whole and was filled with 0xFF bytes by
the entry, so "untouched" is an assertion on bits, too.

No argument set here lets a kernel leave a buffer: the entries refuse those, and test_refusals walks the rules."""
import numpy as np
import pytest

from fft_layout import bins, dp
import fft_variant_calls as V
from fft_variant_calls import same_bits, untouched

pytestmark = pytest.mark.gpu

FAMILIES = [64, 256, 512, 1024, 2048, 4096, 8192, 65536, 131072]
TOL = 4e-15                                 # tests/test_gpu_fft.py: of the largest bin of the frame
GAINS = [(1.0, 1.0 + 5e-13), (0.5, 1.0 + 1e-11)]          # both `y + x`; both `y + x * g`


def shape(P):
    return (3, 5) if P <= 4096 else (2, 2)


@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need a gfx950 device")
    from convopeq_amd import _capi
    return _capi.load()


def blocks(P, n_ch, T, seed):
    """seeded noise with a silent block and an impulse block, as tests/test_gpu_fft.py"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_ch, T, P))
    x[0, T - 1] = 0.0
    x[n_ch - 1, 0] = 0.0
    x[n_ch - 1, 0, 17] = 1.0
    return x


def mode0(lib, x):
    """cpq_diag_partition_fft of x [n_ch][T][P] (silent history): (spectra [n_ch][T][P][2], rows [n_ch][T][P])"""
    n_ch, T, P = x.shape
    spec, out = np.full((n_ch, T, P, 2), -7.0), np.full((n_ch, T, P), -7.0)
    assert lib.cpq_diag_partition_fft(P, n_ch, T, dp(np.ascontiguousarray(x)), dp(spec), dp(out)) == 0
    return spec, out


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
        for a in _cache[key]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cache[key]


def forward_case(lib, P, n_ch, T):
    """(blocks, history, MODE 0 spectra of the frames [previous | block t] with the history in front of block 0)"""
    def make():
        x = blocks(P, n_ch, T, 7000 + P + T)
        hist = np.random.default_rng(7100 + P + T).standard_normal((n_ch, P))
        spec, _ = mode0(lib, np.concatenate([hist[:, None], x], axis=1))
        return x, hist, np.ascontiguousarray(spec[:, 1:])
    return cached(("fwd", P, n_ch, T), make)


def inverse_case(lib, P):
    """(spectra [n_ch][T][P][2] of random blocks, their MODE 0 rows [n_ch][T][P])"""
    def make():
        n_ch, T = shape(P)
        return mode0(lib, blocks(P, n_ch, T, 8000 + P))
    return cached(("inv", P), make)


def check_forward(P, x, hist, ref, head, ring_slots, o):
    """ring placement, history source, XDN, histNew; returns the distance to numpy.fft.rfft"""
    n_ch, T, _ = x.shape
    b = bins(P)
    slots = [(head + t) & (ring_slots - 1) for t in range(T)]
    worst = 0.0
    for c in range(n_ch):
        prev = hist[c]
        for t in range(T):
            got = o["ring"][c, slots[t]]
            assert same_bits(got, ref[c, t]), (P, c, t, "slot differs from the MODE 0 spectrum of the same frame")
            r = np.fft.rfft(np.concatenate([prev, x[c, t]]))
            scale = max(np.abs(r).max(), 1e-300)
            g = got[:, 0] + 1j * got[:, 1]
            assert abs(g[0].real - r[0].real) <= TOL * scale and abs(g[0].imag - r[P].real) <= TOL * scale, (P, c, t)
            err = np.abs(g[1:] - r[b[1:]]).max() / scale
            worst = max(worst, err)
            assert err <= TOL, (P, c, t, err)
            assert same_bits(o["xdn"][c, slots[t]], got[0]), (P, c, t, "XDN")
            prev = x[c, t]
    rest = [s for s in range(ring_slots) if s not in slots]
    assert untouched(o["ring"][:, rest]) and untouched(o["xdn"][:, rest]), (P, head, "a slot outside (head + t) & mask was written")
    assert same_bits(o["hist_new"], x[:, T - 1]), (P, "histNew")
    return worst


def forward_heads(P):
    n_ch, T = shape(P)
    ring = 8 if P <= 4096 else 4
    return [(n_ch, T, ring, h) for h in ((6, 0, 7) if P <= 4096 else (3, 0))] + [(n_ch, 1, ring, ring - 1)]


@pytest.mark.parametrize("P", FAMILIES)
def test_forward_ring_placement_and_history(lib, P):
    """head + T wraps the ring (8 slots, 5 blocks, head 6; above 4096: 4 slots, 2 blocks, head 3), head 0, head = slots - 1, and
    one block alone (the history is its only predecessor)"""
    for n_ch, T, ring, head in forward_heads(P):
        x, hist, ref = forward_case(lib, P, n_ch, T)
        rc, o = V.fft_forward(lib, P, n_ch, T, head, ring, np.ascontiguousarray(x.reshape(n_ch, T * P)), hist)
        assert rc == 0
        d = check_forward(P, x, hist, ref, head, ring, o)
        print(f"forward P = {P}: {T} blocks, head {head} of {ring}: {d:.2e} of the largest bin; ring, XDN, histNew bit-equal")


def test_forward_p4_ragged_split(lib):
    """7 blocks of one channel: the launcher's own split (4 workgroups of 2, 2, 2, 1 frames), ring of 8 from head 6"""
    P, n_ch, T = 4096, 1, 7
    x, hist, ref = forward_case(lib, P, n_ch, T)
    rc, o = V.fft_forward(lib, P, n_ch, T, 6, 8, np.ascontiguousarray(x.reshape(n_ch, T * P)), hist)
    assert rc == 0
    d = check_forward(P, x, hist, ref, 6, 8, o)
    print(f"forward P = 4096, 1 channel x 7 blocks: {d:.2e} of the largest bin")


# (n_side, n_tab, tail_len): every value of every axis
SIDE_CASES = [(0, 0, 0), (1, 1, 1), (2, 64, 63), (2, 0, 65), (1, 64, 511), (0, 1, 63), (2, 1, 0)]


@pytest.mark.parametrize("n_side,n_tab,tail_len", SIDE_CASES)
def test_side_carry(lib, n_side, n_tab, tail_len):
    P, n_ch, T, head, ring = 512, 3, 5, 6, 8
    x, hist, ref = forward_case(lib, P, n_ch, T)

    def plain():
        rc, o = V.fft_forward(lib, P, n_ch, T, head, ring, np.ascontiguousarray(x.reshape(n_ch, T * P)), hist)
        assert rc == 0
        return o["ring"], o["xdn"], o["hist_new"]
    p_ring, p_xdn, p_hist = cached(("plain512",), plain)
    rows = np.concatenate([x.reshape(n_ch, T * P), np.random.default_rng(tail_len).standard_normal((n_ch, tail_len))], axis=1)
    strides, offs = (T * P + 40, T * P + 258)[:n_side], (6, 130)[:n_side]
    tab = (np.arange(n_tab, dtype=np.int64) * 0x100000001 + 3) * (-1) ** np.arange(n_tab)
    tail_stride = tail_len + 3
    rc, o = V.fft_forward(lib, P, n_ch, T, head, ring, np.ascontiguousarray(rows), hist, side=1, n_side=n_side, strides=strides,
                          offs=offs, tab=tab, tail_len=tail_len, tail_stride=tail_stride)
    assert rc == 0
    assert same_bits(o["ring"], p_ring) and same_bits(o["xdn"], p_xdn) and same_bits(o["hist_new"], p_hist)
    check_forward(P, x, hist, ref, head, ring, o)
    for a in range(n_side):
        got = o["side"][a]
        assert same_bits(got[:, offs[a]:offs[a] + T * P], x.reshape(n_ch, T * P)), (a, "side rows")
        assert untouched(got[:, :offs[a]]) and untouched(got[:, offs[a] + T * P:]), (a, "around the side rows")
    assert np.array_equal(o["tab"][:n_tab], tab) and (o["tab"][n_tab:] == -1).all()
    assert same_bits(o["tail"][:, :tail_len], rows[:, T * P:]) and untouched(o["tail"][:, tail_len:])


def ring_cases(P, T):
    """(label, blocks used, ring size, position table or None, pos0)"""
    big = 16 * P
    cases = [("pos0 even", T, big, None, 6), ("pos0 odd", T, big, None, 7),
             ("straddles the ring end, even", 2, 2 * P, None, P + 2), ("straddles the ring end, odd", 2, 2 * P, None, P + 3),
             ("2^40 range, even", T, big, None, (1 << 40) + (1 << 31) + 6), ("2^40 range, odd", T, big, None, (1 << 40) + (1 << 31) + 7)]
    if T == 5:
        cases.append(("table", T, big, [P + 4, 3 * P + 1, -1, 7 * P + 2, 15 * P + P // 2 + 5], 0))
    else:
        cases += [("table, odd and even", T, big, [P + 1, 15 * P + P // 2], 0), ("table, dropped and even", T, big, [-1, 4 * P], 0),
                  ("table, odd wrapping and dropped", T, big, [15 * P + P // 2 + 5, -3], 0)]
    return cases


@pytest.mark.parametrize("P", FAMILIES)
def test_ring_store(lib, P):
    """MODE 1: sample i of block t at ring[c][(p_t + i) & mask], bit-equal to the MODE 0 row; nothing else changes"""
    n_ch, T = shape(P)
    spec, rows = inverse_case(lib, P)
    n = 0
    for label, nb, size, table, pos0 in ring_cases(P, T):
        init = np.random.default_rng(P + size).standard_normal((n_ch, size))
        rc, o = V.fft_inverse_store(lib, 1, P, n_ch, nb, np.ascontiguousarray(spec[:, :nb]), ring_a=init, pos_a=table, pos0=pos0)
        assert rc == 0, label
        want = init.copy()
        for t in range(nb):
            p = table[t] if table is not None else pos0 + t * P
            if p >= 0:
                want[:, (p + np.arange(P)) & (size - 1)] = rows[:, t]
        assert same_bits(o["ring_a"], want), (P, label, int((o["ring_a"] != want).sum()))
        n += 1
    print(f"ring store P = {P}: {n} position sets, every ring bit-equal to the MODE 0 rows placed by numpy")


def tail_schedule(B, n_cb, n_tail, g0, n_samples, ring):
    """entries of every kind in turn: -1; inside the call; in the ring across its end; straddling g0; in the ring"""
    base = (g0 // ring) * ring
    kinds = [lambda cb: -1, lambda cb: g0 + (37 * cb + 11) % (n_samples - B + 1), lambda cb: base - ring - B // 2 - 1,
             lambda cb: g0 - B // 2 + 1, lambda cb: g0 - 3 * B + 5 - 2 * cb]
    return np.array([[kinds[(cb + 2 * l + 1) % 5](cb) for cb in range(n_cb)] for l in range(n_tail)], dtype=np.int64)


def tail_expected(rows, layer, ring, sched, B, g0, gains):
    """store_block2<2> in numpy fp64"""
    n_ch, n = rows.shape
    y = rows.copy()
    k = np.arange(n)
    for l in range(sched.shape[0]):
        s = sched[l, k // B]
        idx = s + k % B
        g = gains[l]
        for c in range(n_ch):
            x = np.where(idx >= g0, layer[l, c, np.clip(idx - g0, 0, n - 1)], ring[l, c, idx & (ring.shape[2] - 1)])
            add = y[c] + x if abs(g - 1.0) < 1.0e-12 else y[c] + x * g
            y[c] = np.where(s >= 0, add, y[c])
    return y


@pytest.mark.parametrize("P", [64, 512, 1024, 4096])
def test_tail_store(lib, P):
    """MODE 2 over n_tail {1, 2} x callback {P, P / 2, 2 P (4 blocks)} x the two gain pairs, g0 != 0"""
    n_ch = 3
    spec, rows = inverse_case(lib, P)
    n = 0
    for B in (P, P // 2, 2 * P):
        T = 4 if B == 2 * P else 5
        n_samples, ring = T * P, 4 * max(B, P)
        g0 = 8 * ring
        sp, r0 = np.ascontiguousarray(spec[:, :T]), np.ascontiguousarray(rows[:, :T]).reshape(n_ch, n_samples)
        rng = np.random.default_rng(9000 + P + B)
        layer, tring = rng.standard_normal((2, n_ch, n_samples)), rng.standard_normal((2, n_ch, ring))
        for n_tail in (1, 2):
            sched = tail_schedule(B, n_samples // B, n_tail, g0, n_samples, ring)
            assert (sched[sched >= 0] + B <= g0 + n_samples).all()
            lay, tr = np.ascontiguousarray(layer[:n_tail]), np.ascontiguousarray(tring[:n_tail])
            for g in GAINS:
                rc, o = V.fft_inverse_store(lib, 2, P, n_ch, T, sp, layer_out=lay, tail_ring=tr, g0=g0, sched=sched, B=B, n_tail=n_tail, g1=g[0], g2=g[1])
                assert rc == 0
                want = tail_expected(r0, lay, tr, sched, B, g0, g)
                assert not same_bits(want, r0)
                assert same_bits(o["out"], want), (P, B, n_tail, g, int((o["out"] != want).sum()))
                n += 1
        rc, o = V.fft_inverse_store(lib, 2, P, n_ch, T, sp, layer_out=layer, tail_ring=tring, g0=g0, sched=np.full((2, n_samples // B), -1), B=B,
                                    n_tail=2, g1=0.5, g2=0.5)
        assert rc == 0 and same_bits(o["out"], r0), (P, B, "a schedule of -1 must leave the MODE 0 rows")
        n += 1
    print(f"tail store P = {P}: {n} launches, every row bit-equal to the numpy restatement of store_block2<2>")


@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("gains", GAINS)
def test_add_store(lib, with_b, gains):
    """MODE 3: ring A (gain 1) then ring B (gain 2) added to the rows; -1, even and odd positions; a position whose i lands on
    the last ring element with i + 1 on the first; the rings stay as they are"""
    P, n_ch, T = 512, 3, 5
    spec, rows = inverse_case(lib, P)
    rng = np.random.default_rng(515)
    ra, rb = rng.standard_normal((n_ch, 4 * P)), rng.standard_normal((n_ch, 2 * P))
    pa = np.array([-1, 6, P + 77, 4 * P - 255, (1 << 40) + 2], dtype=np.int64)           # 4 P - 255 + i = 4 P - 1 at i = 254
    pb = np.array([2 * P - 1, -1, 10, 5 * P + 300, 2 * P - 37], dtype=np.int64)          # i = 0 on the last element; i = 36
    rc, o = V.fft_inverse_store(lib, 3, P, n_ch, T, spec, ring_a=ra, pos_a=pa, ring_b=rb if with_b else None,
                                pos_b=pb if with_b else None, g1=gains[0], g2=gains[1])
    assert rc == 0
    want = rows.copy()
    for ring, pos, g in ((ra, pa, gains[0]),) + (((rb, pb, gains[1]),) if with_b else ()):
        for t in range(T):
            if pos[t] >= 0:
                x = ring[:, (pos[t] + np.arange(P)) & (ring.shape[1] - 1)]
                want[:, t] = want[:, t] + x if abs(g - 1.0) < 1.0e-12 else want[:, t] + x * g
    assert same_bits(want[:, 0], rows[:, 0]) != with_b
    assert same_bits(o["out"], want.reshape(n_ch, T * P)), int((o["out"] != want.reshape(n_ch, T * P)).sum())
    assert same_bits(o["ring_a"], ra) and (not with_b or same_bits(o["ring_b"], rb))


def ir_lengths(P, n_parts):
    return [n_parts * P, (n_parts - 1) * P + 1, (n_parts - 1) * P + P // 2 + 11, (n_parts - 1) * P, P - 37]


@pytest.mark.parametrize("P", FAMILIES)
def test_ir_spectra_and_gain(lib, P):
    """h_eff ending on a partition, one sample into the last, on an odd sample inside it, one partition short, and inside the
    first; then gain[b] = 1 + b / (4 P), a factor of its own per bin, which pins the bin of every storage element"""
    n_parts = 3 if P <= 4096 else 2
    h = np.random.default_rng(6000 + P).standard_normal(n_parts * P)
    gain = 1.0 + np.arange(P + 1) / (4.0 * P)
    b = bins(P)
    assert sorted(b.tolist()) == list(range(P)) and gain[0] != gain[P]
    worst = 0.0
    for length in ir_lengths(P, n_parts):
        rc, o = V.ir_spectra(lib, P, n_parts, h, length, gain)
        assert rc == 0
        H = o["h"]
        hz = np.concatenate([h[:length], np.zeros(n_parts * P - length)])
        for k in range(n_parts):
            if k * P >= length:
                assert (H[k].view(np.uint64) == 0).all(), (P, length, k, "a partition behind the end is not +0.0 throughout")
                continue
            r = np.fft.rfft(np.concatenate([hz[k * P:(k + 1) * P], np.zeros(P)]))
            scale = np.abs(r).max()
            g = H[k, :, 0] + 1j * H[k, :, 1]
            assert abs(g[0].real - r[0].real) <= TOL * scale and abs(g[0].imag - r[P].real) <= TOL * scale, (P, length, k)
            err = np.abs(g[1:] - r[b[1:]]).max() / scale
            worst = max(worst, err)
            assert err <= TOL, (P, length, k, err)
        assert same_bits(o["hdn"], H[:, 0]), (P, length, "HDN")
        want = H * gain[b][None, :, None]
        want[:, 0, 1] = H[:, 0, 1] * gain[P]
        assert same_bits(o["h_gain"], want), (P, length, int((o["h_gain"] != want).sum()))
        assert same_bits(o["hdn_gain"], want[:, 0]), (P, length, "HDN after the gain")
    print(f"IR spectra P = {P}: {worst:.2e} of the largest bin over 5 lengths; HDN and the gain per bin bit-equal")


def test_refusals(lib):
    res = V.walk_refusals(lib)
    assert len(res) >= 55
    assert [r for r in res if r[2] != V.INVALID_ARG] == []
    assert V.valid_calls(lib) == [(k, 0) for k in ("forward", "forward", "inverse", "inverse", "inverse", "ir")]
