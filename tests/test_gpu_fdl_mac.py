"""The FDL multiply-accumulate kernels (convopeq_amd/csrc/mac_kernels.hip) in isolation, through the diagnostic entry
cpq_diag_fdl_mac: exactly the launches an engine makes for one call (launch_fdl_mac, then launch_fdl_mac_dcnyq for the 16- and
32-row tiles) on buffers this file fills, so that K (partitions in use), T (rows per call), head, the ring size, the IR slot
table and the kernel variant are chosen here and not by an engine.  Reference: plain numpy,

    Y[c, t, b] = sum_{k < K} X[c, (head + t - k) & (ring - 1), b] * H[slot[c], k, b]          (complex, b >= 1)
    Y[c, t, 0] = ( sum_k Re X Re H , sum_k Im X Im H )                                       (packed DC, Nyquist)

Exact cases.  X and H are integers in [-1024, 1024] stored as fp64 and the reference is int64.  The largest intermediate is
the Gauss term (a + b)(c + d) <= 2^22 per step over K <= 320 steps, below 2^31 << 2^53, so FMA or mul/add, the split real
part of the small tiles, the three-multiply form of the cooperative kernel and the wave reduction of k_fdl_mac_dcnyq must
all give the same BITS: the assertion is equality, and one dropped, doubled or misplaced row moves a result by >= 1.  What a
call must not consume is poisoned with 2^40 in both parts (finite and still exact: a consumed poison row shows as a difference
near 2^50): ring slots outside {head + t - k}, IR rows K .. h_rows - 1 of every slot, IR slots no channel names.  One case
per variant repeats with zeros there (the documented padding), so that a failure says which of the two broke.  The
diagnostic fills Y with NaN before the launch: an element no kernel stores fails too.

Products taken (a full cross product is not needed; every axis keeps all its values):
  * variant {4, 8, 16, 32, cooperative} x K {1 ... 25, 31, 32, 33, 63, 64, 65, 259} x T {TT - 1, 2 TT + 1} (cooperative: 9
    forced, 65) x IR slots {private, shared} at P = 64, 3 channels, head wrapping inside the K loop, smallest ring;
  * around the anchors K = 3, 9, 16, 33 per variant: T {1, TT - 1, TT, TT + 1, 2 TT + 1} (cooperative: 1, 9 forced; 48, 63,
    64, 65, 128, 129) x head {0, ring - 1, K / 2, ring - T / 2} x ring {smallest, twice that};
    (the ring holds at least K + T + 32 slots, so head + T and head - K cannot both wrap in one call: K / 2 makes head - k
    wrap inside the K loop, ring - T / 2 makes head + t wrap inside a tile);
  * P {64, 128, 256, 512} x channels {1, 3, 5, 9} and P = 4096 x channels {1, 3} per variant at K = 3, 9, 33 (at P = 4096 both
    kernels' workgroup counts are multiples of 16 whatever the channel count, so the early-return workgroups exist only
    below; 9 channels there would also need more than 64 MB);
  * IR slots {private, shared, permutation with a repeated and an unused slot} x h_rows {smallest, + 13} per variant;
  * tile = 0 at T = 5, 6, 11, 12, 47, 48: the variant used is 4, 8, 8, 16, 16, cooperative.

Kernel instantiations and a case that runs each (P = 64, 3 channels unless said):
  k_fdl_mac<4,4,0>   test_exact_k_sweep[4-*]  T = 9 (three tiles)        k_fdl_mac<8,4,0>   test_exact_k_sweep[8-*]  T = 17
  k_fdl_mac<4,4,1>   test_exact_k_sweep[4-*]  T = 3, shared slot         k_fdl_mac<8,4,1>   test_exact_k_sweep[8-*]  T = 7, shared
  k_fdl_mac<4,4,2>   test_exact_k_sweep[4-*]  T = 3, private slots       k_fdl_mac<8,4,2>   test_exact_k_sweep[8-*]  T = 7, private
  k_fdl_mac<16,4>    test_exact_k_sweep[16-*] T = 15, 33                 k_fdl_mac<32,4>    test_exact_k_sweep[32-*] T = 31, 65
  k_fdl_mac_wg       test_exact_k_sweep[coop-*] T = 9 (forced), 65; test_auto_variant[48-0]
  k_fdl_mac_dcnyq    every tile 16 / 32 case (bin 0): K < 64, = 64, = 65 and 259 in test_exact_k_sweep[16-*] / [32-*]

Rounding cases.  Standard-normal X and H (zeros outside the consumed set), reference in np.longdouble (exact rationals where
that is not wider than 2^-60), asserted per element with u = 2^-53:

    |Y - ref| <= (2 K + 8) u S,    S[c, t, b] = sum_k (|Re X| + |Im X|) (|Re H| + |Im H|)

A K-term FMA recurrence costs at most K u of its absolute sum to first order; the Gauss form adds one rounding each for
a + b and c + d and two final subtractions, and its three absolute sums together stay below 2 S; the tree reduction of
k_fdl_mac_dcnyq is below the recurrence.  The bound is derived, not fitted.  Worst |Y - ref| / (u S) printed on the device
(normal / cancelling input; bound 74 at K = 33, 526 at K = 259; measurements on an MI355X, the bound is not tuned to them):
    tile 4         K = 33: 1.65 / 2.28    K = 259: 1.57 / 5.23        tile 8         K = 33: 2.25 / 1.96    K = 259: 1.34 / 4.61
    tile 16        K = 33: 1.81 / 3.97    K = 259: 1.98 / 9.38        tile 32        K = 33: 2.09 / 3.00    K = 259: 2.09 / 7.97
    cooperative    K = 33: 2.32 / 2.91    K = 259: 1.78 / 7.16

One call equals two: a ring filled once, T rows in one call and as T1 + (T - T1) rows, bit-equal in the exact setting.

Measured on an MI355X: 340 tests, every exact case equal, 7.3 s for the whole file."""
import ctypes as C
import fractions

import numpy as np
import pytest

from mac_fft_calls import INVALID_ARG, MAC_BAD as BAD_ARGS, MAC_GOOD as GOOD, MAC_POINTERS, mac_buffers, mac_call

pytestmark = pytest.mark.gpu

COOP = -1                       # tile value of the diagnostic that forces the workgroup-cooperative kernel at any T
VARIANTS = [4, 8, 16, 32, COOP]
VID = {4: "4", 8: "8", 16: "16", 32: "32", COOP: "coop"}
K_SWEEP = list(range(1, 26)) + [31, 32, 33, 63, 64, 65, 259]
K_ANCHORS = [3, 9, 16, 33]
POISON = float(2 ** 40)


@pytest.fixture(scope="module")
def amd():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need a gfx950 device")
    import convopeq_amd
    return convopeq_amd


@pytest.fixture(scope="module")
def lib(amd):
    from convopeq_amd import _capi
    return _capi.load()


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def align_up(v, a):
    return (v + a - 1) // a * a


def ring_min(K, T):
    """the engines' ring size (engine_core.cpp, engine_native.cpp layerGeometry)"""
    return next_pow2(align_up(K, 32) + 32 + T)


def h_rows_min(K):
    """the smaller of the engines' two slot sizes (engine_native.cpp layerGeometry)"""
    return align_up(K, 32) + 16


def t_values(variant):
    if variant == COOP:
        return [1, 9, 48, 63, 64, 65, 128, 129]       # 1 and 9: forced below the automatic threshold of 48
    return [1, variant - 1, variant, variant + 1, 2 * variant + 1]


def sweep_t(variant):
    return [9, 65] if variant == COOP else [variant - 1, 2 * variant + 1]


def slot_table(mode, n_ch):
    """(ir_slot, n_ir_slots, h_private)"""
    if mode == "private":
        return np.arange(n_ch, dtype=np.int32), n_ch, 1
    if mode == "shared":                              # slot 0 is never named
        return np.full(n_ch, 1, dtype=np.int32), 2, 0
    assert mode == "perm"                             # reversed, the first two channels on one slot, slot 1 unused
    s = np.arange(n_ch, 0, -1, dtype=np.int32)
    if n_ch > 1:
        s[1] = s[0]
    s[s == 1] = 0
    return s, n_ch + 1, 0


def make_case(rng, P, n_ch, K, T, head, ring, slots, n_slots, h_rows, fill=POISON, normal=False):
    """X [n_ch][ring][P][2], H [n_slots][h_rows][P][2]: data where the call consumes, `fill` everywhere else"""
    draw = (lambda shape: rng.standard_normal(shape)) if normal else (lambda shape: rng.integers(-1024, 1025, shape).astype(np.float64))
    X = np.full((n_ch, ring, P, 2), fill)
    used = (head + np.arange(-(K - 1), T)) & (ring - 1)
    assert len(set(used.tolist())) == K + T - 1
    X[:, used] = draw((n_ch, K + T - 1, P, 2))
    H = np.full((n_slots, h_rows, P, 2), fill)
    for s in sorted(set(slots.tolist())):
        H[s, :K] = draw((K, P, 2))
    return X, H


def reference(X, H, slots, K, T, head, dtype):
    """(Y [n_ch][T][P][2], S [n_ch][T][P]) accumulated in `dtype` (np.int64: exact; np.longdouble)"""
    n_ch, ring, P, _ = X.shape
    rows = np.arange(T)
    p = np.zeros((n_ch, T, P), dtype)
    q = np.zeros_like(p)
    im = np.zeros_like(p)
    S = np.zeros_like(p)
    for k in range(K):
        x = X[:, (head + rows - k) & (ring - 1)].astype(dtype)         # [n_ch][T][P][2]
        h = H[slots, k].astype(dtype)[:, None]                         # [n_ch][1][P][2]
        p += x[..., 0] * h[..., 0]
        q += x[..., 1] * h[..., 1]
        im += x[..., 0] * h[..., 1] + x[..., 1] * h[..., 0]
        S += (np.abs(x[..., 0]) + np.abs(x[..., 1])) * (np.abs(h[..., 0]) + np.abs(h[..., 1]))
    Y = np.stack([p - q, im], axis=-1)
    Y[:, :, 0, 0] = p[:, :, 0]
    Y[:, :, 0, 1] = q[:, :, 0]
    return Y, S


def run_mac(lib, X, H, slots, K, T, tile, head, h_private, expect=0):
    n_ch, ring, P, _ = X.shape
    n_slots, h_rows = H.shape[:2]
    assert X.flags.c_contiguous and H.flags.c_contiguous and X.dtype == np.float64 and H.dtype == np.float64
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    Y = np.full((n_ch, T, P, 2), -7.0)
    used = C.c_int32(-99)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.cpq_diag_fdl_mac(P, n_ch, K, T, tile, head, ring, n_slots, h_rows, h_private, dp(X), dp(H),
                              slots.ctypes.data_as(C.POINTER(C.c_int32)), dp(Y), C.byref(used))
    assert rc == expect, (rc, expect)
    return Y, used.value


def check_exact(lib, rng, variant, P, n_ch, K, T, head, ring, mode="private", h_extra=0, fill=POISON):
    """one exact case; returns None or a one-line description of the failure"""
    slots, n_slots, h_private = slot_table(mode, n_ch)
    X, H = make_case(rng, P, n_ch, K, T, head, ring, slots, n_slots, h_rows_min(K) + h_extra, fill)
    got, used = run_mac(lib, X, H, slots, K, T, variant, head, h_private)
    assert used == (0 if variant == COOP else variant)
    ref, _ = reference(X, H, slots, K, T, head, np.int64)
    assert np.abs(ref).max() < 2 ** 31
    bad = ~(got == ref.astype(np.float64))            # NaN (an element that was not stored) differs too
    if not bad.any():
        return None
    c, t, b, part = np.argwhere(bad)[0]
    return (f"variant {VID[variant]} P {P} channels {n_ch} K {K} T {T} head {head} ring {ring} slots {mode} h_rows +{h_extra} "
            f"fill {fill:g}: {int(bad.any(axis=-1).sum())} of {bad[..., 0].size} elements differ, first at channel {c} block {t} "
            f"bin {b} ({'re' if part == 0 else 'im'}): got {got[c, t, b, part]!r}, expected {int(ref[c, t, b, part])}")


def assert_none_failed(failures, n_run):
    assert not failures, f"{len(failures)} of {n_run} cases differ:\n" + "\n".join(failures[:20])


# ------------------------------------------------------------------------------------------------ a. exact cases
@pytest.mark.parametrize("K", K_SWEEP)
@pytest.mark.parametrize("variant", VARIANTS, ids=[VID[v] for v in VARIANTS])
def test_exact_k_sweep(lib, variant, K):
    rng = np.random.default_rng(10000 * (variant + 2) + K)
    P, n_ch = 64, 3
    failures, n = [], 0
    for T in sweep_t(variant):
        ring = ring_min(K, T)
        for mode in ("private", "shared"):
            failures.append(check_exact(lib, rng, variant, P, n_ch, K, T, max(1, K // 2), ring, mode))
            n += 1
    assert_none_failed([f for f in failures if f], n)


@pytest.mark.parametrize("variant", VARIANTS, ids=[VID[v] for v in VARIANTS])
def test_exact_t_head_ring(lib, variant):
    rng = np.random.default_rng(777 + variant)
    failures, n = [], 0
    for T in t_values(variant):
        for K in K_ANCHORS:
            for ring in (ring_min(K, T), 2 * ring_min(K, T)):
                for head in sorted({0, ring - 1, max(1, K // 2), ring - max(1, T // 2)}):
                    failures.append(check_exact(lib, rng, variant, 64, 2, K, T, head, ring))
                    n += 1
    assert_none_failed([f for f in failures if f], n)


# P = 4096 with 1 and 3 channels only (module docstring: no early-return workgroups there, and 64 MB)
P_CHANNELS = [(P, n) for P in (64, 128, 256, 512) for n in (1, 3, 5, 9)] + [(4096, 1), (4096, 3)]


@pytest.mark.parametrize("P,n_ch", P_CHANNELS)
@pytest.mark.parametrize("variant", VARIANTS, ids=[VID[v] for v in VARIANTS])
def test_exact_partition_sizes_and_channels(lib, variant, P, n_ch):
    rng = np.random.default_rng(31 * P + 7 * n_ch + variant)
    failures, n = [], 0
    for K in (3, 9, 33):
        for T in ([48, 65] if variant == COOP else [variant + 1]):
            ring = ring_min(K, T)
            assert n_ch * ring * P * 16 <= 64 << 20
            failures.append(check_exact(lib, rng, variant, P, n_ch, K, T, ring - 2, ring, "private" if K != 9 else "shared"))
            n += 1
    assert_none_failed([f for f in failures if f], n)


@pytest.mark.parametrize("h_extra", [0, 13])
@pytest.mark.parametrize("mode", ["private", "shared", "perm"])
@pytest.mark.parametrize("variant", VARIANTS, ids=[VID[v] for v in VARIANTS])
def test_exact_ir_slot_tables(lib, variant, mode, h_extra):
    rng = np.random.default_rng(4242 + 10 * variant + h_extra)
    failures, n = [], 0
    for K in K_ANCHORS:
        for T in ([9, 65] if variant == COOP else [variant - 1, variant + 1]):       # one tile (streaming variants) and two
            failures.append(check_exact(lib, rng, variant, 128, 5, K, T, 1, ring_min(K, T), mode, h_extra))
            n += 1
    assert_none_failed([f for f in failures if f], n)


@pytest.mark.parametrize("variant", VARIANTS, ids=[VID[v] for v in VARIANTS])
def test_exact_with_zero_padding(lib, variant):
    """the documented contract (rows K ... of every IR slot are zero, a silent ring): the poisoned cases' twin"""
    rng = np.random.default_rng(99 + variant)
    failures, n = [], 0
    for K in (5, 33):
        for T in sweep_t(variant):
            failures.append(check_exact(lib, rng, variant, 64, 3, K, T, max(1, K // 2), ring_min(K, T), "private", 0, fill=0.0))
            n += 1
    assert_none_failed([f for f in failures if f], n)


@pytest.mark.parametrize("T,expected", [(5, 4), (6, 8), (11, 8), (12, 16), (47, 16), (48, 0)])
def test_auto_variant(lib, T, expected):
    rng = np.random.default_rng(500 + T)
    for K in (7, 33):
        for mode in ("private", "shared"):
            slots, n_slots, h_private = slot_table(mode, 3)
            ring = ring_min(K, T)
            X, H = make_case(rng, 64, 3, K, T, ring - 3, ring, slots, n_slots, h_rows_min(K))
            got, used = run_mac(lib, X, H, slots, K, T, 0, ring - 3, h_private)
            assert used == expected
            ref, _ = reference(X, H, slots, K, T, ring - 3, np.int64)
            assert np.array_equal(got, ref.astype(np.float64)), (T, K, mode, int((got != ref).any(axis=-1).sum()))


# --------------------------------------------------------------------------------------------- b. rounding cases
def exact_rational_error(X, H, slots, K, T, head, got):
    """|got - exact| and S per element with exact rational arithmetic (hosts whose long double is not wider than fp64)"""
    n_ch, ring, P, _ = X.shape
    F = fractions.Fraction
    err = np.zeros((n_ch, T, P))
    S = np.zeros((n_ch, T, P))
    for c in range(n_ch):
        for t in range(T):
            for b in range(P):
                p = q = im = F(0)
                s = 0.0
                for k in range(K):
                    a, bb = (F(float(v)) for v in X[c, (head + t - k) & (ring - 1), b])
                    cc, d = (F(float(v)) for v in H[slots[c], k, b])
                    p += a * cc
                    q += bb * d
                    im += a * d + bb * cc
                    s += float((abs(a) + abs(bb)) * (abs(cc) + abs(d)))
                re, im = (p, q) if b == 0 else (p - q, im)
                dr, di = float(F(float(got[c, t, b, 0])) - re), float(F(float(got[c, t, b, 1])) - im)
                err[c, t, b] = np.hypot(dr, di)
                S[c, t, b] = s
    return err, S


@pytest.mark.parametrize("kind", ["normal", "cancelling"])
@pytest.mark.parametrize("K", [33, 259])
@pytest.mark.parametrize("variant", VARIANTS, ids=[VID[v] for v in VARIANTS])
def test_rounding_bound(lib, variant, K, kind):
    rng = np.random.default_rng(2000 + 3 * K + variant)
    wide = np.finfo(np.longdouble).eps < 2.0 ** -60
    P, n_ch = 64, 2 if wide else 1
    T = 65 if variant == COOP else 2 * variant + 1
    if not wide:
        T = min(T, 9)
    ring = ring_min(K, T)
    head = ring - 2
    slots, n_slots, h_private = slot_table("private", n_ch)
    X, H = make_case(rng, P, n_ch, K, T, head, ring, slots, n_slots, h_rows_min(K), fill=0.0, normal=True)
    if kind == "cancelling":
        # H follows the rows block t* = T / 2 meets: even bins H ~ X (Re = sum a^2 - sum b^2, a small difference of two large
        # sums; the Gauss form also gets Im from three large sums), odd bins H ~ conj(X) (Im cancels)
        ts = T // 2
        for c in range(n_ch):
            hk = X[c, (head + ts - np.arange(K)) & (ring - 1)] * (1.0 + 1e-3 * rng.standard_normal((K, P, 2)))
            hk[:, 1::2, 1] *= -1.0
            H[c, :K] = hk
    got, used = run_mac(lib, X, H, slots, K, T, variant, head, h_private)
    assert used == (0 if variant == COOP else variant)
    assert np.isfinite(got).all()
    if wide:
        ref, S = reference(X, H, slots, K, T, head, np.longdouble)
        d = got.astype(np.longdouble) - ref
        err = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2).astype(np.float64)
        S = S.astype(np.float64)
    else:
        err, S = exact_rational_error(X, H, slots, K, T, head, got)
    u = 2.0 ** -53
    ratio = err / (u * S)
    c, t, b = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"variant {VID[variant]} K {K} {kind}: worst |Y - ref| / (u S) = {ratio.max():.3f} at channel {c} block {t} bin {b} "
          f"(bound {2 * K + 8}); reference {'long double' if wide else 'exact rationals'}")
    if kind == "cancelling":      # H does follow X at block t*: on the odd bins Re = sum a^2 + b^2 >= S / 2 up to the 1e-3 noise
        assert (got[:, T // 2, 1::2, 0] > 0.4 * S[:, T // 2, 1::2]).all()
    assert (err <= (2 * K + 8) * u * S).all(), (VID[variant], K, kind, float(ratio.max()), int(c), int(t), int(b))


# ------------------------------------------------------------------------------------------ c. one call equals two
@pytest.mark.parametrize("tile,T,T1", [(4, 9, 3), (8, 17, 5), (16, 33, 7), (32, 65, 11), (COOP, 129, 9), (0, 48, 47), (0, 65, 5)],
                         ids=["4", "8", "16", "32", "coop", "auto-47+1", "auto-5+60"])
def test_one_call_equals_two(lib, tile, T, T1):
    rng = np.random.default_rng(8000 + T)
    for K in (7, 33):
        ring = ring_min(K, T)
        head = ring - T1 - 1                          # the second call's head + t wraps
        slots, n_slots, h_private = slot_table("private", 3)
        X, H = make_case(rng, 64, 3, K, T, head, ring, slots, n_slots, h_rows_min(K))
        whole, v = run_mac(lib, X, H, slots, K, T, tile, head, h_private)
        first, v1 = run_mac(lib, X, H, slots, K, T1, tile, head, h_private)
        rest, v2 = run_mac(lib, X, H, slots, K, T - T1, tile, (head + T1) & (ring - 1), h_private)
        if (tile, T, T1) == (0, 48, 47):
            assert (v, v1, v2) == (0, 16, 4)          # the point: three different kernels, the same bits
        if (tile, T, T1) == (0, 65, 5):
            assert (v, v1, v2) == (0, 4, 0)
        two = np.concatenate([first, rest], axis=1)
        ref, _ = reference(X, H, slots, K, T, head, np.int64)
        assert np.array_equal(whole, ref.astype(np.float64)), (tile, K, "one call")
        assert np.array_equal(two, whole), (tile, K, int((two != whole).any(axis=-1).sum()))


# ---------------------------------------------------------------------------------------------- d. argument errors
# (the table and its caller: tests/mac_fft_calls.py, which tests/test_host_and_abi_cpu.py walks without a device)
@pytest.mark.parametrize("what", list(BAD_ARGS))
def test_argument_errors(lib, what):
    a = dict(GOOD, **BAD_ARGS[what])
    X, H, Y, used = mac_buffers(a)
    assert mac_call(lib, a, X, H, Y, used) == INVALID_ARG, what
    assert used.value == -99 and (Y == -7.0).all()                  # refused before anything ran
    # the call after it, with good arguments, succeeds and computes K = 5 ones times ones
    Xg, Hg = np.ones((2, 128, 64, 2)), np.ones((2, 48, 64, 2))
    assert mac_call(lib, GOOD, Xg, Hg, Y, used) == 0
    assert used.value == 4
    got = Y.reshape(-1)[:2 * 3 * 64 * 2].reshape(2, 3, 64, 2)
    assert (got[:, :, 1:, 0] == 0.0).all() and (got[:, :, 1:, 1] == 10.0).all() and (got[:, :, 0] == 5.0).all()


def test_null_pointers_are_refused(lib):
    X, H, Y, used = mac_buffers()
    for name in MAC_POINTERS:
        assert mac_call(lib, GOOD, X, H, Y, used, null=name) == INVALID_ARG
    assert mac_call(lib, GOOD, X, H, Y, used) == 0
