"""The 128-row workgroup of the cooperative FDL MAC kernel (k_fdl_mac_wg<16, ...>, convopeq_amd/csrc/mac_kernels.hip) through
cpq_diag_fdl_mac with tile = ROWS128, bit for bit against the int64 model of tests/test_gpu_fdl_mac.py (imported, with its case
builder: small-integer spectra, 2^40 in every ring slot, IR row and IR slot the call must not consume; the diagnostic
pre-fills the device destination with 0xFF bytes, so an element no kernel stores is a NaN and differs).

What is new in that geometry, and the case that meets it:
  * the staging map -- waves 0-7 fetch the FDL row, waves 8-15 the IR row of the next chunk, where the 64-row workgroup has
    every wave fetch both: every case with K > 8 (one staged chunk and more);
  * the skips of the last two chunks: rem = K - 8 (chunks - 1) = 1 (K = 1, 9, 17, 33), 7 (K = 7), 8 (K = 8, 16, 40), with no
    chunk before the last (K <= 8), one (K = 9, 16) and several; a row skipped that a step needs leaves a stale or zero
    value in the ring or the stage, a step run past K consumes poison: both move the result;
  * the double-buffered IR stage: K = 17, 33, 40 use each stage twice and more;
  * the 17-block ring: K = 40 with T = 256 walks 5 chunks over 16 waves in two groups;
  * groups: T = 128 (one), 256 (two: the XCD remap of logical ids, base = head + 128 grp), 136 and 200 (a last group of 8 and
    72 rows: waves 1-15 and 9-15 of it have no output row and only feed the ring);
  * P = 64 (one column) and 128 (two), 3 channels of which two share an IR slot, slot 0 named by nobody;
  * head = ring - T / 2 (head + t wraps inside the call) and head = K / 2 (head - k wraps inside the history rows);
  * element 0, the packed (DC, Nyquist) pair, compared as (M1, M2) on its own;
  * the same inputs through the 64-row and the 128-row workgroup: equal bytes.
Equality is the assertion throughout (the bound on the intermediates is that of tests/test_gpu_fdl_mac.py: below 2^31)."""
import numpy as np
import pytest

from mac_rows128_calls import ROWS128, ROWS128_USED
from test_gpu_fdl_mac import COOP, h_rows_min, make_case, reference, ring_min, run_mac

pytestmark = pytest.mark.gpu

K_VALUES = [1, 7, 8, 9, 16, 17, 33, 40]
T_VALUES = [128, 136, 200, 256]
N_CH = 3
SLOTS = np.array([1, 2, 1], dtype=np.int32)       # channels 0 and 2 share slot 1; slot 0 is poison
N_SLOTS = 3


@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need a gfx950 device")
    from convopeq_amd import _capi
    return _capi.load()


def heads(K, T, ring):
    return sorted({ring - T // 2, max(1, K // 2)})


def case(rng, P, K, T, head):
    ring = ring_min(K, T)
    X, H = make_case(rng, P, N_CH, K, T, head, ring, SLOTS, N_SLOTS, h_rows_min(K))
    ref, _ = reference(X, H, SLOTS, K, T, head, np.int64)
    assert np.abs(ref).max() < 2 ** 31
    return X, H, ref.astype(np.float64)


def describe(got, ref):
    bad = ~(got == ref)
    c, t, b, part = np.argwhere(bad)[0]
    return (f"{int(bad.any(axis=-1).sum())} of {bad[..., 0].size} elements differ, first at channel {c} row {t} bin {b} "
            f"({'re' if part == 0 else 'im'}): got {got[c, t, b, part]!r}, expected {ref[c, t, b, part]!r}")


@pytest.mark.parametrize("T", T_VALUES)
@pytest.mark.parametrize("K", K_VALUES)
def test_rows128_exact(lib, K, T):
    rng = np.random.default_rng(128000 + 1000 * K + T)
    for P in (64, 128):
        for head in heads(K, T, ring_min(K, T)):
            X, H, ref = case(rng, P, K, T, head)
            got, used = run_mac(lib, X, H, SLOTS, K, T, ROWS128, head, 0)
            assert used == ROWS128_USED
            # element 0 packs (DC, Nyquist): M1 = sum Re X Re H and M2 = sum Im X Im H, not their difference
            assert np.array_equal(got[:, :, 0, :], ref[:, :, 0, :]), (P, K, T, head, "bin 0")
            assert np.array_equal(got, ref), (P, K, T, head, describe(got, ref))


@pytest.mark.parametrize("T", [128, 200])
@pytest.mark.parametrize("K", [9, 33])
def test_rows128_equals_rows64(lib, K, T):
    rng = np.random.default_rng(64128 + 10 * K + T)
    P, head = 128, ring_min(K, T) - T // 2
    X, H, ref = case(rng, P, K, T, head)
    a, va = run_mac(lib, X, H, SLOTS, K, T, COOP, head, 0)
    b, vb = run_mac(lib, X, H, SLOTS, K, T, ROWS128, head, 0)
    assert (va, vb) == (0, ROWS128_USED)
    assert a.tobytes() == b.tobytes() == ref.tobytes()


@pytest.mark.parametrize("T", [128, 200, 256])
def test_automatic_rule_keeps_the_64_row_workgroup(lib, T):
    """the 128-row workgroup measured slower at the bench shape (RESULTS.md): tile = 0 does not choose it at any T"""
    rng = np.random.default_rng(900 + T)
    K, head = 9, 3
    X, H, ref = case(rng, 64, K, T, head)
    got, used = run_mac(lib, X, H, SLOTS, K, T, 0, head, 0)
    assert used == 0
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("T", [1, 9, 65])
def test_rows128_forced_below_one_group(lib, T):
    """forceable at any T: one group of which 15, 14 and 7 waves have no output row"""
    rng = np.random.default_rng(700 + T)
    for K in (7, 33):
        head = max(1, K // 2)
        X, H, ref = case(rng, 64, K, T, head)
        got, used = run_mac(lib, X, H, SLOTS, K, T, ROWS128, head, 0)
        assert used == ROWS128_USED
        assert np.array_equal(got, ref), (K, T, describe(got, ref))
