"""minphase_kernels.hip where tests/test_gpu_ir_minphase.py does not go: the value edges of the pointwise stages (the 1e-300 floor,
the +-50 clamp on either part, the 1e-18 flush, silence), rows of N = 2^19 ... 2^23 (N1 and N2 of 1024 and 2048, N2 = 4096, the
4-column tile of N1 = 2048, the top of the two-level twiddle table), cpq_diag_cfft at every length 2^1 ... 2^23 that file leaves
out, and a chunk boundary (kMinphaseMaxChunkRows = 65536 rows) inside one IR.

Tolerance, as in that file: the device is compared with the host path cpq_ir_convert_to_minimum_phase, per row within
limit = max(8 d_ref, 8 * 2^-52 * peak(host)), d_ref = max |host - oracle| (tests/test_minphase_edges_cpu.py requires
d_ref <= 1e-10 peak of every input here).  Pointwise, so that the flush may fall either way on a value near 1e-18: element i
passes if |device - host| <= limit, or if one of the two is exactly 0 and the other is below 1e-18 + limit; d_ref is taken under
the same rule (minphase_edge_inputs.yardstick).  Every case prints d_ref, the difference and the ratio.

Measured on an MI355X (RESULTS.md): worst ratio 0.21 over the value edges (flush at n = 1025), 0.05 ... 0.10 at the large sizes;
cfft relative L2 0 ... 4.8e-16 against bounds of 8.9e-16 ... 2.0e-14; the impulse at most 4 * 2^-52 (2^20 ... 2^22).  Value-only
mutants of the kernels and what caught them: the floor at 1e-200 -- comb at all four sizes; the clamp at +-60 -- huge and comb;
no flush -- tiny, silence, half_silent, flush and late_impulse; the top half of the twiddle table's upper level aliased onto the
lower (N = 2^23) -- test_large_sizes[2097152] and test_cfft_against_numpy[23]."""
import importlib.util
import math
import os
import time

import numpy as np
import pytest

import convopeq_amd as amd
import minphase_edge_inputs as E
from convopeq_amd import _capi as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def O():
    spec = importlib.util.spec_from_file_location("ir_ingest_oracle", os.path.join(os.path.dirname(HERE), "oracle", "ir_ingest_oracle.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def same(got, want):
    return got is not None and got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def within(dev, host, d_ref, label):
    worst = 0.0
    for r in range(host.shape[0]):
        diff, limit, ratio = E.worst_ratio(dev[r], host[r], float(d_ref[r]))
        print(f"{label} row {r}: d_ref {d_ref[r]:.3e}  device - host {diff:.3e}  limit {limit:.3e}  ratio {ratio:.3f}")
        worst = max(worst, ratio) if ratio == ratio else float("nan")
    return worst


def no_denormal_leftovers(y):
    return not np.any((y != 0.0) & (np.abs(y) < E.FLUSH))


@pytest.mark.parametrize("name,n", E.edge_cases())
def test_value_edges(O, name, n):
    """n = 700: k_minphase_small at N = 4096; n = 2000: the column and row passes at N = 8192; 1024 | 1025: the last row of the
    one and the first of the other"""
    x, host, orc, d_ref = E.reference((name, n), E.INPUTS[name](n), amd.ir_convert_to_minimum_phase, O.convert_to_minimum_phase)
    got, status = amd.ir_minimum_phase_batch([x])
    assert status == [K.CPQ_OK]
    dev = got[0]
    assert dev.shape == x.shape
    worst = within(dev, host, d_ref, f"{name} n {n}")
    print(f"{name} n {n}: worst ratio {worst:.3f}")
    assert worst <= 1.0
    assert np.all(np.isfinite(dev)) and no_denormal_leftovers(dev)
    if name in ("tiny", "silence"):
        assert not dev.any()
    elif name == "half_silent":
        assert dev[0].any() and not dev[1].any()
    elif name in ("flush", "late_impulse"):
        assert np.any(dev == 0.0) and np.any(dev != 0.0)
        print(f"{name} n {n}: zeros device {int((dev == 0.0).sum())} host {int((host == 0.0).sum())}")
    elif name == "huge":
        peak_dev, peak_host = float(np.abs(dev).max()), float(np.abs(host).max())
        assert peak_host > 1e18 and abs(peak_dev - peak_host) <= E.limit_of(host[0], float(d_ref[0]))


@pytest.mark.parametrize("n", E.LARGE_SIZES)
def test_large_sizes(O, n):
    t0 = time.perf_counter()
    x, host, orc, d_ref = E.reference(("large", n), E.large_row(n), amd.ir_convert_to_minimum_phase, O.convert_to_minimum_phase)
    t1 = time.perf_counter()
    dev = amd.ir_minimum_phase(x)
    t2 = time.perf_counter()
    assert dev.shape == x.shape
    worst = within(dev, host, d_ref, f"n {n}")
    print(f"n {n} (N = 2^{int(math.log2(E.fft_size(n)))}): worst ratio {worst:.3f}  wall: references {t1 - t0:.2f} s (0 when shared), "
          f"device call {t2 - t1:.2f} s, compare {time.perf_counter() - t2:.2f} s")
    assert worst <= 1.0
    assert np.all(np.isfinite(dev)) and no_denormal_leftovers(dev)
    assert K.load().cpq_ir_minimum_phase_last_kernel_ms() > 0.0


def cfft(x, inverse):
    rows, n = x.shape
    buf = np.ascontiguousarray(x, dtype=np.complex128)
    out = np.empty_like(buf)
    rc = K.load().cpq_diag_cfft(buf.view(np.float64).ctypes.data_as(K.c_double_p), int(math.log2(n)), rows, int(inverse),
                                out.view(np.float64).ctypes.data_as(K.c_double_p))
    assert rc == K.CPQ_OK
    return out


def exact_roots(n, n0):
    """exp(-2 pi i n0 k / n) for k = 0 ... n - 1, from the angle reduced to the first octant in integers (as in
    tests/test_gpu_ir_minphase.py)"""
    m = (np.arange(n, dtype=np.int64) * n0) % n
    octant, rem = np.divmod(m * 8, n)
    frac = rem / n
    theta = np.where(octant % 2 == 0, frac, 1.0 - frac) * (np.pi / 4)
    c, s = np.cos(theta), np.sin(theta)
    c, s = np.where(octant % 2 == 0, c, s), np.where(octant % 2 == 0, s, c)
    quad = octant // 2
    re = np.select([quad == 0, quad == 1, quad == 2], [c, -s, -c], s)
    im = -np.select([quad == 0, quad == 1, quad == 2], [s, c, -s], -c)
    return re, im


# every length of cpq_diag_cfft that tests/test_gpu_ir_minphase.py leaves out (it runs 2, 3, 12, 13, 15, 17): both parities of the
# closing and opening radix-2 stage in the LDS core, and N1 | N2 up to 2048 | 4096 on the column and row passes
@pytest.mark.parametrize("log2n", [1, 4, 5, 6, 7, 8, 9, 10, 11, 14, 16, 18, 19, 20, 21, 22, 23])
def test_cfft_against_numpy(log2n):
    """relative L2 error <= 8 log2(N) 2^-53 (Higham, Accuracy and Stability, Thm 24.2, doubled because numpy's own error is in the
    comparison), forward and inverse; forward then inverse against the input at twice that.  The unit impulse against the exact
    roots is printed, not asserted: its 4 * 2^-52 was measured up to 2^17 only and the twiddle products grow in number with N."""
    t0 = time.perf_counter()
    n = 1 << log2n
    rows = 2 if log2n <= 22 else 1
    rng = np.random.default_rng(100 + log2n)
    x = rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))
    bound = 8 * log2n * 2.0 ** -53
    fwd = None
    for inverse in (False, True):
        want = np.fft.ifft(x, axis=1) if inverse else np.fft.fft(x, axis=1)
        got = cfft(x, inverse)
        if not inverse:
            fwd = got
        for r in range(rows):
            rel = float(np.linalg.norm(got[r] - want[r]) / np.linalg.norm(want[r]))
            print(f"log2n {log2n} inverse {inverse} row {r}: rel L2 {rel:.3e}, bound {bound:.3e}")
            assert rel <= bound
    back = cfft(fwd, True)
    for r in range(rows):
        rel = float(np.linalg.norm(back[r] - x[r]) / np.linalg.norm(x[r]))
        print(f"log2n {log2n} forward then inverse row {r}: rel L2 {rel:.3e}, bound {2 * bound:.3e}")
        assert rel <= 2 * bound
    if log2n >= 18:
        n0s = [1, (n // 3) | 1][:rows]
        e = np.zeros((rows, n), dtype=np.complex128)
        for r, n0 in enumerate(n0s):
            e[r, n0] = 1.0
        got = cfft(e, False)
        for r, n0 in enumerate(n0s):
            re, im = exact_roots(n, n0)
            err = max(float(np.abs(got[r].real - re).max()), float(np.abs(got[r].imag - im).max()))
            print(f"log2n {log2n} impulse at {n0}: {err / 2.0 ** -52:.2f} * 2^-52")
    print(f"log2n {log2n}: wall {time.perf_counter() - t0:.2f} s")


WIDE = 65537                # one row more than kMinphaseMaxChunkRows
PATTERNS = np.array([[1.0, 0.5, -0.25], [0.3, -0.7, 0.2], [0.0, 1.0, 0.0], [-0.9, 0.1, 0.4], [1e-3, 2e-3, -3e-3], [0.25, 0.25, 0.25],
                     [0.6, -0.1, 0.05]])


def wide_batch():
    """an IR of 65537 channels x 3 samples (N = 16; channel c holds pattern c mod 7) and a stereo IR of 3 samples: 65539 rows of
    one group, so the first chunk ends inside the first IR, on its channel 65535"""
    return [PATTERNS[np.arange(WIDE) % len(PATTERNS)].copy(), np.array([[0.8, -0.3, 0.1], [0.2, 0.9, -0.4]])]


def test_chunk_boundary_inside_an_ir():
    lib = K.load()
    irs = wide_batch()
    got, status = amd.ir_minimum_phase_batch(irs)
    assert status == [K.CPQ_OK, K.CPQ_OK] and lib.cpq_ir_minimum_phase_last_kernel_ms() > 0.0
    assert got[0].shape == (WIDE, 3) and got[1].shape == (2, 3)
    solo = amd.ir_minimum_phase(PATTERNS)                          # each pattern converted in a call of 7 rows
    for p in range(len(PATTERNS)):
        assert same(solo[p:p + 1], amd.ir_minimum_phase(PATTERNS[p:p + 1]))
    assert np.all(np.isfinite(solo)) and solo.any()
    # every row against the row of the same input converted alone: rows 0, 65535 and 65536 are among them
    assert same(got[0], solo[np.arange(WIDE) % len(PATTERNS)])
    for row in (0, 1, 65534, 65535, 65536):
        assert same(got[0][row:row + 1], amd.ir_minimum_phase(irs[0][row:row + 1]))
    stereo = amd.ir_minimum_phase(irs[1])
    assert same(got[1], stereo)
    # 80 bytes a row (16 n + 32): 1000 rows a chunk, 66 chunks, the stereo IR split from nothing it shares a chunk with
    capped, status = amd.ir_minimum_phase_batch(irs, workspace_bytes=80 * 1000)
    assert status == [K.CPQ_OK, K.CPQ_OK] and same(capped[0], got[0]) and same(capped[1], got[1])
    # a NaN in the one channel of the first IR that lies in the second chunk: the flag is raised in a later chunk than the one
    # that holds the IR's first row, and refuses the whole IR
    U = K.CPQ_ERR_UNSUPPORTED
    poisoned = [irs[0].copy(), irs[1]]
    poisoned[0][65536, 1] = np.nan
    for cap in (0, 80 * 1000):
        bad, status = amd.ir_minimum_phase_batch(poisoned, workspace_bytes=cap)
        assert status == [U, K.CPQ_OK] and bad[0] is None and same(bad[1], stereo)
