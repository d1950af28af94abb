"""cpq_ir_minimum_phase / _batch, cpq_ir_prepare_batch(CPQ_PHASE_MINIMUM) and cpq_diag_cfft on the device (minphase_kernels.hip).

Tolerance: the device is compared with the host path cpq_ir_convert_to_minimum_phase on the same input.  The yardstick d_ref is
computed here, on the CPU: d_ref = max |host - oracle.convert_to_minimum_phase(x)|, two CPU implementations of the same
mathematics with different FFTs.  Required: max |device - host| <= max(8 d_ref, 8 * 2^-52 * peak(host)); the factor 8 allows for
the device's log / exp / sincos differing from glibc's by an ulp or two on top of the reordered FFT, the floor covers the short
rows where d_ref is 0.  Every case prints d_ref and the device's difference.

Sizes: N_LDS = 4096 complex points, so rows up to 1024 samples run in k_minphase_small and longer ones through the column and
row passes; 1, 2, 3 (N = 4, 8, 16), 255 / 256 / 257 (N doubles), 1023 / 1024 / 1025 (the boundary), 4097 (N = 2^15: N1 != N2),
16385 (2^17), 48000 (2^18, the bench's size)."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

import convopeq_amd as amd
from convopeq_amd import _capi as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOG2_LDS = 12


@pytest.fixture(scope="module")
def O():
    spec = importlib.util.spec_from_file_location("ir_ingest_oracle", os.path.join(os.path.dirname(HERE), "oracle", "ir_ingest_oracle.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def same(got, want):
    return got is not None and got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def rows_of(n, seed, kinds="abc"):
    """(a) uniform noise in +-0.5, (b) the same noise under exp(-6 t / n) with x[0] += 1, (c) noise under a two-sided decay about n / 3"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    out = []
    for k in kinds:
        x = rng.uniform(-0.5, 0.5, n)
        if k == "b":
            x = x * np.exp(-6.0 * t / n)
            x[0] += 1.0
        elif k == "c":
            x = x * np.exp(-np.abs(t - n // 3) * 8.0 / n)
        out.append(x)
    return np.stack(out)


_REF = {}


def reference(O, x):
    """(host path, d_ref per row), computed once per input"""
    key = (x.shape, x.tobytes()[:256], float(x.sum()))
    if key not in _REF:
        host = amd.ir_convert_to_minimum_phase(x)
        orc = O.convert_to_minimum_phase(x)
        _REF[key] = (host, np.abs(host - orc).max(axis=1))
    return _REF[key]


def within(dev, host, d_ref, label):
    worst = 0.0
    for r in range(host.shape[0]):
        diff = float(np.abs(dev[r] - host[r]).max())
        limit = max(8.0 * float(d_ref[r]), 8.0 * 2.0 ** -52 * float(np.abs(host[r]).max()))
        print(f"{label} row {r}: d_ref {d_ref[r]:.3e}  device - host {diff:.3e}  limit {limit:.3e}  ratio {diff / limit:.3f}")
        worst = max(worst, diff / limit)
    return worst


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4097, 16385])
def test_device_against_host_path(O, n):
    x = rows_of(n, 1000 + n)
    host, d_ref = reference(O, x)
    dev = amd.ir_minimum_phase(x)
    assert dev.shape == x.shape
    worst = within(dev, host, d_ref, f"n {n}")
    print(f"n {n}: worst ratio {worst:.3f}")
    assert worst <= 1.0
    assert not np.any((dev != 0.0) & (np.abs(dev) < 1e-18))


def test_one_row_of_the_bench_size(O):
    x = rows_of(48000, 48000, "a")
    host, d_ref = reference(O, x)
    dev = amd.ir_minimum_phase(x)
    worst = within(dev, host, d_ref, "n 48000")
    print(f"n 48000: worst ratio {worst:.3f}")
    assert worst <= 1.0
    assert K.load().cpq_ir_minimum_phase_last_kernel_ms() > 0.0


def batch_irs():
    """mono and stereo IRs of five lengths across three FFT sizes: N = 4096 (small kernel), 8192 and 2^15 (column and row passes)"""
    return [rows_of(1000, 1, "ab"), rows_of(2000, 2, "c"), rows_of(700, 3, "b"), rows_of(1500, 4, "ac"), rows_of(4097, 5, "b"),
            rows_of(1000, 6, "c"), rows_of(8000, 7, "ab")]


def test_batch_is_independent_of_its_company_and_of_the_workspace():
    lib = K.load()
    irs = batch_irs()
    got, status = amd.ir_minimum_phase_batch(irs)
    assert status == [K.CPQ_OK] * len(irs) and lib.cpq_ir_minimum_phase_last_kernel_ms() > 0.0
    for ir, g in zip(irs, got):
        assert same(g, amd.ir_minimum_phase(ir))
    # just over one row's need at the largest FFT size (16 n + 16 N + 32 bytes): one row per chunk there, a few rows per chunk in the other groups
    tight = 16 * 8000 + 16 * 32768 + 32 + 8
    again, status = amd.ir_minimum_phase_batch(irs, workspace_bytes=tight)
    assert status == [K.CPQ_OK] * len(irs) and all(same(a, g) for a, g in zip(again, got))
    again, _ = amd.ir_minimum_phase_batch(irs[::-1])
    assert all(same(a, g) for a, g in zip(again[::-1], got))
    again, _ = amd.ir_minimum_phase_batch(irs)
    assert all(same(a, g) for a, g in zip(again, got))
    with pytest.raises(amd.CpqError) as e:
        amd.ir_minimum_phase_batch(irs, workspace_bytes=tight - 9)
    assert e.value.status == K.CPQ_ERR_INVALID_ARG and str(tight - 8) in str(e.value)
    # a call that launches nothing
    assert amd.ir_minimum_phase_batch([]) == ([], []) and lib.cpq_ir_minimum_phase_last_kernel_ms() < 0.0


def test_statuses_are_per_ir():
    irs = batch_irs()[:5]
    solo = [amd.ir_minimum_phase(ir) for ir in irs]
    poisoned = [ir.copy() for ir in irs]
    poisoned[1][0, 77] = np.nan             # four-step path
    poisoned[2][0, 5] = np.nan              # small kernel
    too_long = np.zeros((1, 2097153))
    too_long[0, 0] = 1.0
    got, status = amd.ir_minimum_phase_batch(poisoned + [too_long])
    U = K.CPQ_ERR_UNSUPPORTED
    assert status == [0, U, U, 0, 0, U]
    assert got[1] is None and got[2] is None and got[5] is None
    for i in (0, 3, 4):
        assert same(got[i], solo[i])
        assert not np.any((got[i] != 0.0) & (np.abs(got[i]) < 1e-18)) and np.all(np.isfinite(got[i]))
    # a NaN in one channel refuses the whole IR
    stereo = irs[0].copy()
    stereo[1, 3] = np.inf
    got, status = amd.ir_minimum_phase_batch([stereo, irs[3]])
    assert status == [U, 0] and got[0] is None and same(got[1], solo[3])
    with pytest.raises(amd.CpqError) as e:
        amd.ir_minimum_phase(stereo)
    assert e.value.status == U


def test_properties():
    """the bounds of tests/test_ir_ingest_cpu.py::test_minimum_phase_conversion on its input (the sample IR conditioned to 12000
    samples: 65536-point transforms), and on both paths a minimum-phase sequence that comes back from behind a delay"""
    ir, rate = amd.ir_load_wav(os.path.join(HERE, "golden", "impulse_room_correction_hpf_lpf.wav"))
    x = amd.ir_prepare(ir, rate, 48000.0, 0.25)["ir"]
    n = x.shape[1]
    got = amd.ir_minimum_phase(x)
    for ch in range(2):
        a, b = np.abs(np.fft.rfft(x[ch], 4 * n)), np.abs(np.fft.rfft(got[ch], 4 * n))
        strong = a > 1e-3 * a.max()
        assert np.abs(b[strong] / a[strong] - 1.0).max() < 1e-3
        ea, eb = np.cumsum(x[ch] ** 2), np.cumsum(got[ch] ** 2)
        assert np.all(eb[:n // 2] >= ea[:n // 2] * (1 - 1e-9) - 1e-15)          # energy arrives no later than in any other phase
        t = np.arange(n)
        assert (t * got[ch] ** 2).sum() / (got[ch] ** 2).sum() <= (t * x[ch] ** 2).sum() / (x[ch] ** 2).sum()
    for n in (1000, 2000):                  # small kernel, column and row passes
        t = np.arange(n, dtype=np.float64)
        h = 0.5 * 0.9 ** t - 0.3 * 0.8 ** t
        delayed = np.zeros((1, n))
        delayed[0, 5:] = h[:n - 5]
        got = amd.ir_minimum_phase(delayed)
        assert np.abs(got[0] - h).max() < 1e-9
        a, b = np.abs(np.fft.rfft(delayed[0], 4 * n)), np.abs(np.fft.rfft(got[0], 4 * n))
        assert np.abs(b / a - 1.0).max() < 1e-3
    for n in (1024, 4096):                  # a decaying exponential is minimum phase already
        e = (0.5 * 0.99 ** np.arange(n, dtype=np.float64))[None, :]
        assert np.abs(amd.ir_minimum_phase(e) - e).max() < 1e-9


def cfft(x, inverse):
    rows, n = x.shape
    buf = np.ascontiguousarray(x, dtype=np.complex128)
    out = np.empty_like(buf)
    rc = K.load().cpq_diag_cfft(buf.view(np.float64).ctypes.data_as(K.c_double_p), int(math.log2(n)), rows, int(inverse),
                                out.view(np.float64).ctypes.data_as(K.c_double_p))
    assert rc == K.CPQ_OK
    return out


@pytest.mark.parametrize("log2n", [2, 3, LOG2_LDS, LOG2_LDS + 1, 15, 17])
def test_cfft_against_numpy(log2n):
    """relative L2 error <= 8 log2(N) 2^-53: the worst-case order of Higham, Accuracy and Stability, Thm 24.2, for accurately
    computed twiddles, doubled because numpy's own error is in the comparison; a unit impulse against the exact roots at 4 * 2^-52"""
    n = 1 << log2n
    rng = np.random.default_rng(log2n)
    x = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    bound = 8 * log2n * 2.0 ** -53
    for inverse in (False, True):
        want = np.fft.ifft(x, axis=1) if inverse else np.fft.fft(x, axis=1)
        got = cfft(x, inverse)
        for r in range(2):
            rel = float(np.linalg.norm(got[r] - want[r]) / np.linalg.norm(want[r]))
            print(f"log2n {log2n} inverse {inverse} row {r}: rel L2 {rel:.3e}, bound {bound:.3e}")
            assert rel <= bound
    # impulses at 1 and at an odd index near N / 3: X[k] = w^(n0 k), exact from the angle reduced to the first octant in integers
    n0s = [1, (n // 3) | 1]
    e = np.zeros((2, n), dtype=np.complex128)
    for r, n0 in enumerate(n0s):
        e[r, n0] = 1.0
    got = cfft(e, False)
    for r, n0 in enumerate(n0s):
        m = (np.arange(n, dtype=np.int64) * n0) % n
        octant, rem = np.divmod(m * 8, n)           # angle = (octant + rem / n) * pi / 4
        frac = rem / n
        theta = np.where(octant % 2 == 0, frac, 1.0 - frac) * (np.pi / 4)
        c, s = np.cos(theta), np.sin(theta)
        c, s = np.where(octant % 2 == 0, c, s), np.where(octant % 2 == 0, s, c)         # angle within the quadrant
        quad = octant // 2
        re = np.select([quad == 0, quad == 1, quad == 2], [c, -s, -c], s)
        im = -np.select([quad == 0, quad == 1, quad == 2], [s, c, -s], -c)
        err = max(float(np.abs(got[r].real - re).max()), float(np.abs(got[r].imag - im).max()))
        print(f"log2n {log2n} impulse at {n0}: {err / 2.0 ** -52:.2f} * 2^-52")
        assert err <= 4 * 2.0 ** -52


def test_prepare_batch_minimum_phase_and_a_stream(O, oracle):
    lib = K.load()
    B = 512
    ir, rate = amd.ir_load_wav(os.path.join(HERE, "golden", "impulse_room_correction_hpf_lpf.wav"))
    assert rate == 48000.0
    head = np.stack([ir[0, :4096], ir[-1, :4096]])
    irs = [head, rows_of(3000, 31, "b"), rows_of(900, 32, "bc")]
    secs = 0.05                                        # 2400 samples: four-step transforms of 16384 points
    batch = amd.ir_prepare_batch([(x, 48000.0) for x in irs], 48000.0, secs, phase_mode=K.CPQ_PHASE_MINIMUM)
    assert lib.cpq_ir_minimum_phase_last_kernel_ms() > 0.0
    for x, got in zip(irs, batch):
        want = amd.ir_prepare(x, 48000.0, 48000.0, secs, phase_mode=K.CPQ_PHASE_MINIMUM)
        trimmed = amd.ir_prepare(x, 48000.0, 48000.0, secs)["ir"]
        host, d_ref = reference(O, trimmed)
        assert np.array_equal(host, want["ir"])        # the host transform of the trimmed IR is what cpq_ir_prepare kept
        assert got["ir"].shape == want["ir"].shape and within(got["ir"], want["ir"], d_ref, "prepare") <= 1.0
        assert abs(got["scale"]["scale_factor"] / want["scale"]["scale_factor"] - 1.0) <= 1e-12
        assert got["ir_peak_latency"] == want["ir_peak_latency"]
    # the first IR on a one-stream engine against the oracle's Nuc loaded with the same device-made IR
    taps, scale = batch[0]["ir"], batch[0]["scale"]["scale_factor"]
    x = np.stack([oracle.gen_pcm(4 * B, stream=0, channel=ch) for ch in range(2)])
    ref = np.empty_like(x)
    for ch in range(2):
        nuc = oracle.Nuc()
        assert nuc.set_impulse(taps[ch] * scale, B)
        ref[ch] = nuc.run(x[ch], B)
        nuc.close()
    eng = amd.BatchedEngine(1, block_size=B, max_ir_len=taps.shape[1], max_blocks_per_call=1)
    eng.prepare_to_play(48000.0, B)
    eng.set_impulse(0, taps[0] * scale, taps[1] * scale)
    y = np.concatenate([eng.conv_process(x[:, i * B:(i + 1) * B]) for i in range(4)], axis=1)
    eng.close()
    err = float(np.sqrt(np.mean(np.square(y - ref))))
    print("device-made minimum-phase IR on a stream: rms err", err, "signal rms", float(np.sqrt(np.mean(np.square(ref)))))
    assert np.any(ref) and err <= 1e-13
