"""CPU tests of the output stage's host side: cpq_out_design against tests/out_model.py, the limiter model's knee, attack, release
and split invariance, the arithmetic of the time-parallel DC kernel emulated lane for lane, and out_design.cpp under the
address and undefined-behaviour sanitizers as a program of its own.

Release.  In fp64 the reference's release step env = 1 + (env - 1) * releaseCoeff does not come back to 1.0 after an attack: it
stalls at a fixed point a few hundred ulps below it (8 kHz: 0.9999999999999556, reached 24066 samples after an attack to
threshold / 2; 48 kHz: 0.9999999999997335 after 135800) and stays there bit for bit.  The kernel's streaming pass rests on
exactly that: an envelope that is a fixed point of the release step, 1.0 included, with no desired gain below it does not move.

DC scan bar.  The scan reassociates the one-pole recurrences, so it may stand a small multiple of the sequential fp64 form's own
distance from a long-double run away.  Measured here over the signals below (largest |y - long double| over a run, relative to
that of the sequential fp64 form): 0.16 - 1.00 x.  The bar is the 8 x the meter tests use; the GPU tests hold the kernel to it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import out_model as M
from out_edge_inputs import scan_dc, scan_section, scan_tables  # noqa: F401  (the kernel's fast path, lane by lane)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LD = np.longdouble
DC_BAR = 8.0


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


# ---------------------------------------------------------------------------------------------------------------- design
@pytest.mark.parametrize("rate", (44100.0, 48000.0, 96000.0, 8000.0))
def test_design_matches_model(amd, rate):
    alpha, rel = amd.out_design(rate)
    ma, mr = M.design(rate)
    assert list(alpha) == ma and rel == mr
    assert 0.0 < alpha[0] < alpha[1] < 1.0 and abs(alpha[0] / (2 * np.pi * 2.7 / rate) - 1) < 2e-3 and abs(alpha[1] / alpha[0] - 11 / 9) < 1e-3


def test_design_fallbacks_and_binding(amd):
    from convopeq_amd import _capi as K
    for bad in (0.0, -48000.0, float("nan"), float("inf"), float("-inf")):
        alpha, rel = amd.out_design(bad)
        assert list(alpha) == [1.0e-6, 1.0e-6] == M.design(bad)[0]
        assert rel == M.design(bad)[1] == (1.0 if bad == float("inf") else 0.0)
    lib = K.load()
    r = C.c_double()
    assert lib.cpq_out_design(48000.0, None, C.byref(r)) == K.CPQ_ERR_INVALID_ARG
    assert K.KERNEL_IDS["k_out"] == 11 and lib.cpq_kernel_name(11) == b"k_out" and lib.cpq_abi_version() == 2
    assert (K.CPQ_OUT_DC_BLOCK, K.CPQ_OUT_HEADROOM, K.CPQ_OUT_LIMITER, K.CPQ_OUT_CLAMP, K.CPQ_OUT_ALL) == (
        M.DC_BLOCK, M.HEADROOM, M.LIMITER, M.CLAMP, M.ALL) == (1, 2, 4, 8, 15)
    assert lib.cpq_engine_set_output_stage(None, 0) == K.CPQ_ERR_INVALID_ARG and lib.cpq_out_reset(None) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_out_process(None, None, None, 64) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_out_read_envelope(None, 0, C.byref(r)) == K.CPQ_ERR_INVALID_ARG


# --------------------------------------------------------------------------------------------------------------- limiter
def test_knee_is_continuous_and_never_below_one():
    up = lambda v: np.nextafter(v, 2.0)
    g = lambda p: float(M.desired_gain(np.array([p]), np.array([0.0]))[0])
    assert g(0.0) == 1.0 and g(M.CLIP_START) == 1.0 and abs(g(up(M.CLIP_START)) - 1.0) < 1e-15
    assert g(M.THRESHOLD) == 1.0 and abs(g(up(M.THRESHOLD)) - 1.0) < 2e-16 and g(up(M.THRESHOLD)) < 1.0
    # to the letter: inside the knee peak <= threshold, so threshold / peak >= 1 and the "reduction" is a gain >= 1, which the
    # envelope (never above 1) never takes: the limiter acts above the threshold only
    p = np.linspace(M.CLIP_START, M.THRESHOLD, 1001)
    d = M.desired_gain(p, -p)
    assert d.min() >= 1.0 and 1.005 < d.max() < 1.007
    assert g(2.0) == M.THRESHOLD / 2.0 and g(float("nan")) == 1.0 and g(float("inf")) == 0.0
    assert float(M.desired_gain(np.array([0.1]), np.array([-3.0]))[0]) == M.THRESHOLD / 3.0       # the larger channel decides


def test_attack_is_immediate_and_release_stalls_at_a_fixed_point():
    _, rel = M.design(8000.0)
    x = np.zeros((2, 40000))
    x[0, 0] = 2.0
    st = M.OutStage(8000.0, 1)
    y = st.process(x, 512, M.LIMITER)
    assert y[0, 0] == 2.0 * (M.THRESHOLD / 2.0)
    g, _ = M.envelope_run(M.desired_gain(x[0], x[1]), 1.0, rel)
    assert g[0] == M.THRESHOLD / 2.0 and np.all(np.diff(g) >= 0.0)
    stall = int(np.argmax(g == g[-1]))
    print(f"8 kHz: release stalls after {stall} samples at {g[-1]!r}")
    assert 20000 < stall < 30000 and g[-1] < 1.0 and 1.0 - g[-1] < 1e-12 and st.env[0] == g[-1]
    assert 1.0 + (g[-1] - 1.0) * rel == g[-1]                       # a fixed point of the release step ...
    g2, e2 = M.envelope_run(np.ones(64), g[-1], rel)
    assert np.all(g2 == g[-1]) and e2 == g[-1]                      # ... so a quiet group leaves it as it is, bit for bit
    g3, e3 = M.envelope_run(np.full(64, 1.02), 1.0, rel)            # and so is 1.0, the envelope of a stream that never limited
    assert np.all(g3 == 1.0) and e3 == 1.0
    for rate in (44100.0, 48000.0, 96000.0):                        # never back to 1.0 at any rate
        _, r = M.design(rate)
        e = 1.0 - 2.0 ** -40
        for _ in range(200000):
            e = 1.0 + (e - 1.0) * r
        assert e < 1.0 and 1.0 + (e - 1.0) * r == e


@pytest.mark.parametrize("flags", (M.ALL, M.HEADROOM | M.LIMITER | M.CLAMP))
def test_splitting_the_signal_changes_nothing(flags):
    rng = np.random.default_rng(5)
    n = 3000
    x = rng.standard_normal((2, n)) * np.repeat(rng.uniform(0.1, 1.6, n // 100), 100) + 0.2
    ref = M.OutStage(48000.0, 1)
    y = ref.process(x, n, flags)
    assert np.abs(y).max() <= M.H and ref.env[0] < 1.0
    for cb in (64, 441, 512):
        st = M.OutStage(48000.0, 1)
        assert np.array_equal(st.process(x, cb, flags), y) and st.env == ref.env and st.dc == ref.dc
        st = M.OutStage(48000.0, 1)                                 # several calls
        parts = [st.process(x[:, a:b], cb, flags) for a, b in ((0, 1), (1, 1000), (1000, 1441), (1441, n))]
        assert np.array_equal(np.concatenate(parts, axis=1), y) and st.env == ref.env


# --------------------------------------------------------------------------------------------------------- the DC scan
def dc_signals(n, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return {"noise": 0.25 * rng.standard_normal(n),
            "noise on a large offset": 0.9 + 0.05 * rng.standard_normal(n),
            "sines": 0.4 * np.sin(2 * np.pi * 0.0021 * t + 0.3) + 0.3 * np.sin(2 * np.pi * 0.0517 * t + 1.1) - 0.2,
            "quiet": 1.0e-6 * rng.standard_normal(n) + 1.0e-3}


def dc_distance(x, rate, calls=None):
    """(long-double run, largest |sequential fp64 - long double|) of one channel, cut into the given calls (callbacks)"""
    alpha, _ = M.design(rate)
    runs = {}
    for dt in (LD, np.float64):
        st, parts, o = [0.0, 0.0], [], 0
        for n in (calls or [len(x)]):
            y, st = M.dc_block(x[o:o + n], alpha, st, dt)
            parts.append(y)
            o += n
        runs[dt] = np.concatenate(parts)
    return runs[LD], float(np.max(np.abs(runs[np.float64].astype(LD) - runs[LD])))


@pytest.mark.parametrize("rate", (8000.0, 44100.0, 48000.0, 96000.0))
def test_dc_scan_against_long_double(rate):
    alpha, _ = M.design(rate)
    n = 3 * 2048 + 5
    for name, x in dc_signals(n).items():
        ref, dist = dc_distance(x, rate)
        one, _ = scan_dc(x, alpha)
        parts, st, o = [], (0.0, 0.0), 0
        for m in (2047, 1, 2049, n - 4097):                        # the same samples in four calls
            y, st = scan_dc(x[o:o + m], alpha, st)
            parts.append(y)
            o += m
        four = np.concatenate(parts)
        r1 = float(np.max(np.abs(one.astype(LD) - ref))) / dist
        r4 = float(np.max(np.abs(four.astype(LD) - ref))) / dist
        print(f"{rate:.0f} Hz, {name}: sequential fp64 {dist:.3e} from long double; scan {r1:.2f} x, in four calls {r4:.2f} x")
        assert r1 <= DC_BAR and r4 <= DC_BAR


def test_dc_scan_zeros_and_first_chunk():
    alpha, _ = M.design(48000.0)
    y, st = scan_dc(np.zeros(5000), alpha)
    assert not y.any() and st == (0.0, 0.0)
    x = dc_signals(8)["noise"]                                      # from a zero state the first chunk is the sequential form itself
    y, st = scan_dc(x, alpha)
    ys, ss = M.dc_block(x, alpha, [0.0, 0.0])
    assert np.array_equal(y, ys) and list(st) == ss


# -------------------------------------------------------------------------------------------------------------- sanitizers
def test_out_design_under_sanitizers(tmp_path):
    exe = tmp_path / "out_design_check"
    csrc = os.path.join(ROOT, "convopeq_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "sanitize", "out_design_check.cpp"), os.path.join(csrc, "out_design.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 failed checks" in r.stdout and "FAILED" not in r.stdout
