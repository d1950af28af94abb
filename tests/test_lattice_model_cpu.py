"""CPU tests of the adaptive shaper's host side: tests/lattice_model.py against the reference's recorded codes
(tests/golden/lattice_ref.npz, written by tests/golden/make_lattice_ref.py from the reference's own LatticeNoiseShaper.h),
cpq_dither_design against the default set, the two new entries' refusals, and dither_design.cpp (DitherHost's lattice path)
under the address and undefined-behaviour sanitizers as a program of its own against the model.  Every comparison is bit for
bit; a NaN matches a NaN."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import lattice_model as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SETS, BITS = "abcde", (8, 16, 24)
CASES = [(case, bits) for case in SETS for bits in BITS]


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "lattice_ref.npz"))


def same_bits_or_nan(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    a0, b0 = np.ascontiguousarray(np.where(na, 0.0, a)), np.ascontiguousarray(np.where(nb, 0.0, b))
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a0.view(np.uint64), b0.view(np.uint64))


def run_model(fx, case, bits, keep=None):
    x, (n1, n2) = fx["input"], fx["calls"]
    st = L.Lattice(1, bits)
    st.set_coeffs(None, fx["set1_" + case])
    parts = [st.process(x[:, :n1], float(fx["headroom"]))]
    if keep is not None:
        keep.append(np.abs(st.state).max())
    if bool(fx["swap_" + case]):
        st.set_coeffs(None, fx["set2_" + case])
    parts.append(st.process(x[:, n1:], float(fx["headroom"])))
    if keep is not None:
        keep.append(np.abs(st.state).max())
    return np.concatenate(parts, axis=1)


@pytest.fixture(scope="module")
def model_rows(fixture):
    """the model's rows of every case, computed once"""
    peaks = {}
    rows = {}
    for case, bits in CASES:
        peaks[case, bits] = []
        rows[case, bits] = run_model(fixture, case, bits, peaks[case, bits])
    return rows, peaks


@pytest.mark.parametrize("case,bits", CASES)
def test_model_equals_the_reference(fixture, model_rows, case, bits):
    want = L.recorded(fixture, case, bits)
    assert same_bits_or_nan(model_rows[0][case, bits], want)
    x = fixture["input"]
    assert np.array_equal(np.isnan(want), np.isnan(x))                      # a NaN in is a NaN out for that sample only
    assert want[1, 505] == 1.0 - 2.0 ** -(bits - 1) and want[0, 510] == -1.0     # +-inf goes to the rails


def test_fixture_covers_what_it_should(fixture, model_rows):
    x = fixture["input"]
    assert x.shape == (2, 2051) and list(fixture["calls"]) == [1000, 1051] and float(fixture["headroom"]) == L.H
    assert np.isnan(x).sum() >= 2 and np.isposinf(x).any() and np.isneginf(x).any()
    assert list(fixture["set1_a"]) == list(L.DEFAULT) == list(fixture["set1_e"]) and list(fixture["set2_e"]) == list(fixture["set1_b"])
    assert np.abs(fixture["set1_b"]).max() <= 0.3 and len(fixture["set1_d"]) == 6
    assert L.clamp_coeffs(fixture["set1_d"]) == [0.85, -0.85, 0.0, 0.0, 0.25, -0.125, 0.0, 0.0, 0.0]
    rows, peaks = model_rows
    for bits in BITS:
        c = L.recorded(fixture, "c", bits)
        ok = ~np.isnan(c)
        assert max(peaks["c", bits]) == 2.0                                 # the states reach the +-2 clamp
        assert (c[ok] == -1.0).any() and (c[ok] == 1.0 - 2.0 ** -(bits - 1)).any()      # and the output both rails
        assert not same_bits_or_nan(rows["a", bits], rows["b", bits])
        n1 = int(fixture["calls"][0])
        assert same_bits_or_nan(rows["e", bits][:, :n1], rows["a", bits][:, :n1])
        assert not same_bits_or_nan(rows["e", bits][:, n1:], rows["a", bits][:, n1:])
        assert not same_bits_or_nan(rows["e", bits][:, n1:], rows["b", bits][:, n1:])   # the generators were not rewound


def test_exact_fma():
    """the rational route is a single rounding: cases where multiply-then-add rounds twice and lands elsewhere"""
    rng = np.random.default_rng(3)
    differ = 0
    for _ in range(2000):
        a, b = rng.uniform(-2.0, 2.0), rng.uniform(-0.85, 0.85)
        c = -(a * b) * (1.0 + rng.integers(-3, 4) * 2.0 ** -52)
        r = L.fma(a, b, c)
        assert r == float(Fraction(a) * Fraction(b) + Fraction(c))
        differ += r != a * b + c
    assert differ > 100
    assert L.fma(3.0, 1.0 + 2.0 ** -52, -3.0) == 3.0 * 2.0 ** -52
    assert L.fma(1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0) == -(2.0 ** -60)              # fl(a b) = 1: two roundings give 0
    assert math.copysign(1.0, L.fma(0.0, 0.5, -0.0)) == 1.0 and math.copysign(1.0, L.fma(-0.0, 0.5, -0.0)) == -1.0
    assert math.copysign(1.0, L.fma(2.0, 0.5, -1.0)) == 1.0


@pytest.mark.parametrize("bits", (1, 8, 16, 24, 32))
def test_design_is_the_default_set(amd, bits):
    for rate in (44100.0, 48000.0, 1.0e6, -1.0):                           # the rate is ignored
        c, scale = amd.dither_design(rate, amd.CPQ_DITHER_ADAPTIVE9, bits)
        assert list(c) == list(L.DEFAULT) + [0.0] * 7 and scale == 2.0 ** -(bits - 1)


def test_refusals_and_binding(amd):
    from convopeq_amd import _capi as K
    lib = K.load()
    k = np.zeros(9)
    kp = k.ctypes.data_as(K.c_double_p)
    assert lib.cpq_dither_set_adaptive_coeffs(None, 0, kp, 9) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_dither_get_adaptive_coeffs(None, 0, kp) == K.CPQ_ERR_INVALID_ARG
    c, s = np.empty(16), C.c_double()
    cp = c.ctypes.data_as(K.c_double_p)
    for sh, bits in ((4, 0), (4, 33), (3, 16), (5, 16)):
        assert lib.cpq_dither_design(48000.0, sh, bits, cp, C.byref(s)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_dither_design(48000.0, 4, 16, None, C.byref(s)) == K.CPQ_ERR_INVALID_ARG
    assert K.CPQ_DITHER_ADAPTIVE9 == amd.CPQ_DITHER_ADAPTIVE9 == L.ADAPTIVE9 == 4
    assert K.KERNEL_IDS["k_dither"] == 12 and len(K.KERNEL_IDS) == 13 and lib.cpq_kernel_name(13) == b"?"      # CPQ_K_COUNT stays 13
    assert lib.cpq_abi_revision() == 1
    header = open(os.path.join(ROOT, "include", "convopeq_mi355x.h")).read()
    assert "#define CPQ_DITHER_ADAPTIVE9 4" in header and "#define CPQ_HAS_ADAPTIVE_DITHER 1" in header
    assert "kAdaptiveNoiseShaperSampleRateBankCount" in header and "clampStateSIMD" in header


def test_splitting_the_signal_changes_nothing():
    rng = np.random.default_rng(11)
    n = 200
    x = 0.4 * rng.standard_normal((4, n))
    sets = ([0.82, -0.68, 0.55, -0.43, 0.33, -0.25, 0.18, -0.12, 0.07], [0.1, -0.2, 0.3])

    def make():
        st = L.Lattice(2, 16)
        for s, k in enumerate(sets):
            st.set_coeffs(s, k)
        return st
    ref = make()
    y = ref.process(x, 1.0)
    assert np.array_equal(y * 32768.0, np.rint(y * 32768.0)) and not np.array_equal(y[0], y[2])
    for cut in (1, 63, 65):
        st = make()
        parts = [st.process(x[:, o:o + cut], 1.0) for o in range(0, n, cut)]
        assert same_bits_or_nan(np.concatenate(parts, axis=1), y)
        assert np.array_equal(st.state, ref.state) and np.array_equal(st.rng, ref.rng)


def test_dither_host_under_sanitizers(fixture, model_rows, tmp_path):
    """DitherHost's lattice path == the model (which == the reference's codes), as a stand-alone program"""
    dump = tmp_path / "cases.txt"
    x, (n1, n2) = fixture["input"], fixture["calls"]
    hexes = lambda a: " ".join(f"{v:x}" for v in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).reshape(-1).tolist())
    with open(dump, "w") as f:
        for case, bits in CASES:
            a, b = fixture["set1_" + case], fixture["set2_" + case]
            nb = len(b) if bool(fixture["swap_" + case]) else -1
            f.write(f"case {bits} {n1} {n2} {len(a)} {nb}\n{hexes(a)}\n{hexes(b)}\n{hexes(x)}\n{hexes(model_rows[0][case, bits])}\n")
    exe = tmp_path / "lattice_design_check"
    csrc = os.path.join(ROOT, "convopeq_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "sanitize", "lattice_design_check.cpp"), os.path.join(csrc, "dither_design.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f" {len(CASES)} cases, 0 failed checks" in r.stdout and "FAILED" not in r.stdout
