"""CPU tests of the dither stage's host side: tests/dither_model.py against the reference's recorded codes
(tests/golden/dither_ref.npz, written by tests/golden/make_dither_ref.py from the reference's own two headers), cpq_dither_design
against the model, and dither_design.cpp (DitherHost) under the address and undefined-behaviour sanitizers as a program of its
own against the same codes.  Every comparison is bit for bit; a NaN matches a NaN."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dither_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = [(sh, bits, rate) for sh in (M.FIXED4, M.FIXED15) for bits in (8, 16, 24) for rate in (44100.0, 48000.0, 64000.0, 1.0e6)]


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "dither_ref.npz"))


expected = M.recorded


def same_bits_or_nan(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    a0, b0 = np.ascontiguousarray(np.where(na, 0.0, a)), np.ascontiguousarray(np.where(nb, 0.0, b))
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a0.view(np.uint64), b0.view(np.uint64))


@pytest.mark.parametrize("sh,bits,rate", CASES)
def test_model_equals_the_reference(fixture, sh, bits, rate):
    x, (n1, n2) = fixture["input"], fixture["calls"]
    st = M.Dither(rate, 1, sh, bits)
    y = np.concatenate([st.process(x[:, :n1], float(fixture["headroom"])), st.process(x[:, n1:], float(fixture["headroom"]))], axis=1)
    want = expected(fixture, sh, bits, rate)
    assert same_bits_or_nan(y, want)
    assert np.isnan(want).any() == (sh == M.FIXED15)          # only the 15-tap shaper lets a NaN through
    assert not np.isinf(want).any()


def test_fixture_covers_what_it_should(fixture):
    x = fixture["input"]
    assert x.shape == (2, 2051) and list(fixture["calls"]) == [1000, 1051] and float(fixture["headroom"]) == M.H
    assert np.isnan(x).sum() >= 2 and np.isposinf(x).any() and np.isneginf(x).any()
    assert (x[:, 200:260] == 0.0).all() and (np.abs(x[:, 300:360]) == 1.5).all() and (x[:, 400:440] == 1.0e-9).all()
    clamped = expected(fixture, M.FIXED15, 16, 48000.0)[0, 320:340]
    assert np.all(clamped <= 1.0 - 2.0 ** -15) and np.all(clamped > 0.99)


@pytest.mark.parametrize("sh,bits,rate", CASES + [(M.FIXED4, 1, 96000.0), (M.FIXED15, 32, 10.0), (M.FIXED4, 20, 176400.0),
                                                  (M.FIXED15, 16, 767999.99), (M.FIXED4, 16, 200000.0)])
def test_design_matches_model(amd, sh, bits, rate):
    c, scale = amd.dither_design(rate, sh, bits)
    mc, ms = M.design(rate, sh, bits)
    assert list(c) == mc and scale == ms == 2.0 ** -(bits - 1)


def test_design_refusals_and_binding(amd):
    from convopeq_amd import _capi as K
    lib = K.load()
    c, s = np.empty(16), C.c_double()
    cp = c.ctypes.data_as(K.c_double_p)
    for sh, bits in ((0, 16), (3, 16), (-1, 16), (1, 0), (2, 33), (1, -5)):
        assert lib.cpq_dither_design(48000.0, sh, bits, cp, C.byref(s)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_dither_design(48000.0, 1, 16, None, C.byref(s)) == K.CPQ_ERR_INVALID_ARG
    assert K.KERNEL_IDS["k_dither"] == 12 and lib.cpq_kernel_name(12) == b"k_dither" and lib.cpq_kernel_name(13) == b"?"
    assert lib.cpq_abi_revision() == 1 and lib.cpq_abi_version() == 2
    assert (K.CPQ_DITHER_OFF, K.CPQ_DITHER_FIXED4, K.CPQ_DITHER_FIXED15) == (M.OFF, M.FIXED4, M.FIXED15) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "convopeq_mi355x.h")).read()
    assert f"#define CPQ_DITHER_TILE    {K.CPQ_DITHER_TILE}" in header and "#define CPQ_HAS_DITHER 1" in header
    assert lib.cpq_engine_set_dither(None, 1, 16) == K.CPQ_ERR_INVALID_ARG and lib.cpq_dither_reset(None) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_dither_process(None, None, None, 64) == K.CPQ_ERR_INVALID_ARG


def test_the_four_tap_sum_check_refuses_four_presets():
    """setCoefficients keeps the constructor's 48 kHz set when a preset's sum is off 1.0 by more than 1e-12"""
    for rate, refused in ((44100.0, True), (88200.0, False), (176400.0, True), (192000.0, False), (352800.0, True), (384000.0, True),
                          (705600.0, False), (768000.0, False)):
        assert (M.design(rate, M.FIXED4, 16)[0][:4] == list(M.PRESETS4[1])) == refused


@pytest.mark.parametrize("sh", (M.FIXED4, M.FIXED15))
def test_splitting_the_signal_changes_nothing(sh):
    rng = np.random.default_rng(11)
    n = 400
    x = 0.4 * rng.standard_normal((4, n))
    ref = M.Dither(48000.0, 2, sh, 16)
    y = ref.process(x, 1.0)
    assert np.array_equal(y * 32768.0, np.rint(y * 32768.0))
    for cut in (1, 63, 64, 65):
        st = M.Dither(48000.0, 2, sh, 16)
        parts = [st.process(x[:, o:o + cut], 1.0) for o in range(0, n, cut)]
        assert same_bits_or_nan(np.concatenate(parts, axis=1), y)
        assert np.array_equal(st.err, ref.err) and np.array_equal(st.rng, ref.rng)


def test_zero_input_is_the_dither_pattern_alike_across_streams():
    for sh in (M.FIXED4, M.FIXED15):
        y = M.Dither(48000.0, 3, sh, 16).process(np.zeros((6, 64)), 1.0)
        assert y.any() and np.array_equal(y[0], y[2]) and np.array_equal(y[1], y[5]) and not np.array_equal(y[0], y[1])
        assert np.abs(y).max() <= 8.0 / 32768.0


def test_dither_host_under_sanitizers(fixture, tmp_path):
    dump = tmp_path / "cases.txt"
    x, (n1, n2) = fixture["input"], fixture["calls"]
    hexes = lambda a: " ".join(f"{v:x}" for v in np.ascontiguousarray(a).view(np.uint64).reshape(-1).tolist())
    with open(dump, "w") as f:
        for sh, bits, rate in CASES:
            f.write(f"case {sh} {bits} {rate!r} {n1} {n2}\n{hexes(x)}\n{hexes(expected(fixture, sh, bits, rate))}\n")
    exe = tmp_path / "dither_design_check"
    csrc = os.path.join(ROOT, "convopeq_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "sanitize", "dither_design_check.cpp"), os.path.join(csrc, "dither_design.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f" {len(CASES)} cases, 0 failed checks" in r.stdout and "FAILED" not in r.stdout
