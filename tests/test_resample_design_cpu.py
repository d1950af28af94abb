"""cpq_resample_design: the rate reduction and its refusals, and the polyphase prototype's sums, symmetry, stop band and pass band.
The pass-band yardstick is the reference's own error on the fixture's signals (tests/golden/resample_ref.npz, d_ref)."""
import math

import numpy as np
import pytest

import convopeq_amd as amd
from convopeq_amd import _capi as K
import resample_model as M

RATES = (44100, 48000, 88200, 96000, 176400, 192000, 352800, 384000)


@pytest.fixture(scope="module")
def golden():
    return np.load(M.GOLDEN)


@pytest.fixture(scope="module")
def designs():
    return {p: amd.resample_design(*p) for p in M.PAIRS}


def response(d, freqs_hz):
    """|H(f)| of the prototype h[k L + p] = taps[p][k] at the rate L * in_rate, DC gain L taken out (longdouble sums)"""
    h = d["taps"].T.reshape(-1).astype(np.longdouble)
    m = np.arange(len(h), dtype=np.longdouble) - np.longdouble(d["T"] * d["L"]) / 2
    out = []
    for f in freqs_hz:
        w = 2 * np.longdouble(np.pi) * np.longdouble(f) / (np.longdouble(d["in_rate"]) * d["L"])
        out.append(float(np.hypot((h * np.cos(w * m)).sum(), (h * np.sin(w * m)).sum()) / d["L"]))
    return np.array(out)


def test_reduction_of_every_common_pair():
    for a in RATES:
        for b in RATES:
            d = amd.resample_design(a, b)
            g = math.gcd(a, b)
            assert (d["L"], d["M"]) == (b // g, a // g)
            assert d["L"] <= K.CPQ_RESAMPLE_MAX_FACTOR and d["M"] <= K.CPQ_RESAMPLE_MAX_FACTOR
            assert d["T"] % 2 == 0 and d["group_delay"] == d["T"] / 2 and d["taps"].shape == (d["L"], d["T"])
            assert d["cutoff"] == pytest.approx(0.98 * min(a, b) / a, rel=1e-15)
    d = amd.resample_design(48000, 48000)                   # equal rates are not an error
    assert (d["L"], d["M"]) == (1, 1)


@pytest.mark.parametrize("pair", [(44100.5, 48000), (48000, 44100.25), (7999, 48000), (48000, 768001), (0, 48000), (-48000, 48000),
                                  (float("nan"), 48000), (float("inf"), 48000),
                                  (48000, 44101),       # L = 44101
                                  (44100, 44099),       # M = 44100
                                  (48000, 47963)])      # 47963 is prime
def test_refusals(pair):
    with pytest.raises(amd.CpqError) as e:
        amd.resample_design(*pair)
    assert e.value.status == K.CPQ_ERR_UNSUPPORTED


def test_factor_bound_is_1280():
    d = amd.resample_design(10240, 8008)        # gcd 8: 1001 : 1280
    assert (d["L"], d["M"]) == (1001, 1280)
    d = amd.resample_design(8008, 10240)
    assert (d["L"], d["M"]) == (1280, 1001)
    for pair in ((10248, 8000), (8000, 10248)):     # gcd 8: 1000 : 1281
        with pytest.raises(amd.CpqError) as e:
            amd.resample_design(*pair)
        assert e.value.status == K.CPQ_ERR_UNSUPPORTED


def test_capacity_is_checked():
    lib = K.load()
    info = K.ResampleInfo()
    n = lib.cpq_resample_design(48000.0, 96000.0, info, None, 0)
    assert n == info.l * info.taps
    buf = np.zeros(n)
    assert lib.cpq_resample_design(48000.0, 96000.0, None, buf.ctypes.data_as(K.c_double_p), n - 1) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_resample_design(48000.0, 96000.0, None, buf.ctypes.data_as(K.c_double_p), n) == n


def test_every_phase_sums_to_one(designs):
    for d in designs.values():
        sums = np.array([math.fsum(row) for row in d["taps"]])
        assert np.max(np.abs(sums - 1.0)) <= d["T"] * 2.0 ** -52


def test_table_is_symmetric(designs):
    for d in designs.values():
        h = d["taps"].T.reshape(-1)             # h[m], t = m / L - T / 2: even about m = L T / 2
        assert h[0] == 0.0
        assert np.array_equal(h[1:], h[1:][::-1])


def test_stop_band_is_140_db_down(designs):
    for (a, b), d in designs.items():
        h = d["taps"].T.reshape(-1)
        n = 1 << int(math.ceil(math.log2(len(h) * 16)))
        mag = np.abs(np.fft.rfft(h, n)) / d["L"]
        f = np.fft.rfftfreq(n, 1.0 / (a * d["L"]))
        worst = 20 * np.log10(mag[f >= min(a, b) / 2].max())
        print(f"{a}->{b}: stop band {worst:.1f} dB")
        assert worst <= -140.0


def test_pass_band_at_the_fixture_tones(designs, golden):
    for (a, b), d in designs.items():
        key = M.pair_key(a, b)
        allowed = float(golden["d_ref_" + key]) / float(np.max(np.abs(golden["x_" + key])))
        dev = np.abs(response(d, M.TONES) - 1.0)
        print(f"{a}->{b}: pass-band deviation {dev.max():.2e}, allowed {allowed:.2e}")
        assert dev.max() <= allowed
