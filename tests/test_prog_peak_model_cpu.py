"""The numpy model of the true peak per programme (tests/prog_peak_model.py) on EBU Tech 3341's true-peak cases 15 to 19,
synthesised at 48 kHz: the acceptance check of the interpolator table.  2 s of sine with a linear fade-in and fade-out of 100 ms
(without the fades the start transient puts case 18 outside its bar).  Cases 20 to 23 need EBU's files and are left out."""
import math

import numpy as np
import pytest

import prog_peak_model as PK

FS = 48000
CASES = {15: (FS / 4, 0.0, 0.5, -6.4, -5.8), 16: (FS / 4, 45.0, 0.5, -6.4, -5.8), 17: (FS / 6, 60.0, 0.5, -6.4, -5.8),
         18: (FS / 8, 67.5, 0.5, -6.4, -5.8), 19: (FS / 4, 45.0, 1.41, 2.6, 3.2)}


def ebu_sine(case):
    f, deg, amp = CASES[case][:3]
    n, fade = 2 * FS, FS // 10
    x = amp * np.sin(2.0 * np.pi * f * np.arange(n) / FS + math.radians(deg))
    env = np.ones(n)
    env[:fade] = np.arange(fade) / fade
    env[n - fade:] = np.arange(fade, 0, -1) / fade
    return x * env


def test_the_table():
    c = PK.COEF * 8192.0
    assert c[0].sum() == 8205 and c[3].sum() == 8205 and c[1].sum() == 7971 and c[2].sum() == 7971
    assert np.array_equal(c[2], c[1][::-1]) and np.array_equal(c[3], c[0][::-1])
    assert np.array_equal(c, np.round(c))           # every coefficient an integer over 8192: exact in binary
    # the prototype (phases interleaved, at 4 x 48 kHz) is a coherent interpolation low-pass
    proto = np.empty(48)
    for p in range(4):
        proto[p::4] = PK.COEF[p]
    w = np.abs(np.fft.rfft(proto, 4 * 48000 // 100))         # 100 Hz bins at 192 kHz
    db = 20.0 * np.log10(np.maximum(w / 4.0, 1e-12))
    # DC is 32352 / 32768 = -0.111 dB, the largest deviation up to 20 kHz
    assert abs(db[0] - 20.0 * math.log10(32352.0 / 32768.0)) <= 1e-9
    assert np.all(np.abs(db[:201]) <= abs(db[0]) + 1e-9) and abs(db[240] + 6.2) <= 0.1
    assert np.all(db[300:] <= -39.8)                # the highest stop-band lobe stands at -39.85 dB (68.7 kHz)


@pytest.mark.parametrize("case", sorted(CASES))
def test_ebu_3341_true_peak(case):
    lo, hi = CASES[case][3:]
    tp, sp = PK.peaks(ebu_sine(case), FS)
    got = float(PK.dbtp(tp[0]))
    print(f"case {case}: {got:.3f} dBTP (sample peak {float(PK.dbtp(sp[0])):.3f} dBFS), bar [{lo}, {hi}]")
    assert lo <= got <= hi


def test_two_phases_read_the_same_on_cases_16_and_18():
    for case in (16, 18):
        four, _ = PK.peaks(ebu_sine(case), FS)
        two, _ = PK.peaks(ebu_sine(case), 96000)            # the 2x phase set on the same samples
        print(f"case {case}: 4 phases {float(PK.dbtp(four[0])):.3f}, 2 phases {float(PK.dbtp(two[0])):.3f} dBTP")
        assert abs(float(PK.dbtp(four[0])) - float(PK.dbtp(two[0]))) <= 0.0005
        assert -6.4 <= float(PK.dbtp(two[0])) <= -5.8


def test_no_phases_from_176400():
    x = ebu_sine(16)
    tp, sp = PK.peaks(x, 192000)
    assert tp[0] == sp[0] == np.abs(x).max()


@pytest.mark.parametrize("g", (0.1, 1.0 / 3.0, 0.7071, 1.2589254117941673))
def test_scaling(g):
    rng = np.random.default_rng(5)
    x = np.stack([ebu_sine(17), 0.3 * rng.standard_normal(2 * FS)])
    tp, _ = PK.peaks(x, FS)
    scaled, _ = PK.peaks(g * x, FS)
    bound = PK.scaling_bound(x, FS, g)
    print(f"g {g}: |tp(g x) - g tp(x)| {np.abs(scaled - g * tp)}, bound {bound}")
    assert np.all(np.abs(scaled - g * tp) <= bound)


def test_scrub_and_history():
    x = np.array([[0.5, np.nan, -0.25, np.inf, 1e300, -1e300, 0.125]])
    clean = np.array([[0.5, 0.0, -0.25, 0.0, 0.0, 0.0, 0.125]])
    assert np.array_equal(PK.peaks(x, 8000)[0], PK.peaks(clean, 8000)[0]) and PK.peaks(x, 8000)[1][0] == 0.5
    # the first sample alone: zero history, so the peak is the largest |c[p][0]| times it
    tp, sp = PK.peaks(np.array([[1.0]]), 8000)
    assert tp[0] == np.abs(PK.COEF[:, 0]).max() and sp[0] == 1.0
    assert PK.peaks(np.zeros((2, 50)), 8000)[0].tolist() == [0.0, 0.0]
