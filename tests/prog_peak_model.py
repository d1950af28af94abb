"""numpy restatement of the true peak per programme of convopeq_amd/csrc/prog_plan.hpp (ITU-R BS.1770-4 Annex 2: the 48-tap,
4-phase interpolator), independent of the C++, beside tests/prog_model.py (which stays as it is: the loudness).

  peaks(x, rate)            x [rows, n], each row a programme from its start -> (true_peak, sample_peak), linear, per row
  interpolated(x, p)        |y| of phase p at every sample, zero history
  sum_bound(x, rate)        per row: sum_k |c[p][k]| |x[i - k]| at the (i, p) of the true peak
  scaling_bound(x, rate, g) per row: how far tp(g x) may stand from g tp(x)

Per sample i and phase p: y = c[p][0] x[i], then y = y + c[p][k] x[i - k] for k = 1 ... 11 in that order, the multiply and the
add rounding separately: numpy's elementwise operations are exactly that.  A maximum does not depend on order, so the device's
result is this one to the bit."""
import numpy as np

PHASE0 = (14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68)
PHASE1 = (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155)
COEF = np.array([PHASE0, PHASE1, PHASE1[::-1], PHASE0[::-1]], dtype=np.float64) / 8192.0
TAPS = 12


def phases(rate):
    return (0, 1, 2, 3) if rate < 88200 else (0, 2) if rate < 176400 else ()


def scrub(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) < 1.0e300, x, 0.0)


def _padded(x):
    x = scrub(np.atleast_2d(x))
    return np.concatenate([np.zeros((x.shape[0], TAPS - 1)), x], axis=1), x.shape[1]


def interpolated(x, p):
    xp, n = _padded(x)
    y = COEF[p][0] * xp[:, TAPS - 1:]
    for k in range(1, TAPS):
        y = y + COEF[p][k] * xp[:, TAPS - 1 - k:TAPS - 1 - k + n]
    return np.abs(y)


def peaks(x, rate):
    xs = scrub(np.atleast_2d(x))
    sp = np.abs(xs).max(axis=1) if xs.shape[1] else np.zeros(xs.shape[0])
    ph = phases(rate)
    if not ph or not xs.shape[1]:
        return sp.copy(), sp
    tp = np.zeros(xs.shape[0])
    for p in ph:
        tp = np.maximum(tp, interpolated(xs, p).max(axis=1))
    return tp, sp


def sum_bound(x, rate):
    xp, n = _padded(x)
    out = np.zeros(xp.shape[0])
    best = np.full(xp.shape[0], -1.0)
    for p in phases(rate):
        y = interpolated(x, p)
        i = y.argmax(axis=1)
        for r in range(xp.shape[0]):
            if y[r, i[r]] > best[r]:
                best[r] = y[r, i[r]]
                out[r] = sum(abs(COEF[p][k]) * abs(xp[r, TAPS - 1 + i[r] - k]) for k in range(TAPS))
    return out


def scaling_bound(x, rate, g):
    """|tp(g x) - g tp(x)| per row.  B = sum_k |c[p][k]| |x[i - k]| at the peak.  A 12-term sum of products computed in fp64
    stands within gamma_12 B of the exact one (gamma_n = n u / (1 - n u), u = 2^-53); on g x every input carries one more
    rounding: gamma_13 g B; g tp(x) is one more multiply: u g tp(x)."""
    u = 2.0 ** -53

    def gamma(n):
        return n * u / (1.0 - n * u)
    tp, _ = peaks(x, rate)
    return g * sum_bound(x, rate) * (gamma(12) + gamma(13)) + u * g * tp


def dbtp(v):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(v)
