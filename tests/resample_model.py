"""numpy model of cpq_ir_resample and the closed-form signals of tests/golden/resample_ref.npz.

The filter is read from cpq_resample_design (resample_design below), never re-derived.  Output j of a row is
    sum over k < T of taps[(j M) mod L][k] * x[floor(j M / L) + T / 2 - k]
with x zero outside the row; the model adds the T products of every output in np.longdouble."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_ref.npz")
TONES = (50.0, 997.0, 7001.0, 15011.0, 19001.0)
PAIRS = ((44100, 48000), (48000, 44100), (96000, 48000), (88200, 48000), (44100, 96000), (48000, 96000), (96000, 44100))
T_CENTRE, SIGMA, DURATION = 0.02, 0.002, 0.04
STOP_CARRIER, STOP_PAIR = 30000.0, (96000, 48000)
IMPULSE_AT, IMPULSE_LEN, IMPULSE_PAIR = 100, 512, (44100, 48000)


def _times(n, rate):
    return np.arange(n, dtype=np.longdouble) / np.longdouble(rate) - np.longdouble(T_CENTRE)


def _envelope(tc):
    return np.exp(-(tc * tc) / np.longdouble(2.0 * SIGMA * SIGMA))


def passband_signal(n, rate):
    """0.1 exp(-(t - 0.02)^2 / (2 0.002^2)) sum_k cos(2 pi f_k (t - 0.02) + 0.3 k) at t = i / rate, i < n (longdouble, rounded once)"""
    tc = _times(n, rate)
    two_pi = 2 * np.longdouble(np.pi) + np.longdouble(2.4492935982947064e-16)      # 2 pi to 2^-106
    s = np.zeros(n, dtype=np.longdouble)
    for k, f in enumerate(TONES):
        s += np.cos(two_pi * np.longdouble(f) * tc + np.longdouble(0.3) * k)
    return (np.longdouble(0.1) * _envelope(tc) * s).astype(np.float64)


def stopband_signal(n, rate):
    """the same envelope at 0.5 on a 30 kHz carrier"""
    tc = _times(n, rate)
    two_pi = 2 * np.longdouble(np.pi) + np.longdouble(2.4492935982947064e-16)
    return (np.longdouble(0.5) * _envelope(tc) * np.cos(two_pi * np.longdouble(STOP_CARRIER) * tc)).astype(np.float64)


def input_len(rate):
    return int(round(DURATION * rate))


def out_len(n, in_rate, out_rate):
    """ceil(n out / in) in integers"""
    return -((-n * int(out_rate)) // int(in_rate))


def pair_key(in_rate, out_rate):
    return f"{int(in_rate)}_{int(out_rate)}"


def resample_rows(design, x, n_out=None, outputs=None):
    """the model: x one row; design from convopeq_amd.resample_design.  Returns (y, bound) with y np.longdouble and
    bound[j] = sum_k |taps * x| of output j (what the dot-product error bound scales with).  outputs: the indices wanted."""
    L, M, T, taps = design["L"], design["M"], design["T"], design["taps"]
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if outputs is None:
        outputs = np.arange(out_len(n, design["in_rate"], design["out_rate"]) if n_out is None else n_out)
    outputs = np.asarray(outputs, dtype=np.int64)
    pad = np.concatenate([np.zeros(T), x, np.zeros(T)]).astype(np.longdouble)
    tl = taps.astype(np.longdouble)
    y = np.zeros(len(outputs), dtype=np.longdouble)
    bound = np.zeros(len(outputs), dtype=np.longdouble)
    k = np.arange(T)
    for i, j in enumerate(outputs.tolist()):
        p, n0 = (j * M) % L, (j * M) // L
        idx = n0 + T // 2 - k
        ok = (idx >= -T) & (idx < n + T)
        prod = tl[p][ok] * pad[idx[ok] + T]
        y[i] = prod.sum()
        bound[i] = np.abs(prod).sum()
    return y, bound
