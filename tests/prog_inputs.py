"""The programmes the programme-loudness tests run (tests/test_prog_model_cpu.py asserts their properties, the GPU tests meter
them) and their references, computed once per process: the fp64 sequential model's hop sums and their distance d_ref from the
np.longdouble run of the same model."""
import functools
import math

import numpy as np

import prog_model as P

RATE = 8000
H = RATE // 10


def tone(seconds, dbfs, rate=RATE, freq=1000.0, phase=0.0):
    """stereo sine of peak `dbfs` per channel"""
    t = np.arange(int(round(seconds * rate)))
    row = 10.0 ** (dbfs / 20.0) * np.sin(2.0 * math.pi * freq * t / rate + phase)
    return np.stack([row, row])


def stepped(seconds, db0, step_db, seed, noise_db=-50.0):
    """a 1 kHz / 440 Hz pair whose level rises by step_db every second, over a little noise: distinct levels block by block"""
    n = seconds * RATE
    t = np.arange(n)
    level = 10.0 ** ((db0 + step_db * (t // RATE)) / 20.0)
    rng = np.random.default_rng(seed)
    noise = 10.0 ** (noise_db / 20.0) * rng.standard_normal((2, n))
    return np.stack([level * np.sin(2.0 * math.pi * 1000.0 * t / RATE), level * np.sin(2.0 * math.pi * 440.0 * t / RATE + 0.3)]) + noise


def ebu_3341_1(rate=RATE, seconds=5):
    return tone(seconds, -23.0, rate)


def ebu_3341_3(rate=RATE, edge=2, plateau=10):
    return np.concatenate([tone(edge, -36.0, rate), tone(plateau, -23.0, rate), tone(edge, -36.0, rate)], axis=1)


def ebu_3342_1(rate=RATE, each=10):
    return np.concatenate([tone(each, -20.0, rate), tone(each, -30.0, rate)], axis=1)


def scrubbed():
    x = tone(5, -23.0)
    x[0, 1234] = math.nan
    x[1, 2047] = math.inf
    x[0, 2048] = -math.inf
    x[1, 20000] = 1.0e300
    x[0, 31999] = -1.0e300
    return x


def inputs():
    """name -> rows [2, n] at 8000 Hz"""
    return {
        "main60": stepped(60, -28.0, 0.15, seed=5),
        "ebu_3341_1": ebu_3341_1(),
        "ebu_3341_3": ebu_3341_3(),
        "ebu_3342_1": ebu_3342_1(),
        "short_399ms": tone(0.399, -23.0),
        "silence": np.zeros((2, 5 * RATE)),
        "tone_minus80": tone(5, -80.0),
        "hops_4": tone(0.4, -23.0),
        "hops_30": tone(3.0, -23.0),
        "ramp40": stepped(42, -30.0, 0.25, seed=6),
        "scrub": scrubbed(),
    }


# rates whose hop grid meets the 2048-sample span grid (H = 1024: every second hop ends on a span end; H = 2048: a hop is a span)
# and the rate of the longest hop (H = 76800: a hop lies across 38 spans); samples per row
GRID_RATES = {10240: 2 * 10240, 20480: 2 * 20480, 768000: 160000}


def rate_inputs():
    """rate -> 2 s of rows [2, n] (GRID_RATES: their own lengths): a tone pair over noise"""
    out = {}
    for rate, n in ((44100, 2 * 44100), (48000, 2 * 48000)) + tuple(GRID_RATES.items()):
        t = np.arange(n)
        rng = np.random.default_rng(rate)
        out[rate] = np.stack([0.2 * np.sin(2.0 * math.pi * 997.0 * t / rate), 0.1 * np.sin(2.0 * math.pi * 3001.0 * t / rate)]) \
            + 0.01 * rng.standard_normal((2, n))
    return out


SPIKE = 9.9e299                     # passes the scrub (|v| < 1e300); its K-weighted square overflows


def spiked():
    """5 s of the -23 dBFS tone with one sample of 9.9e299 in each channel, both in hop 1: that hop sum is +inf, and the filters
    ring down from 1e300 through the hops behind it (pole radius 0.97 at 8000 Hz: about 30 hops until the tone is back)"""
    x = tone(5, -23.0)
    x[0, 1234] = SPIKE
    x[1, 1300] = -SPIKE
    return x


@functools.lru_cache(maxsize=None)
def spiked_reference():
    """dict(x, E, E_ld, d): the fp64 and long-double models' hop sums and, per hop, their distance d (inf - finite where the fp64
    square overflowed and the long-double one did not: those hops are compared for being +inf, not to a bar)"""
    x = spiked()
    with np.errstate(over="ignore", invalid="ignore"):
        e64 = P.hop_sums(x, RATE, np.float64)[0]
        eld = P.hop_sums(np.concatenate([x, x]), RATE, np.longdouble)[0]
        d = np.abs(e64.astype(np.longdouble) - eld).astype(np.float64)
    return dict(x=x, E=e64, E_ld=eld, d=d)


def stream_programme(s, seconds=3.5):
    """programme of stream s of the geometry tests: its own level, pitch and noise"""
    rng = np.random.default_rng(1000 + s)
    n = int(seconds * RATE)
    t = np.arange(n)
    a = 10.0 ** (rng.uniform(-35.0, -15.0) / 20.0)
    f = rng.uniform(100.0, 3000.0)
    return np.stack([a * np.sin(2.0 * math.pi * f * t / RATE), a * np.sin(2.0 * math.pi * f * t / RATE + 1.0)]) + 0.1 * a * rng.standard_normal((2, n))


def _reference(named, rate):
    names = list(named)
    lengths = [named[k].shape[1] for k in names]
    x = np.zeros((2 * len(names), max(lengths)))
    for i, k in enumerate(names):
        x[2 * i:2 * i + 2, :lengths[i]] = named[k]
    e64 = P.hop_sums(x, rate, np.float64, lengths)
    eld = P.hop_sums(x, rate, np.longdouble, lengths)
    out = {}
    for i, k in enumerate(names):
        d = float(np.max(np.abs(e64[i].astype(np.longdouble) - eld[i]))) if len(e64[i]) else 0.0
        out[k] = dict(x=named[k], E=e64[i].astype(np.float64), E_ld=eld[i], d_ref=d)
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """name -> dict(x, E = the fp64 model's hop sums, E_ld = the long-double run's, d_ref = max |E - E_ld|)"""
    return _reference(inputs(), RATE)


@functools.lru_cache(maxsize=None)
def rate_reference(rate):
    return _reference({"x": rate_inputs()[rate]}, rate)["x"]


def hop_bar(ref, hop_len):
    """per hop: max(8 d_ref, 4 H 2^-52 E)"""
    return np.maximum(8.0 * ref["d_ref"], 4.0 * hop_len * 2.0 ** -52 * ref["E"])
