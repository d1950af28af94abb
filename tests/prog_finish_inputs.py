"""Planted hop sums for k_prog_finish alone (cpq_diag_prog_finish; tests/test_gpu_prog_finish.py runs them on the device,
tests/test_prog_finish_inputs_cpu.py asserts here what the constructions claim, tests/golden/prog_finish_edge_cases.txt carries
some of them to tests/sanitize/prog_plan_check.cpp).

Exact programmes.  At 10240 Hz a hop is H = 1024 samples, and E[h] = 30720 v[h] with v a multiple of 1 / 64 in [0, 64] (0 only in
the silent stretches) makes E a whole multiple of 480 below 2^21.  A momentary block is (sum of 4 E) / 4096, a multiple of
15 / 128; a short-term block is (sum of 30 E) / 30720 = (sum of 64 v) / 64.  Both are exact, any sum of up to 2^17 of them is
exact in any order (below 2^53 in units of 1 / 128), and a mean is one correctly rounded division: numpy's finish
(tests/prog_model.py), which adds in another order than the device's lanes and tree, must give the device's mean squares and
counts bit for bit.

Ties.  Hop sums that put a block exactly on a gate, with the neighbouring doubles beside them; every gate is strict (z > gate).
What each expects is derived by hand in ties() and asserted of the model in the CPU test."""
import ctypes as C
import functools
import math

import numpy as np

import prog_model as P

RATE = 10240
H = RATE // 10
UNIT = 30720.0                      # E = UNIT v: 30 H
SORT_MAX = 8192
LANES = 256
N_HOPS = (0, 3, 4, 29, 30, 39, 40, 259, 260, 2580, 2590, 10270, 81939, 81940, 81949)
KINDS = ("random", "ascending", "descending", "constant", "two_level", "loud_silent_loud")
Z_NAMES = ("z_int", "z_gate", "z_mom_max", "z_short_max", "z_lo", "z_hi")           # the order of cpq_diag_prog_finish's z
N_NAMES = ("n_abs", "n_rel", "n_short_abs", "n_short_kept")                         # ... and of its counts


def short_count(n_hops):
    return (n_hops - 30) // 10 + 1 if n_hops >= 30 else 0


def sort_size(n_cand):
    p = 2
    while p < n_cand:
        p <<= 1
    return p


def exact(kind, n, seed=0):
    """n hop sums of one kind: 30720 v, v = k / 64 with k a whole number in 1 ... 4096 (0 in silent stretches)"""
    i = np.arange(n)
    if kind == "random":
        k = np.random.default_rng(1000 + seed).integers(1, 4097, n)
    elif kind == "ascending":
        k = 1 + (i * 4095) // max(n - 1, 1)
    elif kind == "descending":
        k = 4096 - (i * 4095) // max(n - 1, 1)
    elif kind == "constant":
        k = np.full(n, 1234 + seed)
    elif kind == "two_level":                       # runs of 70 hops at two levels 9 dB apart: the kept values tie in runs
        k = np.where((i // 70) % 2 == 0, 4096, 512)
    elif kind == "loud_silent_loud":
        # 50 loud hops, 45 of silence, 50 loud, 45 at v = 1 / 64, and again: candidates inside the silence fail the absolute gate
        # (n_short_abs < n_cand), those inside the quiet stretch pass it and fail the relative one (n_short_kept < n_short_abs)
        ph = (i + 17 * seed) % 190
        loud = np.random.default_rng(2000 + seed).integers(2048, 4097, n)
        k = np.where(ph < 50, loud, np.where(ph < 95, 0, np.where(ph < 145, loud, 1)))
    else:
        raise KeyError(kind)
    return UNIT * (k.astype(np.float64) / 64.0)


def kept_programme(kept, quiet_head=False):
    """a random exact programme with `kept` values in the range's sort; quiet_head: 60 silent hops in front, whose four candidates
    are padding in front of the kept values (the first kept candidate then holds 10 loud hops, the second 20)"""
    if quiet_head:
        return np.concatenate([np.zeros(60), exact("random", 10 * kept + 5, seed=kept)])
    return exact("random", 30 + 10 * (kept - 1) + 5, seed=kept)


def exact_cases():
    """(name, E) of every exact programme: every n_hops of N_HOPS at least once, every kind at 40, 2590 and 81940 hops, the kept
    counts of the two percentile picks"""
    out = [(f"random_{n}", exact("random", n, seed=n)) for n in N_HOPS]
    for n in (40, 2590, 81940):
        out += [(f"{kind}_{n}", exact(kind, n, seed=1)) for kind in KINDS[1:]]
    for kept in (1, 2, 3, 10, 11, 21):
        out.append((f"kept_{kept}", kept_programme(kept)))
        out.append((f"kept_{kept}_quiet_head", kept_programme(kept, True)))
    return out


def _up(v):
    return float(np.nextafter(v, math.inf))


def _down(v):
    return float(np.nextafter(v, -math.inf))


def _first_above(e0, w, gate):
    """the smallest double e >= e0 with e / w > gate"""
    e = e0
    while not e / w > gate:
        e = _up(e)
    return e


def ties():
    """name -> (E, expected): expected holds the counts and mean squares derived by hand; the model must give them (CPU test)"""
    out = {}
    # relative gate, momentary: four blocks at z = 1 and four at z = 19 pass the absolute gate, their mean is 10 and
    # 0.1 * 10.0 == 1.0: the blocks at 1.0 sit on the gate and stay out.  One ulp up they are in: (4 (1 + 2^-52) + 76) rounds to 80,
    # so the gate stays 1.0 and the mean of all eight is 10.0.  One ulp down the sum rounds to 80 as well and they stay out.
    for tag, lo, n_rel, z_int in (("tie", 1.0, 4, 19.0), ("up", _up(1.0), 8, 10.0), ("down", _down(1.0), 4, 19.0)):
        E = np.zeros(60)
        E[10], E[30] = 4096.0 * lo, 4096.0 * 19.0
        out[f"rel_momentary_{tag}"] = (E, dict(n_abs=8, n_rel=n_rel, z_gate=10.0, z_int=z_int, z_mom_max=19.0))
    # absolute gate, momentary: 4096 zAbs / 4096 is zAbs itself
    for tag, e, n_abs in (("tie", 4096.0 * P.Z_ABS, 0), ("up", 4096.0 * _up(P.Z_ABS), 4)):
        E = np.zeros(20)
        E[8] = e
        out[f"abs_momentary_{tag}"] = (E, dict(n_abs=n_abs, n_rel=n_abs, z_mom_max=e / 4096.0))
    # absolute gate, short-term: hop 5 lies in the candidate b = 29 alone; 30720.0 zAbs / 30720.0 == zAbs for this zAbs (asserted
    # in the CPU test).  up: the next hop sum whose quotient is above the gate
    e0 = UNIT * P.Z_ABS
    for tag, e, n_sa in (("tie", e0, 0), ("up", _first_above(e0, UNIT, P.Z_ABS), 1)):
        E = np.zeros(40)
        E[5] = e
        out[f"abs_short_{tag}"] = (E, dict(n_abs=4, n_rel=4, n_short_abs=n_sa, n_short_kept=n_sa, z_short_max=e / UNIT))
    # relative gate, short-term: 60 hops have the candidates b = 29, 39, 49, 59; hop 5 lies in the first alone and hop 55 in the
    # last alone, the two in between are silent.  z = 1 and z = 199 pass the absolute gate, their mean is 100 and
    # 0.01 * 100.0 == 1.0: the candidate at 1.0 sits on the gate.  up: (1 + 2^-52) + 199 rounds to 200, the gate stays 1.0.
    for tag, e, kept, z_lo in (("tie", UNIT, 1, 199.0), ("up", _first_above(UNIT, UNIT, 1.0), 2, None), ("down", _down(UNIT), 1, 199.0)):
        E = np.zeros(60)
        E[5], E[55] = e, UNIT * 199.0
        want = dict(n_short_abs=2, n_short_kept=kept, z_hi=199.0, z_short_max=199.0)
        want["z_lo"] = e / UNIT if z_lo is None else z_lo
        out[f"rel_short_{tag}"] = (E, want)
    return out


def value_cases():
    """name -> E: hop sums of inf and nan, denormals and values near 1e300 inside exact programmes"""
    out = {}
    base = exact("random", 265, seed=7)
    for name, at, v in (("inf_mid", 100, math.inf), ("inf_behind_the_last_candidate", 263, math.inf), ("nan_mid", 100, math.nan),
                        ("nan_first", 0, math.nan)):
        E = base.copy()
        E[at] = v
        out[name] = E
    E = base.copy()
    E[40], E[41], E[150] = math.inf, math.nan, math.inf
    out["inf_and_nan"] = E
    out["denormal"] = base * 2.0 ** -1060           # every block below zAbs, every hop sum a denormal
    out["denormal_and_one_loud"] = np.concatenate([base[:200] * 2.0 ** -1060, [UNIT], base[:64] * 2.0 ** -1060])
    out["near_1e300"] = base * (1.0e300 / UNIT / 64.0)
    return out


def fixture_cases():
    """what tests/golden/prog_finish_edge_cases.txt holds: every tie, and padding between kept values at three sort sizes"""
    out = [(name, E) for name, (E, _) in ties().items()]
    out += [(f"loud_silent_loud_{n}", exact("loud_silent_loud", n, seed=1)) for n in (40, 260, 2590)]
    out += [("kept_3_quiet_head", kept_programme(3, True)), ("two_level_260", exact("two_level", 260)),
            ("descending_260", exact("descending", 260))]
    return out


@functools.lru_cache(maxsize=None)
def model(name_or_kind, n=None, seed=0):
    """P.finish of a programme of this module, computed once: model("random", 2590, 3), or model(name) for a name of
    exact_cases(), ties() or value_cases()"""
    if n is not None:
        return P.finish(exact(name_or_kind, n, seed), H)
    named = dict(exact_cases())
    named.update({k: v[0] for k, v in ties().items()})
    named.update(value_cases())
    return P.finish(named[name_or_kind], H)


def record(r):
    """a P.finish result as (z [6], counts [4]) in the order of cpq_diag_prog_finish"""
    return np.array([float(r[k]) for k in Z_NAMES]), np.array([r[k] for k in N_NAMES], dtype=np.int32)


def tree_mean(z, keep):
    """mean of z[keep] in the device's order: lane t adds its blocks t, t + 256, ... in ascending order, then the 256-slot tree"""
    lanes = np.zeros(LANES)
    for t in range(LANES):
        for v in z[t::LANES][keep[t::LANES]]:
            lanes[t] = lanes[t] + v
    s = LANES // 2
    while s >= 1:
        lanes[:s] = lanes[:s] + lanes[s:2 * s]
        s //= 2
    n = int(np.count_nonzero(keep))
    return lanes[0] / n if n else 0.0


# ------------------------------------------------------------------------------------------------------------------ the entry
def diag_prog_finish(hops, n_hops=None, rate=RATE):
    """cpq_diag_prog_finish on hops [S, max_hops] (or one row): (status, results [S] as dicts, z [S, 6], counts [S, 4])"""
    from convopeq_amd import _capi as K
    hops = np.ascontiguousarray(np.atleast_2d(hops), dtype=np.float64)
    S, max_hops = hops.shape
    n_hops = max_hops if n_hops is None else n_hops
    if max_hops == 0:                               # no hops yet: the entry wants a row of at least one element behind them
        hops, max_hops = np.zeros((S, 1)), 1
    res = (K.LoudnessResult * S)()
    z = np.full((S, 6), np.nan)
    counts = np.full((S, 4), -1, dtype=np.int32)
    rc = K.load().cpq_diag_prog_finish(S, n_hops, max_hops, float(rate), hops.ctypes.data_as(K.c_double_p), res,
                                       z.ctypes.data_as(K.c_double_p), counts.ctypes.data_as(C.POINTER(C.c_int32)))
    names = [name for name, _ in K.LoudnessResult._fields_]
    return rc, [{k: getattr(r, k) for k in names} for r in res], z, counts


def refusals(lib):
    """(label, status) of every refusal rule of cpq_diag_prog_finish once, and of every null pointer"""
    from convopeq_amd import _capi as K
    E = np.ones(64)
    p, r = E.ctypes.data_as(K.c_double_p), (K.LoudnessResult * 1)()
    z, c = np.zeros(6), np.zeros(4, dtype=np.int32)
    zp, cp = z.ctypes.data_as(K.c_double_p), c.ctypes.data_as(C.POINTER(C.c_int32))
    bad = [("null hops", (1, 40, 64, 10240.0, None, r, zp, cp)), ("null out", (1, 40, 64, 10240.0, p, None, zp, cp)),
           ("no stream", (0, 40, 64, 10240.0, p, r, zp, cp)), ("32768 streams", (32768, 40, 64, 10240.0, p, r, zp, cp)),
           ("max_hops 0", (1, 0, 0, 10240.0, p, r, zp, cp)), ("n_hops -1", (1, -1, 64, 10240.0, p, r, zp, cp)),
           ("n_hops above max_hops", (1, 65, 64, 10240.0, p, r, zp, cp)), ("rate 10245", (1, 40, 64, 10245.0, p, r, zp, cp)),
           ("rate 7990", (1, 40, 64, 7990.0, p, r, zp, cp)), ("rate nan", (1, 40, 64, math.nan, p, r, zp, cp)),
           ("8193 short-term blocks", (1, 81950, 81950, 10240.0, p, r, zp, cp)),
           ("2^28 + 1 elements", (32767, 40, 8193, 10240.0, p, r, zp, cp))]
    assert 32767 * 8193 > 1 << 28
    return [(label, lib.cpq_diag_prog_finish(*args)) for label, args in bad]


# ---------------------------------------------------------------------------------------------------------------- the fixture
def write_fixture(path):
    """the case / want text format of tests/golden/prog_finish_cases.txt, the wants from the numpy model"""
    z_keys = ("z_gate", "z_int", "z_mom_max", "z_short_max", "z_lo", "z_hi")
    n_keys = ("n_blocks", "n_abs", "n_rel", "n_short_kept")
    with open(path, "w") as f:
        for name, E in fixture_cases():
            r = P.finish(E, H)
            f.write(f"case {name} {H} {len(E)}\n")
            f.write(" ".join(float(e).hex() for e in E) + "\n")
            f.write("want " + " ".join(str(r[k]) for k in n_keys) + " " + " ".join(float(r[k]).hex() for k in z_keys) + "\n")
