"""What tests/prog_finish_inputs.py claims of its planted hop sums, checked without a GPU: the exact programmes are exact, the tie
cases tie, the hand-derived counts are the model's, the library's host finish (cpq_loudness_finish_host) reproduces the numpy
model on all of it, the fixture for the sanitizer program is the helper's, and cpq_diag_prog_finish refuses what it must before
it looks for a device."""
import math
import os

import numpy as np
import pytest

import prog_finish_inputs as F
import prog_model as P

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "prog_finish_edge_cases.txt")
COUNTS = ("n_hops", "n_blocks", "n_abs", "n_rel", "n_short_kept")
FIGURES = ("integrated", "range", "momentary_max", "short_term_max", "relative_gate")


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_exact_programmes_are_exact():
    """the model in fp64 and in np.longdouble: identical mean squares and counts, so no sum or block of these programmes rounds"""
    sizes = set()
    for name, E in F.exact_cases():
        assert np.all(E == np.round(E)) and np.all(E % 480.0 == 0.0) and E.max(initial=0.0) <= 30720.0 * 64.0, name
        a, b = F.model(name), P.finish(E, F.H, np.longdouble)
        za, na = F.record(a)
        zb, nb = F.record(b)
        assert np.array_equal(bits(za), bits(zb)) and np.array_equal(na, nb), (name, za, zb, na, nb)
        assert float(a["z_short_mean"]) == float(b["z_short_mean"]) and a["n_cand"] == F.short_count(len(E)), name
        sizes.add(F.sort_size(a["n_cand"]))
    assert {2, 4, 32, 256, 512, 2048, 8192} <= sizes


def test_exact_programmes_cover_what_they_are_for():
    got = {name: F.model(name) for name, _ in F.exact_cases()}
    assert {len(E) for _, E in F.exact_cases()} >= set(F.N_HOPS)
    for n in (40, 2590, 81940):
        for kind in F.KINDS:
            assert f"{kind}_{n}" in got
    for kept in (1, 2, 3, 10, 11, 21):
        assert got[f"kept_{kept}"]["n_short_kept"] == kept == got[f"kept_{kept}"]["n_cand"]
        q = got[f"kept_{kept}_quiet_head"]
        assert q["n_short_kept"] == kept == q["n_short_abs"] and q["n_cand"] == kept + 4
    for n in (2590, 81940):
        r = got[f"loud_silent_loud_{n}"]        # padding between kept values, at both gates of the range
        assert r["n_short_kept"] < r["n_short_abs"] < r["n_cand"] and r["n_rel"] < r["n_abs"] < r["n_blocks"]
        E = dict(F.exact_cases())[f"loud_silent_loud_{n}"]
        c = P.blocks(E, 30, F.H)[0::10]
        keep = (c > P.Z_ABS) & (c > 0.01 * float(r["z_short_mean"]))
        assert np.count_nonzero(np.diff(keep.astype(int))) >= 10
        assert len(np.unique(P.blocks(dict(F.exact_cases())[f"constant_{n}"], 30, F.H))) == 1
    r = got["random_81940"]
    assert r["n_short_kept"] == F.SORT_MAX and got["random_81949"]["n_cand"] == F.SORT_MAX and got["random_81939"]["n_cand"] == F.SORT_MAX - 1
    two = P.blocks(dict(F.exact_cases())["two_level_2590"], 30, F.H)[0::10]
    assert len(two) == 257 and len(np.unique(two)) < 20         # runs of ties among the kept values


def test_numpy_sum_and_the_device_order_agree_on_the_longest_programme():
    E = dict(F.exact_cases())["random_81940"]
    zm = P.blocks(E, 4, F.H)
    r = F.model("random_81940")
    assert F.tree_mean(zm, zm > P.Z_ABS) == float(r["z_gate"])
    assert F.tree_mean(zm, (zm > P.Z_ABS) & (zm > 0.1 * float(r["z_gate"]))) == float(r["z_int"])


def test_tie_cases_tie_and_their_neighbours_do_not():
    T = F.ties()
    for name, (E, want) in T.items():
        r = F.model(name)
        for k, v in want.items():
            assert r[k] == v, (name, k, r[k], v)
    # relative gate, momentary: the four quiet blocks are the gate itself
    r = F.model("rel_momentary_tie")
    zm = P.blocks(T["rel_momentary_tie"][0], 4, F.H)
    assert 0.1 * float(r["z_gate"]) == 1.0 and np.count_nonzero(zm == 1.0) == 4 and np.count_nonzero(zm == 19.0) == 4
    assert 0.1 * float(F.model("rel_momentary_up")["z_gate"]) == 1.0 and 0.1 * float(F.model("rel_momentary_down")["z_gate"]) == 1.0
    assert P.blocks(T["rel_momentary_up"][0], 4, F.H)[7] == np.nextafter(1.0, 2.0)
    assert P.blocks(T["rel_momentary_down"][0], 4, F.H)[7] == np.nextafter(1.0, 0.0)
    # absolute gate, momentary and short-term: the block is zAbs, the neighbour the next double above it
    assert np.count_nonzero(P.blocks(T["abs_momentary_tie"][0], 4, F.H) == P.Z_ABS) == 4
    assert np.count_nonzero(P.blocks(T["abs_momentary_up"][0], 4, F.H) == np.nextafter(P.Z_ABS, 1.0)) == 4
    assert P.blocks(T["abs_short_tie"][0], 30, F.H)[0] == P.Z_ABS and F.UNIT * P.Z_ABS / F.UNIT == P.Z_ABS
    up = T["abs_short_up"][0][5]
    # the two neighbouring hop sums whose decisions differ (hop sums lie further apart here than blocks: the quotient skips a double)
    assert up == np.nextafter(F.UNIT * P.Z_ABS, 1.0) and np.nextafter(up, 0.0) / F.UNIT == P.Z_ABS < up / F.UNIT
    assert P.blocks(T["abs_short_up"][0], 30, F.H)[0] == up / F.UNIT <= np.nextafter(np.nextafter(P.Z_ABS, 1.0), 1.0)
    # relative gate, short-term: an exact tie exists: mean 100, 0.01 * 100.0 == 1.0, the candidate is 1.0
    for tag in ("tie", "up", "down"):
        r = F.model(f"rel_short_{tag}")
        assert float(r["z_short_mean"]) == 100.0 and 0.01 * float(r["z_short_mean"]) == 1.0, tag
    assert P.blocks(T["rel_short_tie"][0], 30, F.H)[0] == 1.0
    assert P.blocks(T["rel_short_up"][0], 30, F.H)[0] == np.nextafter(1.0, 2.0)
    assert P.blocks(T["rel_short_down"][0], 30, F.H)[0] == np.nextafter(1.0, 0.0)


def test_value_cases_in_the_model():
    r = F.model("inf_mid")
    assert math.isinf(float(r["z_gate"])) and r["n_abs"] > 0 and r["n_rel"] == 0 and r["integrated"] == -math.inf
    assert r["n_short_abs"] == r["n_cand"] and r["n_short_kept"] == 0           # the mean is inf: nothing is above 0.01 of it
    r = F.model("inf_behind_the_last_candidate")
    assert r["n_rel"] == 0 and r["n_short_kept"] == r["n_cand"] == 24 and math.isinf(float(r["z_short_max"])) and math.isfinite(float(r["z_hi"]))
    for name in ("denormal", "denormal_and_one_loud"):
        E = F.value_cases()[name]
        assert np.all((E[E < 1.0] > 0.0) & (E[E < 1.0] < 2.0 ** -1022)), name
    assert F.model("denormal")["n_abs"] == 0 and float(F.model("denormal")["z_mom_max"]) > 0.0
    assert F.model("denormal_and_one_loud")["n_abs"] == 4 and F.model("denormal_and_one_loud")["n_short_kept"] == 3
    E = F.value_cases()["near_1e300"]
    assert E.max() > 1.0e299 and np.isfinite(P.blocks(E, 30, F.H).sum()) and F.model("near_1e300")["n_short_kept"] == 24


def test_host_finish_reproduces_the_model(amd):
    """counts equal, and every figure the logarithm of the model's mean square to the bit (one libm on both sides)"""
    named = F.exact_cases() + [(k, v[0]) for k, v in F.ties().items()]
    named += [(k, v) for k, v in F.value_cases().items() if "nan" not in k and k != "near_1e300"]
    for name, E in named:
        want, got = F.model(name), amd.loudness_finish_host(E, F.RATE)
        for k in COUNTS:
            assert got[k] == want[k], (name, k, got[k], want[k])
        for k in FIGURES:
            assert got[k] == want[k], (name, k, got[k], want[k])
    # inexact sums: the counts, the maxima and the picks do not depend on the order
    want, got = F.model("near_1e300"), amd.loudness_finish_host(F.value_cases()["near_1e300"], F.RATE)
    assert [got[k] for k in COUNTS + ("momentary_max", "short_term_max", "range")] == [want[k] for k in COUNTS + ("momentary_max", "short_term_max", "range")]
    assert abs(got["integrated"] - want["integrated"]) <= 10.0 / math.log(10.0) * 262 * 2.0 ** -52
    # a hop sum of nan is in no block that counts
    got = amd.loudness_finish_host(F.value_cases()["nan_mid"], F.RATE)
    assert got["n_blocks"] == 262 and got["n_abs"] == 262 - 4 == got["n_rel"] and got["n_short_kept"] == 24 - 3
    assert all(math.isfinite(got[k]) for k in FIGURES)


def test_fixture_is_the_helpers(tmp_path):
    fresh = tmp_path / "cases.txt"
    F.write_fixture(str(fresh))
    assert open(FIXTURE).read() == fresh.read_text()
    assert os.path.getsize(FIXTURE) < 200 * 1024


def test_diag_prog_finish_refuses_before_looking_for_a_device(amd):
    import torch
    from convopeq_amd import _capi
    lib = _capi.load()
    res = F.refusals(lib)
    assert len(res) == 12
    assert [r for r in res if r[1] != _capi.CPQ_ERR_INVALID_ARG] == []
    assert b"prog_finish" in lib.cpq_last_error(None)
    if not torch.cuda.is_available():
        for E, n in ((np.ones(40), None), (np.ones((3, 64)), 40), (np.ones(81949), None), (np.ones(5), 0)):
            rc, res, z, counts = F.diag_prog_finish(E, n)
            assert rc == _capi.CPQ_ERR_NO_DEVICE and np.isnan(z).all() and (counts == -1).all()
