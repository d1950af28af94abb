"""k_prog_finish alone (cpq_diag_prog_finish) on the planted hop sums of tests/prog_finish_inputs.py.  Every comparison is for equal
bits; there is no tolerance in this file.

Exact programmes: every block, every sum of blocks in any order and every mean is exact or one correctly rounded division
(tests/test_prog_finish_inputs_cpu.py asserts it), so the numpy model, which shares no code with the kernel and adds in another
order, is the reference for all six mean squares and all four counts of ProgRecord.  Ties on the gates: the hand-derived counts
and means, the model, and cpq_loudness_finish_host.  Values (inf, nan, denormals, near 1e300): cpq_loudness_finish_host, which is
the same text on the host; where the sums are exact or do not depend on an order the model as well.  Layout: the bits of the run
without the layout."""
import math

import numpy as np
import pytest

import prog_finish_inputs as F

pytestmark = pytest.mark.gpu

RESULT = ("integrated", "range", "momentary_max", "short_term_max", "relative_gate", "n_hops", "n_blocks", "n_abs", "n_rel", "n_short_kept")
REACHED = set()                     # sort sizes the device has run in this session


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def bits(a):
    return np.atleast_1d(np.ascontiguousarray(a, dtype=np.float64)).view(np.uint64)


def finish(hops, n_hops=None, rate=F.RATE):
    rc, res, z, counts = F.diag_prog_finish(hops, n_hops, rate)
    assert rc == 0, rc
    return res, z, counts


def same_result(got, want, label):
    """two cpq_loudness_result dicts, floats by their bits (nan payloads excepted)"""
    for k in RESULT:
        a, b = got[k], want[k]
        if isinstance(a, float) and math.isnan(a) and math.isnan(b):
            continue
        assert (bits(a)[0] == bits(b)[0]) if isinstance(a, float) else a == b, (label, k, a, b)


def check_against_model(name, E, amd):
    want = F.model(name)
    res, z, counts = finish(E)
    wz, wn = F.record(want)
    print(f"{name}: {len(E)} hops, sort size {F.sort_size(want['n_cand'])}, counts {counts[0].tolist()} model {wn.tolist()}, z {z[0].tolist()}")
    assert np.array_equal(counts[0], wn), (name, counts[0], wn)
    assert np.array_equal(bits(z[0]), bits(wz)), (name, z[0], wz)
    same_result(res[0], amd.loudness_finish_host(E, F.RATE), name)
    assert res[0]["n_hops"] == len(E) and res[0]["n_blocks"] == max(len(E) - 3, 0)
    return want, res[0], z[0], counts[0]


@pytest.mark.parametrize("name", [name for name, _ in F.exact_cases()])
def test_exact_programme_equals_the_model_in_every_bit(amd, name):
    E = dict(F.exact_cases())[name]
    want, res, z, counts = check_against_model(name, E, amd)
    n_cand = F.short_count(res["n_hops"])
    if name.startswith(("random_", "constant_", "two_level_", "kept_")) and "quiet_head" not in name:
        assert res["n_short_kept"] == n_cand            # the sort is full: no padding below its size but the power of two's
    if res["n_short_kept"]:
        assert z[4] <= z[5]
    REACHED.add(F.sort_size(n_cand))


def test_sort_sizes_512_2048_and_8192_were_reached(amd):
    """more than one element per lane (512), passes with j >= 256 (2048, 8192): through n_hops and n_short_kept of runs above"""
    for n, size in ((2590, 512), (10270, 2048), (81940, 8192)):
        E = F.exact("random", n, seed=n)
        res, z, counts = finish(E)
        kept = res[0]["n_short_kept"]
        assert res[0]["n_hops"] == n and kept == F.short_count(n) and F.sort_size(kept) == size and size // 2 < kept
        REACHED.add(size)
    assert {512, 2048, 8192} <= REACHED


@pytest.mark.parametrize("name", list(F.ties()))
def test_tie_on_a_gate(amd, name):
    E, hand = F.ties()[name]
    want, res, z, counts = check_against_model(name, E, amd)
    got = dict(zip(F.Z_NAMES, z.tolist()))
    got.update(zip(F.N_NAMES, counts.tolist()))
    for k, v in hand.items():
        assert got[k] == v, (name, k, got[k], v)


@pytest.mark.parametrize("name", list(F.value_cases()))
def test_value_edges_equal_the_host_finish(amd, name):
    E = F.value_cases()[name]
    res, z, counts = finish(E)
    host = amd.loudness_finish_host(E, F.RATE)
    print(f"{name}: device {res[0]}, z {z[0].tolist()}, counts {counts[0].tolist()}")
    same_result(res[0], host, name)
    if "nan" not in name:                           # the model's maximum would take the nan
        want = F.model(name)
        wz, wn = F.record(want)
        assert np.array_equal(counts[0], wn), (name, counts[0], wn)
        if name != "near_1e300":                    # sums of inexact terms depend on their order: maxima and picks only
            assert np.array_equal(bits(z[0]), bits(wz)), (name, z[0], wz)
        else:
            assert np.array_equal(bits(z[0][2:]), bits(wz[2:]))
    if name == "inf_mid":
        assert math.isinf(z[0][1]) and counts[0][1] == 0 and res[0]["integrated"] == -math.inf and counts[0][0] > 0
        assert res[0]["relative_gate"] == math.inf and counts[0][3] == 0 and counts[0][2] == 24
    if name == "inf_behind_the_last_candidate":     # the range's mean is finite: every candidate is kept, none of them inf
        assert counts[0][3] == 24 and math.isfinite(z[0][5]) and math.isinf(z[0][3]) and math.isinf(z[0][2])
    if name.startswith("nan"):                      # hop 100 lies in three candidates and four momentary blocks, hop 0 in one and one
        assert np.isfinite(z[0]).all() and counts[0].tolist() == ([258, 258, 21, 21] if name == "nan_mid" else [261, 261, 23, 23])
    if name == "denormal":
        assert counts[0].tolist() == [0, 0, 0, 0] and z[0][2] > 0.0 and z[0][3] > 0.0


@pytest.mark.parametrize("fill", (math.nan, 1.0e300, math.inf))
def test_what_lies_behind_n_hops_is_not_read(amd, fill):
    for n, extra in ((260, 40), (40, 1), (3, 300), (0, 5), (2590, 10)):
        E = np.stack([F.exact(F.KINDS[s % 6], n, seed=s) for s in range(3)]) if n else np.zeros((3, 0))
        wide = np.full((3, n + extra), fill)
        wide[:, :n] = E
        res, z, counts = finish(wide, n)
        if n:
            tight = finish(E)
        else:
            tight = finish(np.zeros((3, 1)), 0)
        assert np.array_equal(bits(z), bits(tight[1])) and np.array_equal(counts, tight[2]), (n, extra)
        for s in range(3):
            same_result(res[s], tight[0][s], (n, s))
            if n:
                assert np.array_equal(counts[s], F.record(F.model(F.KINDS[s % 6], n, s))[1])


def programme(s, n):
    return F.exact(F.KINDS[s % 6], n, seed=s)


@pytest.fixture(scope="module")
def alone():
    """the record of each of 300 programmes of 40 and of 260 hops, run alone"""
    return {n: [finish(programme(s, n)) for s in range(300)] for n in (40, 260)}


@pytest.mark.parametrize("S", (1, 3, 300))
@pytest.mark.parametrize("n", (40, 260))
def test_every_stream_as_if_alone(amd, alone, S, n):
    res, z, counts = finish(np.stack([programme(s, n) for s in range(S)]))
    for s in range(S):
        r1, z1, c1 = alone[n][s]
        assert np.array_equal(bits(z[s]), bits(z1[0])) and np.array_equal(counts[s], c1[0]), s
        same_result(res[s], r1[0], s)
        wz, wn = F.record(F.model(F.KINDS[s % 6], n, s))
        assert np.array_equal(bits(z[s]), bits(wz)) and np.array_equal(counts[s], wn), s
    if S > 1:
        assert len({tuple(bits(r).tolist()) for r in z}) > 1


def test_three_streams_of_the_longest_programme(amd):
    n = 81940
    kinds = ("descending", "loud_silent_loud", "random")
    E = np.stack([F.exact(k, n, seed=1 if k != "random" else n) for k in kinds])
    res, z, counts = finish(E)
    for s, k in enumerate(kinds):
        wz, wn = F.record(F.model(f"{k}_{n}"))
        assert np.array_equal(bits(z[s]), bits(wz)) and np.array_equal(counts[s], wn), k
        assert res[s]["n_hops"] == n
    # 81949 hops in a row of 81949: the last row ends where the buffer ends
    E = np.stack([F.exact("random", 81949, seed=s) for s in range(2)])
    res, z, counts = finish(E)
    for s in range(2):
        wz, wn = F.record(F.model("random", 81949, s))
        assert np.array_equal(bits(z[s]), bits(wz)) and np.array_equal(counts[s], wn), s


def test_another_hop_length_divides_as_the_model_does(amd):
    """the same hop sums read at 8000 and 48000 Hz (H = 800, 4800): blocks are no longer dyadic, a block is one division of an exact
    sum and the maxima and picks, which depend on no order, are the model's bits; counts equal"""
    import prog_model as P
    E = F.exact("random", 2590, seed=5)
    for rate in (8000, 48000):
        res, z, counts = finish(E, rate=rate)
        want = P.finish(E, rate // 10)
        wz, wn = F.record(want)
        assert np.array_equal(counts[0], wn) and np.array_equal(bits(z[0][2:]), bits(wz[2:])), rate
        same_result(res[0], amd.loudness_finish_host(E, rate), rate)


def test_refusals_on_the_device_too(amd):
    from convopeq_amd import _capi
    res = F.refusals(_capi.load())
    assert [r for r in res if r[1] != _capi.CPQ_ERR_INVALID_ARG] == []
