"""The scorer's numpy model (tests/score_model.py) against the reference's own verdict on the edge inputs
(tests/golden/score_edges_ref.npz, recorded by tests/golden/make_score_edges_ref.py from tests/score_edge_inputs.py): silence, one
silent channel, single bins at both ends of the transform's split, a wholly consumed Bark band, the densest combs, steps over the
7 dB tonal test and the 6 localAvg peak test, a thr array that dominates.  The model is held to D_EDGE, its own measured deviation
rounded up; the caps and counts it reports are pinned, so that the device test knows what each case exercises.  And the three
cpq_diag_score_* entries refuse every bad argument set before they look for a device."""
import os

import numpy as np
import pytest

import score_edge_inputs as E
import score_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "score_edges_ref.npz"))


@pytest.fixture(scope="module")
def tables():
    return {rate: M.Tables(rate) for rate in (48000.0, 44100.0)}


@pytest.fixture(scope="module")
def results(tables):
    return {n: M.evaluate(E.rows(n), E.thr(n), tables[E.CASES[n][0]]) for n in E.cases()}


def test_the_bar_follows_the_recorded_deviation(fx):
    worst = max(float(fx["d_edge_" + n]) for n in E.cases())
    print("largest recorded d_edge", worst)
    assert worst <= M.D_EDGE <= 10.0 * M.D_REF and M.D_EDGE < 1.1 * worst          # rounded up, not widened
    assert M.GPU_BAR_EDGE == max(8.0 * M.D_EDGE, 2049.0 * 2.0 ** -52)
    assert sorted(k[8:] for k in fx.files if k.startswith("members_")) == sorted(E.cases())


@pytest.mark.parametrize("name", E.cases())
def test_model_against_the_recording(fx, tables, results, name):
    res, t = results[name], tables[E.CASES[name][0]]
    dev = M.deviation(res.array(), fx["members_" + name])
    print(name, "deviation", float(dev.max()), "recorded d_edge", float(fx["d_edge_" + name]), "caps", res.caps, "softplus", res.branches)
    assert dev.max() <= M.D_EDGE, (name, dev)
    assert res.margin > float(fx["margin"])
    want = fx["thr_" + name]
    got = M.masking_thresholds(E.rows(name), t)
    if (want == t.ath_pow).all():
        assert np.array_equal(got, want)
    else:
        floor_equal, d = M.threshold_deviation(got, want, t)
        assert floor_equal and d <= 10.0 * M.D_REF, (name, d)


def test_what_the_cases_exercise(fx, results):
    """the counts the issue of these tests states, on the model the recording has just confirmed"""
    caps = {n: (r.caps["tonal"], r.caps["bands"], r.caps["maskers"]) for n, r in results.items()}
    assert caps["peak_4"] == (1, 23, 24) and results["peak_4"].caps["consumed"] == 9          # band 0 = bins 0..8, all absorbed
    assert caps["peaks_3_2045"] == (2, 24, 26) and caps["peaks_2_2046"] == (0, 24, 24)
    assert caps["comb"] == (100, 10, 110) and caps["comb_44k"] == (99, 11, 110) and caps["comb_thinned"] == (96, 16, 112)
    assert caps["comb_7p5"][0] == caps["comb_7p1"][0] == 73 and caps["comb_6p5"][0] == 0
    for n in ("tone_1", "tone_2", "tone_2046", "tone_2047", "silence", "dc", "nyquist"):
        assert caps[n] == (0, 24, 24), n
    m = {n: fx["members_" + n] for n in E.cases()}
    assert m["nyquist"][2] == 1.0 and m["dc"][2] == 0.0                                        # hf_penalty
    assert m["silence_44k"].tolist() == [0.0] * 5 and m["silence"].tolist() == [0.0] * 5         # (the model's pairwise sums leave 1.7e-14)
    assert results["silence"].caps["min_energy"] < 1.0e-20                                      # every band at 24 kMinPower-sized bins
    # the peak test: tonalPenalty multiplies composite at 6.5 localAvg and not at 5.5
    assert m["bump_6p5"][4] / m["bump_6p5"][0] > 6.0 and m["bump_6p1"][4] / m["bump_6p1"][0] > 6.0 and abs(m["bump_5p5"][4] / m["bump_5p5"][0] - 1.0) < 1e-3
    # the tonal test: 73 tonal maskers at 7.5 dB hold noise_power six orders under the same comb at 6.5 dB
    assert m["comb_6p5"][0] > 1.0e5 * m["comb_7p5"][0]
    assert m["loud_band_thr"][0] < 0.6 * m["loud_band"][0]                                     # thr dominates where noise_power comes from
    # softplus: exp and log1p branches both occur; no input reaches x (zz > 50): the cap that could strip a band of its masker is
    # out of a comb's reach (cap_search)
    assert all(r.branches[0] == 0 for r in results.values())
    assert results["silence"].branches == (0, 0, 2049) and results["loud_band"].branches[1] > 0 and results["loud_band"].branches[2] > 0


def test_masker_candidates_stay_below_the_cap():
    """the bounded search of make_score_edges_ref.py at the fixture's rate: 112 candidates, and the thinned comb is its placement"""
    n, peaks = E.cap_search(48000.0)
    assert n == 112 and tuple(peaks) == E.THINNED_48K


def test_score_diagnostics_refuse_before_looking_for_a_device():
    import torch
    import score_kernel_calls as S
    from convopeq_amd import _capi
    lib = _capi.load()
    S.check_refusals(lib)
    assert {e for e, _, _, _ in S.REFUSALS} == {"spectrum", "lattice", "reduce"}
    if not torch.cuda.is_available():
        assert S.valid_calls(lib) == [S.NO_DEVICE] * 4
