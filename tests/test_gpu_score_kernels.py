"""The scorer's three kernels alone, through cpq_diag_score_spectrum / _score_lattice / _score_reduce, on inputs cpq_scorer_score
cannot produce.

Spectrum: the edge inputs of tests/score_edge_inputs.py against the reference's own verdict on them
(tests/golden/score_edges_ref.npz).  The bar is score_model.GPU_BAR_EDGE = max(8 D_EDGE, 2049 * 2^-52) = 4.55e-13 (deviation as
score_model.deviation defines it), the rule of GPU_BAR with this fixture's own measured deviation; no case is excused.  What the
7 dB tonal test and the 6 localAvg peak test decide is checked on its own: the device falls on the recording's side of every
pair that steps over them.  Table indirection, the fill of what no evaluation names and the blend are byte for byte.
Lattice and reduce: bit for bit against tests/score_model.py (and tests/lattice_model.py), at the chain counts around a wave and
the bucket counts, weights and learner boundaries the scorer's own calls never make."""
import os

import numpy as np
import pytest

import score_edge_inputs as E
import score_kernel_calls as S
import score_model as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBL_MAX = np.finfo(np.float64).max
RATES = (48000.0, 44100.0)
# the pairs that step over a decision: (passes, does not)
PAIRS = (("comb_7p5", "comb_6p5"), ("comb_7p1", "comb_6p5"), ("bump_6p5", "bump_5p5"), ("bump_6p1", "bump_5p5"), ("peaks_3_2045", "peaks_2_2046"))


def is_fill(a):
    return np.ascontiguousarray(a).tobytes() == b"\xff" * np.ascontiguousarray(a).nbytes


@pytest.fixture(scope="module")
def lib():
    import convopeq_amd  # noqa: F401
    from convopeq_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "score_edges_ref.npz"))


@pytest.fixture(scope="module")
def tables():
    return {rate: M.Tables(rate) for rate in RATES}


def case_thr(name):
    t = E.thr(name)
    return np.zeros(E.BINS) if t is None else t           # zeros: powerToDb(kMinPower) = -240 dB, below every threshold in quiet


@pytest.fixture(scope="module")
def device(lib):
    """every case of a rate in one launch, evaluation i on rows i, thr i, slot i: name -> parts [5]; and the same rows through
    thresholds_only: name -> (thr [2049], parts, blended)"""
    parts, thresholds = {}, {}
    for rate in RATES:
        names = E.cases(rate)
        rows = np.stack([E.rows(n) for n in names])
        thr = np.stack([case_thr(n) for n in names])
        evals = [(i, i, i, 0.5) for i in range(len(names))]
        rc, thr_after, p, b = S.spectrum(lib, rate, rows, thr, evals, len(names))
        assert rc == 0 and np.array_equal(thr_after, thr)                   # thr is read, not written
        rc, t_only, p2, b2 = S.spectrum(lib, rate, rows, np.full_like(thr, np.nan), evals, len(names), thresholds_only=True)
        assert rc == 0
        for i, n in enumerate(names):
            parts[n] = p[i]
            thresholds[n] = (t_only[i], p2[i], b2[i:i + 1])
    return parts, thresholds


@pytest.mark.parametrize("name", E.cases())
def test_spectrum_against_the_recording(device, fx, name):
    got, want = device[0][name], fx["members_" + name]
    dev = M.deviation(got, want)
    print(name, "device deviation", float(dev.max()), "members", got)
    assert dev.max() <= M.GPU_BAR_EDGE, (name, dev, got, want)


@pytest.mark.parametrize("a,b", PAIRS)
def test_spectrum_decisions_fall_on_the_recorded_side(device, fx, a, b):
    """wherever the recording's two outcomes differ by more than the bar, the device's differ the same way"""
    ga, gb, wa, wb = device[0][a], device[0][b], fx["members_" + a], fx["members_" + b]
    scale = np.maximum(np.abs(wa), np.abs(wb))
    scale[1:3] = 1.0
    apart = np.abs(wa - wb) > M.GPU_BAR_EDGE * np.where(scale == 0.0, 1.0, scale)
    assert apart[0] and apart[4], (a, b, wa, wb)
    assert np.array_equal(np.sign(ga - gb)[apart], np.sign(wa - wb)[apart]), (ga, gb, wa, wb)
    for g, w in ((ga, wa), (gb, wb)):                                       # and each stays with its own recording, not the other's
        assert np.all(np.abs(g - w)[apart] < 0.5 * np.abs(wa - wb)[apart])


def test_spectrum_integer_outcomes(device, fx):
    d = device[0]
    # the peak test: tonalPenalty multiplies composite_score at 6.5 localAvg and is 0 at 5.5
    assert d["bump_6p5"][4] / d["bump_6p5"][0] > 6.0 and d["bump_6p1"][4] / d["bump_6p1"][0] > 6.0 and abs(d["bump_5p5"][4] / d["bump_5p5"][0] - 1.0) < 1e-3
    # the tonal test: 73 tonal maskers at 7.5 dB, none at 6.5
    assert d["comb_6p5"][0] > 1.0e5 * d["comb_7p5"][0] and d["comb_6p5"][0] > 1.0e5 * d["comb_7p1"][0]
    # exact members: silence is 0 everywhere but for the flatness penalty's rounding, a Nyquist tone alone is all ultra-high
    assert d["nyquist"][2] == 1.0 and d["dc"][2] == 0.0 and d["silence"][[0, 2, 3, 4]].tolist() == [0.0] * 4
    assert d["silence_44k"][[0, 2, 3, 4]].tolist() == [0.0] * 4
    assert d["dc"][3] == 2.0 ** -10 and d["nyquist"][3] == 2.0 ** -10 and d["impulse_0"][3] == d["impulse_odd"][3] == 2.0 ** -14


@pytest.mark.parametrize("name", E.cases())
def test_thresholds_only(device, fx, tables, name):
    thr, parts, blended = device[1][name]
    t = tables[E.CASES[name][0]]
    assert is_fill(parts) and is_fill(blended)
    if name.startswith("silence"):
        assert np.array_equal(thr, np.maximum(t.ath_pow, 1.0e-24 * t.thr_spread))
    floor_equal, dev = M.threshold_deviation(thr, fx["thr_" + name], t) if (fx["thr_" + name] != t.ath_pow).any() else \
        (np.array_equal(thr, fx["thr_" + name]), 0.0)
    print(name, "threshold deviation", dev)
    assert floor_equal and dev <= M.GPU_BAR_EDGE, (name, dev)


def test_spectrum_table_indirection(lib, device):
    """5 evaluations over 3 row pairs and 2 thr arrays, slots permuted into 8: each slot is the same evaluation run alone, byte
    for byte; the slots no evaluation names keep the fill; thr comes back as given"""
    names = ("comb", "loud_band", "bump_6p5")
    rows = np.stack([E.rows(n) for n in names])
    thr = np.stack([np.zeros(E.BINS), E.thr("loud_band_thr")])
    evals = [(2, 0, 6, 0.3), (1, 1, 0, 0.7), (0, 0, 3, 0.5), (1, 0, 7, 1.0), (0, 1, 4, 0.0)]
    rc, thr_after, parts, blended = S.spectrum(lib, 48000.0, rows, thr, evals, 8)
    assert rc == 0 and thr_after.tobytes() == thr.tobytes()
    for r, t, s, a in evals:
        rc, _, p1, b1 = S.spectrum(lib, 48000.0, rows[r:r + 1], thr[t:t + 1], [(0, 0, 0, a)], 1)
        assert rc == 0 and parts[s].tobytes() == p1[0].tobytes() and blended[s:s + 1].tobytes() == b1.tobytes(), (r, t, s)
    for s in (1, 2, 5):
        assert is_fill(parts[s]) and is_fill(blended[s:s + 1])
    # the evaluations that used no thr array are the fixture's cases; the thr array changed the loud band's
    assert parts[3].tobytes() == device[0]["comb"].tobytes() and parts[7].tobytes() == device[0]["loud_band"].tobytes()
    assert parts[0].tobytes() == device[0]["loud_band_thr"].tobytes() != parts[7].tobytes()
    # thresholds_only through the same indirection: thr 1 from row pair 2, thr 0 untouched
    rc, t_only, p, b = S.spectrum(lib, 48000.0, rows, thr, [(2, 1, 5, 0.5)], 8, thresholds_only=True)
    assert rc == 0 and t_only[0].tobytes() == thr[0].tobytes() and t_only[1].tobytes() == device[1]["bump_6p5"][0].tobytes()
    assert is_fill(p) and is_fill(b)


@pytest.mark.parametrize("alpha", [0.0, 0.3, 0.5, 0.7, 1.0])
def test_blend_is_the_kernels_expression(lib, alpha):
    names = ("left_silent", "comb", "nyquist", "silence")
    rows = np.stack([E.rows(n) for n in names])
    rc, _, parts, blended = S.spectrum(lib, 48000.0, rows, np.zeros((1, E.BINS)), [(i, 0, i, alpha) for i in range(4)], 4)
    assert rc == 0
    a = np.float64(alpha)
    want = a * (np.sqrt(parts[:, 4] / 4096.0) * 1000.0) + (1.0 - a) * (parts[:, 3] * 1000.0)
    assert blended.tobytes() == want.tobytes(), (blended, want)


# ---------------------------------------------------------------- lattice
N_MAX = 129
SIZES = (1, 63, 64, 65, 129)


def lattice_inputs():
    """3 source rows; chain i of every size reads row i % 3 with coefficient set i and generator words i.  Set 0 sits at the
    +-0.85 clamp, set 1 is all zero, the others are counter noise within +-0.6 times a decay"""
    seg = np.stack([E.noise(20 + r, scale=2.0 ** (-1 - 2 * r))[0] for r in range(3)])
    u = E.noise(30, scale=4.0)[0][:N_MAX * 9].reshape(N_MAX, 9)              # +-1
    coef = 0.6 * u / (1.0 + 0.25 * np.arange(9))
    coef[0] = 0.85 * np.array([1, -1, 1, -1, 1, -1, 1, -1, 1.0])
    coef[1] = 0.0
    rng = np.array([[E._hash(77 + i, k) | 1 for k in range(4)] for i in range(N_MAX)], dtype=np.uint64)
    return seg, coef, rng


@pytest.fixture(scope="module")
def lattice_want():
    seg, coef, rng = lattice_inputs()
    rows = seg[np.arange(N_MAX) % 3]
    ends = sorted({0, 1} | {n - 1 for n in SIZES} | {n - 2 for n in SIZES if n > 1})[:8]      # an even number of chains for lattice_model
    return {bits: (M.lattice_errors(rows, coef, rng, bits), ends, M.lattice_model_errors(rows[ends], coef[ends], rng[ends], bits))
            for bits in (16, 24)}


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("n", SIZES)
def test_lattice_chain_counts(lib, lattice_want, n, bits):
    seg, coef, rng = lattice_inputs()
    want, ends, exact = lattice_want[bits]
    perm = [(7 * i + 3) % (n + 2) for i in range(n + 2)] if (n + 2) % 7 else [(5 * i + 3) % (n + 2) for i in range(n + 2)]
    assert sorted(perm) == list(range(n + 2))
    chains = [(i % 3, perm[i], i, i) for i in range(n)]
    rc, err = S.lattice(lib, bits, seg, n + 2, chains, coef, rng)
    assert rc == 0
    for i in range(n):
        assert err[perm[i]].tobytes() == want[i].tobytes(), (n, bits, i)
    for i in (0, n - 1):                                                    # the first and the last chain against lattice_model.py
        assert i in ends and err[perm[i]].tobytes() == exact[ends.index(i)].tobytes(), (n, bits, i)
    assert is_fill(err[perm[n]]) and is_fill(err[perm[n + 1]])


# ---------------------------------------------------------------- reduce
COUNTS = ([4, 4, 4, 4], [4, 4, 2, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0])
WEIGHTS = ((0.4, 0.3, 0.2, 0.1), (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 0.0))


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("n_learners,n_cand", [(1, 1), (1, 64), (5, 13), (3, 43)])
def test_reduce(lib, n_learners, n_cand, weights):
    """every learner has its own counts (a wrong pair / n_cand shows), learner boundaries fall inside a wave (5 x 13, 3 x 43)"""
    pairs = n_learners * n_cand
    for shift in range(len(COUNTS) if n_learners == 1 else 1):              # one learner: every count set in turn
        counts = [COUNTS[(l + shift) % len(COUNTS)] for l in range(n_learners)]
        blended = 1.0 + E.noise(40 + pairs)[0][:pairs * 16].reshape(pairs, 16) * 2.0 ** 12
        state = np.zeros(pairs, dtype=np.int32)
        state[::7] = 1
        state[3::11] = 2                                                    # only 1 means refused
        blended[0, 5] = np.nan                                              # pair 0 is refused: whatever blended holds
        rc, scores = S.reduce(lib, n_learners, n_cand, counts, state, blended, weights)
        assert rc == 0
        for pair in range(pairs):
            want = 1e18 if state[pair] == 1 else M.combine(blended[pair].tolist(), counts[pair // n_cand], weights)
            assert scores[pair:pair + 1].tobytes() == np.array([want]).tobytes(), (n_learners, n_cand, pair, counts[pair // n_cand], scores[pair], want)
            if state[pair] != 1 and (sum(counts[pair // n_cand]) == 0 or sum(w for w, c in zip(weights, counts[pair // n_cand]) if c) <= 0.0):
                assert scores[pair] == DBL_MAX


def test_refusals(lib):
    """every rule of the header, by code and message, with a device present too; and the valid sets run"""
    S.check_refusals(lib)
    assert S.valid_calls(lib) == [0] * 4
