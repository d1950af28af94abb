"""Every input of tests/meter_edge_inputs.py does, on the model alone, what its GPU test (test_gpu_meter_edges.py) relies on:
the model's maximum of a callback sits where the kernel could go wrong, a peak arrives callbacks after its sample, a callback
lies over three spans.  No GPU, no library: meter_model.py and numpy."""
import numpy as np
import pytest

import meter_edge_inputs as E
import meter_model as M

FLOOR_PEAK = 1e-3           # a callback of 1e-4 noise alone peaks far below this; a planted 0.9 far above


def test_planted_shapes_put_the_maximum_where_the_docstring_says():
    cb = 256
    for shape, off in ((E.IMP, 61), (E.PAIR, 58)):
        x = np.stack([E.planted(cb, cb, [(0, 100)], shape, 1e-6, seed=1), np.zeros(cb)])
        peak, at, ch = E.peak_trace(x, cb)[0]
        assert (at, ch) == (4 * 100 + off, 0), (shape, at)
    assert abs(E.peak_trace(np.stack([E.planted(cb, cb, [(0, 100)], E.IMP, seed=2), np.zeros(cb)]), cb)[0][0] - E.LOBE) < 1e-3


@pytest.mark.parametrize("cb", (1024, 1536))
def test_seam_case_surrounds_every_seam(cb):
    x, what = E.seam_case(cb)
    assert x.shape == (2 * len(what), 4 * cb) and len(what) == 32 * (cb // E.TILE - 1)
    at = {}
    for s, (t0, shape, p) in enumerate(what):
        tr = E.peak_trace(x[2 * s:2 * s + 2], cb)
        assert tr[1][1:] == tr[3][1:] and tr[1][2] == p % 2                 # both calls, on the planted channel
        assert tr[1][0] > 0.25 and max(tr[0][0], tr[2][0]) < 1e-4            # the floor of this case is 1e-6
        at.setdefault(t0, []).append(tr[1][1])
    assert sorted(at) == list(range(E.TILE, cb, E.TILE))
    for t0, idx in at.items():
        before = {i for i in idx if 4 * t0 - 32 <= i < 4 * t0}
        after = {i for i in idx if 4 * t0 <= i < 4 * t0 + 32}
        assert len(before) >= 8 and len(after) >= 8, (t0, sorted(idx))
        for side in (before, after):
            assert {i % 2 for i in side} == {0, 1}, (t0, sorted(side))
        # the outputs whose stage-1 window reaches the last stage-0 pair of the tile's halo: 4 t0 - 4, - 2 and - 1
        assert before & {4 * t0 - 4, 4 * t0 - 2, 4 * t0 - 1}, sorted(before)


@pytest.mark.parametrize("cb", (516, 520, 1000))
def test_short_tile_case_peaks_where_it_says(cb):
    x, want = E.short_tile_case(cb)
    assert (cb + E.TILE - 1) // E.TILE == 2 and x.shape == (6, 4 * cb)
    for s, (lo, hi) in enumerate(want):
        tr = E.peak_trace(x[2 * s:2 * s + 2], cb)
        for k in (1, 3):
            assert lo <= tr[k][1] < hi and tr[k][2] == 0 and tr[k][0] > 0.25, (s, k, tr[k], lo, hi)
    assert want[0][0] == 4 * 512 * (2 - 1)


@pytest.mark.parametrize("cb", (64, 128, 512))
def test_end_case_cuts_the_lobe_and_hands_it_on(cb):
    x, plants = E.end_case(cb)
    T = 3
    assert plants[0] % T == 0 and plants[1] % T >= 1 and plants[1] // T >= 1 and plants[2] % T == T - 1
    assert x.shape == (40, 4 * T * cb)
    for i, back in enumerate(E.END_BACKS):
        tr = E.peak_trace(x[2 * i:2 * i + 2], cb)
        for k in plants:
            if back <= 15:
                assert FLOOR_PEAK < tr[k][0] < E.LOBE - 1e-3, (back, k, tr[k])         # the zero future cuts the main lobe off
                assert tr[k + 1][0] > FLOOR_PEAK, (back, k)                  # and the next callback inherits the rest
            else:
                assert abs(tr[k][0] - E.LOBE) < 1e-3 and tr[k][1] == 4 * (cb - back) + 61, (back, k, tr[k])
            assert tr[k][2] == i % 2


@pytest.mark.parametrize("cb", E.TINY_CBS)
def test_tiny_case_peaks_arrive_late(cb):
    x, plants = E.tiny_case(cb)
    K = x.shape[1] // cb
    assert K == 4 * E.TINY_T and K * cb == x.shape[1]
    offsets = {p for _, p in plants[0]}
    assert len(offsets) >= min(cb, 8) and all(0 <= p < cb for p in offsets)
    for s in range(2):
        tr = E.peak_trace(x[2 * s:2 * s + 2], cb)
        has = {k for k, _ in plants[s]}
        late = [k for k in range(2, K) if k not in has and k - 1 not in has and tr[k][0] > FLOOR_PEAK]
        if cb <= 16:
            assert late, "no callback's peak comes from an impulse planted two or more callbacks earlier"
            assert all(k - 2 in has or k - 3 in has for k in late)
        if cb == 8:
            assert any(tr[k][0] > 0.25 for k in late)                        # the main lobe itself, two callbacks on
        assert sum(tr[k][0] > FLOOR_PEAK for k in range(K)) >= len(has)


def test_sided_case_keeps_the_neighbours_quiet():
    cb = 1024
    x, hot = E.sided_case(cb)
    assert hot == (1, 4)
    for s in range(6):
        tr = E.peak_trace(x[2 * s:2 * s + 2], cb)
        if s in hot:
            assert all(tr[k][0] > 0.25 and tr[k][2] == (0 if s == 1 else 1) for k in (1, 2, 3)), tr
            assert 4 * E.TILE - 8 <= tr[1][1] < 4 * E.TILE
        else:
            assert max(t[0] for t in tr) < FLOOR_PEAK
    assert not np.array_equal(x[2], x[3])


def test_long_call_case_crosses_the_finish_chunk_and_the_ring():
    x = E.long_call_case()
    B, T = E.LONG_B, E.LONG_T
    assert T > 2 * E.FINISH_CHUNK and x.shape == (4, 2 * T * B) and 2 * T * B >= 4096
    # the ring: 2056 pushed, 100 popped, 2056 pushed -- none dropped, and the write position passes 4095 -> 0
    ring = M.Ring()
    assert all(ring.push(k) for k in range(T))
    assert [ring.pop() for _ in range(100)] == list(range(100))
    assert all(ring.push(T + k) for k in range(T))
    assert ring.w - T <= M.RING - 1 < ring.w - 1
    # the hold that enters callbacks 1024 and 2048 of each call is above the peak found there: a chain restarted at a chunk
    # would return another hold
    for s in range(2):
        tr = E.peak_trace(x[2 * s:2 * s + 2], B)
        hold = M.hold_replay([t[0] for t in tr])
        for call in range(2):
            for c in (E.FINISH_CHUNK, 2 * E.FINISH_CHUNK):
                k = call * T + c
                assert hold[k - 1] * 0.999 > tr[k][0] and hold[k] == hold[k - 1] * 0.999, (s, k)
        assert hold[T - 1] > tr[T][0]                                         # and across the calls


def test_three_span_callbacks_exist():
    for B, (calls, ragged) in E.THREE_SPAN.items():
        assert all(n == 3 * B for n in calls) and sum(calls) >= 4096
        assert max(E.span_counts(calls, B)) == 3, B
        if ragged:
            assert max(E.span_counts(ragged, B)) == 3 and max(ragged) <= 3 * B and any(n % B for n in ragged)
    # [6000, 9000) of a call of 9000 lies over the spans from 4096, 6144 and 8192
    assert E.span_counts([9000], 3000) == [2, 2, 3]
    assert E.span_counts([2048, 2049], 4096) == [1, 2]


def test_call_lists():
    for B in E.MANY_BLOCKS:
        calls = E.many_calls(B)
        assert all(2500 <= n <= 4100 for n in calls) and sum(calls) >= 4096
        assert max((n + B - 1) // B for n in calls) <= M.RING                # a read follows every call
    for calls in (E.CARRY_CALLS, E.CARRY_CALLS_ONES_LAST):
        assert 4096 <= sum(calls) and max(calls) <= 16 * 512
    assert sum(E.CARRY_CALLS) + sum(E.CARRY_CALLS_ONES_LAST) < 30000
    assert E.CARRY_CALLS_ONES_LAST[-3:] == [1, 1, 1] and 1 not in E.CARRY_CALLS_ONES_LAST[:-3]
    assert E.CARRY_CALLS == [1, 2, 7, 8, 9, 15, 16, 17, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097]


def test_scrub_case_sits_on_the_carries():
    x, calls, spots = E.scrub_case()
    assert x.shape == (4, sum(calls)) and sum(calls) >= 4096
    start = np.concatenate([[0], np.cumsum(calls)])
    rel = [(int(np.searchsorted(start, at, side="right")) - 1, int(at)) for at in spots]
    where = {(c, at - int(start[c]), at - int(start[c]) - calls[c]) for c, at in rel}
    assert {(0, 999, -1), (0, 998, -2), (2, 2499, -1), (2, 2498, -2)} <= where              # a call's last two samples
    assert {(c, o) for c, o, _ in where if o in (2046, 2047, 2048)} >= {(1, 2046), (1, 2047), (1, 2048), (2, 2046), (2, 2047)}
    bad = ~(np.isfinite(x) & (np.abs(x) < 1e300))
    assert bad.sum() == 4 * len(spots) and bad[:, spots].all()
    for r in range(4):                                                       # every row gets every value
        vals = x[r, spots]
        assert np.isnan(vals).any() and (vals == np.inf).any() and (vals == 1e300).any() and (vals == -1.5e300).any()
    clean = M.scrub(x)
    assert np.isfinite(clean).all() and not clean[:, spots].any()
    assert start[-1] - max(spots) > 600                                      # calls follow that have to stay finite
