"""The kernels of convopeq_amd/csrc/mix_kernels.hip in isolation, through the diagnostic entries cpq_diag_direct_head, _agc,
_ring_chunks, _convproc_mix, _tail_reader and _rows: the launchers an engine calls, on buffers this file fills, so that the
shapes, strides, positions and flags are chosen here and not by an engine.  Reference: tests/mix_model.py, plain numpy and
Python written from the reference's description of each operation (checked without a GPU in tests/test_mix_model_cpu.py).

Every assertion is BIT EQUALITY (uint64 views, so NaN payloads and -0.0 count): the library is built with -ffp-contract=off,
its only fused operations are the written fma() calls of the direct head and the RMS, and the model fuses at the same places
with an exactly rounded rational.  A misplaced sample, a swapped gain, a fused or unfused operation changes bits.  Whatever
the model says a launch does not store must still hold the entry's 0xFF prefill (or the contents this file supplied).

Inputs are standard-normal unless said.  The 16384 + 257 sizes take a second, partial grid-stride trip (64 x 256 threads);
there the direct head runs on small integers (every product and sum exact, so only placement is modelled, vectorised).

Kernels and a case that runs each:
  k_direct_head          test_direct_head_taps[*], test_direct_head_lengths[*], test_direct_head_flush, _two_calls[*]
  k_rows_add             test_direct_head_lengths[*] (out_stride > n)
  k_agc_block_rms        test_agc_rms[*]
  k_agc_gains            test_agc_gains_table, test_agc_gains_two_calls
  k_agc_ramp             test_agc_gains_table (launch_agc_apply), test_gain_ramp[*] (launch_gain_ramp)
  k_block_silence        test_block_silence[*]
  k_rows_gather_multi    test_gather[*]
  k_ring_chunks<true>    test_ring_chunks[*] (op get; fused, with and without ring B)
  k_ring_chunks<false>   test_ring_chunks[*] (op add, op add2)
  k_convproc_mix         test_convproc_mix[*], test_convproc_mix_null_lengths, test_put_then_mix
  k_ring_put             test_put_then_mix
  k_ring_regrow          test_ring_regrow[*]
  k_tail_schedule        test_tail_schedule[*], test_tail_one_call_equals_sixteen
  k_tail_append          test_tail_append[*]
  k_rows_copy            test_rows_copy[*]
  k_rows_scale           test_rows_scale
  k_bypass_blend         test_bypass_blend[*]
and test_valid_base_sets_run runs every valid argument set of the refusal table (tests/mix_kernel_calls.py) for real.

Measured on an MI355X: 188 tests, every case equal, 3.6 s for the whole file.  test_agc_gains_two_calls failed before
k_agc_gains kept the gain itself in its state (it kept gain - 1, and (gain - 1) + 1 is not the gain below 0.5): RESULTS.md."""
import numpy as np
import pytest

import mix_kernel_calls as K
import mix_model as M

pytestmark = pytest.mark.gpu

BIG = 16384 + 257


@pytest.fixture(scope="module")
def amd():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need a gfx950 device")
    import convopeq_amd
    return convopeq_amd


@pytest.fixture(scope="module")
def lib(amd):
    from convopeq_amd import _capi
    return _capi.load()


def eq(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.float64:
        bad = got.view(np.uint64) != np.ascontiguousarray(want, dtype=np.float64).view(np.uint64)
    else:
        bad = got != want
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {at}: got {got[at]!r}, expected {want[at]!r}")


def ok(rc):
    assert rc == 0, rc


# ---------------------------------------------------------------------------------------------------------------- direct head
NT = [0, 1, 3, 7, 8, 9, 15, 16, 17, 24, 31, 32]


def head_case(rng, n, nt, pad=3, integers=False):
    """4 channels; slot 1 is named by nobody and holds poison; channels 0 and 3 share slot 2; stream 1 (channels 2, 3) may rest"""
    draw = (lambda s: rng.integers(-8, 9, s).astype(np.float64)) if integers else rng.standard_normal
    x = K.ff((4, n + pad))
    x[:, :n] = draw((4, n))
    ir = np.full((4, 32), np.nan)
    taps = np.array([nt, 32, nt, max(nt - 1, 0)], dtype=np.int32)
    for s in (0, 2, 3):
        ir[s, :taps[s]] = draw(int(taps[s]))
    return x, ir, taps, np.array([2, 0, 3, 2], dtype=np.int32), draw((4, 32))


@pytest.mark.parametrize("nt", NT)
def test_direct_head_taps(lib, nt):
    """every tap count at n = 33 (more samples than taps: both sides of p < 0) and n = 5 (n < nt - 1: history only, and the
    history shift with n < 32); NaN behind the n samples of a row, NaN in the taps above nt and in the unused slot"""
    rng = np.random.default_rng(100 + nt)
    for n in (33, 5):
        x, ir, taps, slot, hist = head_case(rng, n, nt)
        rc, o = K.direct_head(lib, x, ir, taps, slot, hist, n=n)
        ok(rc)
        dout, hnew = M.direct_head(x[:, :n], ir, taps, slot, hist)
        eq(o["dout"], dout, f"dout nt {nt} n {n}")
        eq(o["hist_new"], hnew, f"hist_new nt {nt} n {n}")


@pytest.mark.parametrize("n", [1, 5, 31, 32, 33, 255, 256, 257, BIG])
def test_direct_head_lengths(lib, n):
    """every length at nt = 32 and 9; stream 1 rests (wet_on = 0: zeros, history kept); dout added into out rows with
    out_stride > n, whose tails keep their contents.  BIG: integers (exact), second grid-stride trip."""
    rng = np.random.default_rng(200 + n)
    for nt in (32, 9):
        x, ir, taps, slot, hist = head_case(rng, n, nt, integers=n == BIG)
        out = rng.standard_normal((4, n + 5)) if n != BIG else rng.integers(-8, 9, (4, n + 5)).astype(np.float64)
        rc, o = K.direct_head(lib, x, ir, taps, slot, hist, n=n, wet_on=[1, 0], out=out)
        ok(rc)
        if n == BIG:
            dout = M.direct_head_exact(x[:, :n], ir, taps, slot, hist)
            dout[2:] = 0.0
            hnew = np.concatenate([hist, x[:, :n]], axis=1)[:, -32:]
            hnew[2:] = hist[2:]
        else:
            dout, hnew = M.direct_head(x[:, :n], ir, taps, slot, hist, wet_on=[1, 0])
        eq(o["dout"], dout, f"dout n {n} nt {nt}")
        eq(o["hist_new"], hnew, f"hist_new n {n} nt {nt}")
        want = out.copy()
        want[:, :n] = out[:, :n] + dout
        eq(o["out"], want, f"rows_add n {n}")


def test_direct_head_flush(lib):
    """outputs just below and just above 1e-20 (one tap: y = h * x exactly rounded), an Inf input (non-finite: 0), and a
    NaN-producing 0 * Inf"""
    below, above = np.nextafter(1.0e-20, 0.0), np.nextafter(1.0e-20, 1.0)
    x = np.array([[below, above, -below, -above, 1.0e-20, np.inf, 1.0, 0.0]] * 2)
    ir = np.zeros((2, 32))
    ir[0, 0] = 1.0
    ir[1, :3] = [1.0, -1.0, 0.0]                  # three taps: Inf next to finite samples, then 0 * Inf = NaN
    rc, o = K.direct_head(lib, x, ir, [1, 3], [0, 1], np.zeros((2, 32)))
    ok(rc)
    dout, hnew = M.direct_head(x, ir, [1, 3], [0, 1], np.zeros((2, 32)))
    assert list(dout[0]) == [0.0, above, 0.0, -above, 1.0e-20, 0.0, 1.0, 0.0]
    eq(o["dout"], dout, "flush")
    eq(o["hist_new"], hnew, "flush history")


@pytest.mark.parametrize("n1,n2", [(5, 40), (40, 5), (1, 1)])
def test_direct_head_two_calls(lib, n1, n2):
    rng = np.random.default_rng(n1 * 100 + n2)
    x, ir, taps, slot, hist = head_case(rng, n1 + n2, 32, pad=0)
    _, whole = K.direct_head(lib, x, ir, taps, slot, hist)
    _, a = K.direct_head(lib, x[:, :n1], ir, taps, slot, hist)
    rc, b = K.direct_head(lib, x[:, n1:], ir, taps, slot, a["hist_new"])
    ok(rc)
    eq(np.concatenate([a["dout"], b["dout"]], axis=1), whole["dout"], "two calls")
    eq(b["hist_new"], whole["hist_new"], "two calls history")
    eq(whole["dout"], M.direct_head(x, ir, taps, slot, hist)[0], "one call")


# ------------------------------------------------------------------------------------------------------------------------ AGC
RMS_CASES = [(B, 17, 1) for B in (1, 3, 4, 5, 63, 64, 66, 441, 512)] + \
            [(B, nc, T) for B in (5, 66) for nc, T in ((1, 1), (3, 5), (5, 3), (2, 8), (16, 1), (1, 17), (3, 11), (11, 3))]


@pytest.mark.parametrize("B,nc,T", RMS_CASES, ids=[f"B{B}-{nc}x{T}" for B, nc, T in RMS_CASES])
def test_agc_rms(lib, B, nc, T):
    """B % 4 != 0: the scalar remainder; nCh * T = 1, 15, 16, 17, 33: dead groups beside live ones in the last wave"""
    rng = np.random.default_rng(B * 1000 + nc * 31 + T)
    data = K.ff((nc, B * T + 3))
    data[:, :B * T] = rng.standard_normal((nc, B * T))
    rc, o = K.agc(lib, 0, data, B, T)
    ok(rc)
    want = np.array([[M.block_rms(data[c, t * B:(t + 1) * B]) for t in range(T)] for c in range(nc)])
    eq(o["rms"], want, "rms")
    eq(o["data"], data, "data")


def gains_table():
    """[S = 7][T] hand-built RMS sequences (both channels of a stream: the second carries the smaller or a NaN value)"""
    nan, inf = np.nan, np.inf
    rin = [[1.0, 1.0, 1.05, 1.07, 0.7, 0.86, 0.95, 1.0],                 # ratios inside and just outside both dead-band edges
           [0.01, 0.01, 0.01, 40.0, 40.0, 40.0, 0.5, 0.5],               # ratio below 0.06, then above 16
           [1.0e-6, 2.0e-6, 0.9e-6, 1.1e-6, 1.0e-6, 1.0e-6, 3e-6, 1e-7],   # envOut around 1e-6
           [5.0e-20, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],                # envelopes decaying below 1e-20
           [nan, inf, 1001.0, 1000.0, 0.5, nan, 2.0, 0.1],               # NaN, Inf, above 1000
           [0.3, 0.6, 0.2, 0.9, 0.1, 0.5, 0.5, 0.5],                     # attack against release on either side
           [0.3, 0.6, 0.2, 0.9, 0.1, 0.5, 0.5, 0.5]]                     # this stream is off
    rout = [[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
            [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
            [0.9e-6, 1.1e-6, 2.0e-6, 0.5e-6, 1.0e-6, 1.0e-6, 1e-7, 3e-6],
            [5.0e-20, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
            [1.0, nan, 0.5, inf, 1001.0, 1.0, nan, 0.2],
            [0.5, 0.1, 0.9, 0.2, 0.6, 0.3, 0.5, 0.5],
            [0.5, 0.1, 0.9, 0.2, 0.6, 0.3, 0.5, 0.5]]
    S, T = len(rin), len(rin[0])
    full = lambda r: np.array([[r[c // 2][t] if c % 2 == 0 else (np.nan if t % 3 == 0 else 0.5 * r[c // 2][t]) for t in range(T)]
                               for c in range(2 * S)])
    state = np.array([[1.0, 1.0, 1.0], [0.02, 1.0, 0.1], [1.0e-6, 1.0e-6, 1.5], [3.0e-20, 3.0e-20, 1.0], [0.5, 0.5, 1.0], [0.4, 0.4, 1.25],
                      [0.4, 0.4, 1.25]])
    return full(rin), full(rout), state, np.array([1, 1, 1, 1, 1, 1, 0], dtype=np.int32), S, T


COEF = (0.75, 0.25, 0.5)


@pytest.mark.parametrize("B", [5, 64])
def test_agc_gains_table(lib, B):
    """k_agc_gains on the branch table, then k_agc_ramp with those gains; the stream that is off keeps state, gains (0xFF) and data"""
    rin, rout, state, on, S, T = gains_table()
    rng = np.random.default_rng(B)
    data = rng.standard_normal((2 * S, B * T + 2))
    rc, o = K.agc(lib, 1, data, B, T, rms_in=rin, rms_out=rout, state=state, on=on, coef=COEF)
    ok(rc)
    st, gains = M.agc_gains(rin, rout, state, on, T, B, *COEF)
    eq(o["state"], st, "state")
    eq(o["gains"], gains, "gains")
    targets = gains[:6, :, 1] * B / 0.5 + gains[:6, :, 0]           # the table does cross the branches (not asserted bit-wise)
    edge = 1.0 / 1.059            # a passed-through ratio just outside either edge of the dead band, and far ones
    assert ((targets[0] > 1.059) & (targets[0] < 1.07)).any() and ((targets[0] < edge) & (targets[0] > edge - 0.01)).any()
    assert ((targets[5] > 1.1) & (targets[5] < 15.0)).any() and ((targets[5] < 0.9) & (targets[5] > 0.07)).any()
    assert (np.abs(targets - 1.0) < 1e-9).any() and (np.abs(targets - 16.0) < 1e-9).any() and (np.abs(targets - 0.06) < 1e-6).any()
    assert K.untouched(gains[6]) and (st[:, :2] == 0.0).any()
    want = M.gain_ramp(data[:, :B * T], gains, on, B, T)
    eq(o["data"][:, :B * T], want, "ramped data")
    eq(o["data"][:, B * T:], data[:, B * T:], "behind the call")
    eq(o["data"][12:], data[12:], "stream that is off")


def test_agc_gains_two_calls(lib):
    rin, rout, state, on, S, T = gains_table()
    B = 16
    data = np.ones((2 * S, B * T))
    _, whole = K.agc(lib, 1, data, B, T, rms_in=rin, rms_out=rout, state=state, on=on, coef=COEF)
    _, a = K.agc(lib, 1, data[:, :B * 3], B, 3, rms_in=rin[:, :3], rms_out=rout[:, :3], state=state, on=on, coef=COEF)
    rc, b = K.agc(lib, 1, data[:, B * 3:], B, T - 3, rms_in=rin[:, 3:], rms_out=rout[:, 3:], state=a["state"], on=on, coef=COEF)
    ok(rc)
    eq(b["state"], whole["state"], "carried state")
    eq(np.concatenate([a["gains"], b["gains"]], axis=1), whole["gains"], "carried gains")
    eq(np.concatenate([a["data"], b["data"]], axis=1), whole["data"], "carried data")


RAMP_CASES = [(1, 1), (1, 255), (3, 85), (1, 256), (4, 64), (1, 257), (17, 15), (64, 4), (64, 133), (441, 19), (441, 37), (512, 16),
              (512, 33), (17, 500), (3, 5462), (4, 2123)]      # B * T: 1, 255, 256, 257, 8492 (second trip), > 16384 (third trip)


@pytest.mark.parametrize("B,T", RAMP_CASES, ids=[f"B{B}xT{T}" for B, T in RAMP_CASES])
def test_gain_ramp(lib, B, T):
    """launch_gain_ramp: 32 x 256 threads, so B * T above 8192 takes further (partial) trips; S = 2 with on = 10, 01, 11 and S = 3
    with on = 110, 011, 111 (every stream on and off beside a live one)"""
    rng = np.random.default_rng(B * 7 + T)
    pats = ([1, 0], [0, 1], [1, 1], [1, 1, 0], [0, 1, 1], [1, 1, 1])[(B + T) % 2::2]
    for on in pats if B * T <= 4096 else pats[1:2]:
        S = len(on)
        data = K.ff((2 * S, B * T + 1))
        data[:, :B * T] = rng.standard_normal((2 * S, B * T))
        gains = np.stack([1.0 + 0.1 * rng.standard_normal((S, T)), 1e-3 * rng.standard_normal((S, T))], axis=-1)
        rc, o = K.agc(lib, 2, data, B, T, gains=gains, on=on)
        ok(rc)
        want = data.copy()
        want[:, :B * T] = M.gain_ramp(data[:, :B * T], gains, on, B, T)
        eq(o["data"], want, f"on {on}")


@pytest.mark.parametrize("B", [1, 63, 64, 65, 441])
def test_block_silence(lib, B):
    """threshold: |x| > 1e-8 is loud; exactly 1e-8 and NaN are not.  Callback t of stream s holds one candidate at index
    0, 63, 64 or B - 1 of channel 0 or channel 1; the other stream stays silent."""
    thr, up = 1.0e-8, np.nextafter(1.0e-8, 1.0)
    cases = [(v, i, ch) for v in (thr, up, -up, np.nan, -thr) for i in sorted({0, min(63, B - 1), min(64, B - 1), B - 1}) for ch in (0, 1)]
    T = len(cases)
    data = np.zeros((4, B * T + 1))
    data[:, -1] = 1.0                                # behind the call: must not be read
    for t, (v, i, ch) in enumerate(cases):
        data[2 * (t % 2) + ch, t * B + i] = v
    rc, o = K.agc(lib, 3, data, B, T)
    ok(rc)
    want = M.block_silence(data[:, :B * T], 2, B, T)
    assert want.sum() < want.size and [want[t % 2, t] for t, c in enumerate(cases) if c[0] in (up, -up)].count(0) == 2 * T // 5
    eq(o["silent"], want, "silent")


# ---------------------------------------------------------------------------------------------------------------- ring chunks
CH_MAP = [2, -1, 5, 0]
GAINS = [1.0, 1.0 + 5e-13, 1.0 + 2e-12, 0.5, -0.0]


def chunk_sizes():
    for q in (1, 64, 441, 512):
        for n in sorted({1, max(q - 1, 1), q, q + 1, 3 * q + 7}):
            yield q, n
    yield 441, BIG
    yield 512, BIG


CHUNK_CASES = list(chunk_sizes())


@pytest.mark.parametrize("q,n", CHUNK_CASES, ids=[f"q{q}-n{n}" for q, n in CHUNK_CASES])
def test_ring_chunks(lib, q, n):
    """get, add, add2 and the fused get-add (with and without ring B) on one set of tables: rows 1, 3, 4 of 6 and the -1 slot
    are left alone; ring sizes 2, 512 and 2048 with positions that wrap inside a chunk; cnt in {0, 1, q - 1, q}; schedules mix
    -1 and >= 0 independently per layer; one gain pair per case out of 1, 1 + 5e-13 (unity branch), 1 + 2e-12, 0.5, -0.0"""
    rng = np.random.default_rng(q * 100003 + n)
    n_cb = (n + q - 1) // q
    sizes = [(2, 512, 2048), (512, 2048, 2), (2048, 2, 512)][(q + n) % 3]
    ring0, ring_a, ring_b = (rng.standard_normal((4, s)) for s in sizes)
    pos = [int(rng.integers(0, 1 << 41)) if i % 2 else sizes[0] - 1 + (i % 3) for i in range(n_cb)]
    cnt = [[0, 1, max(q - 1, 0), q][(i + n) % 4] for i in range(n_cb)]
    sched_a = [-1 if i % 3 == 1 else (sizes[1] - 2 + i if i % 2 else int(rng.integers(0, 1 << 41))) for i in range(n_cb)]
    sched_b = [-1 if i % 4 in (1, 2) else sizes[2] - 1 + 5 * i for i in range(n_cb)]           # chunk 0: both layers
    ga, gb = GAINS[(q + n) % 5], GAINS[(q + 2 * n + 1) % 5]
    out = K.ff((6, n + 3))
    out[CH_MAP[0]] = rng.standard_normal(n + 3)            # rows with contents for the adds; row 5 of ch_map[2] keeps 0xFF
    out[CH_MAP[3]] = rng.standard_normal(n + 3)
    out[1] = 3.0

    def tail_kept(o):
        eq(o["out"][:, n:], out[:, n:], "behind n")
        eq(o["out"][[1, 3, 4]], out[[1, 3, 4]], "rows no channel names")

    rc, get = K.ring_chunks(lib, K.GET, out, CH_MAP, n, q, ring0=ring0, pos=pos, cnt=cnt)
    ok(rc)
    want_get = M.ring_get_chunks(out, CH_MAP, n, q, ring0, pos, cnt)
    eq(get["out"], want_get, "get")
    tail_kept(get)

    rc, add = K.ring_chunks(lib, K.ADD, want_get, CH_MAP, n, q, ring_a=ring_a, sched_a=sched_a, gain_a=ga)
    ok(rc)
    want_a = M.ring_add_chunks(want_get, CH_MAP, n, q, ring_a, sched_a, ga)
    eq(add["out"], want_a, f"add gain {ga!r}")
    if ga == 1.0 + 5e-13:
        eq(want_a, M.ring_add_chunks(want_get, CH_MAP, n, q, ring_a, sched_a, 1.0), "unity branch is a plain add")

    rc, add2 = K.ring_chunks(lib, K.ADD2, want_get, CH_MAP, n, q, ring_a=ring_a, sched_a=sched_a, gain_a=ga, ring_b=ring_b,
                             sched_b=sched_b, gain_b=gb)
    ok(rc)
    want_ab = M.ring_add_chunks(want_a, CH_MAP, n, q, ring_b, sched_b, gb)           # layer A first, then layer B
    eq(add2["out"], want_ab, f"add2 gains {ga!r} {gb!r}")
    tail_kept(add2)

    rc, fused = K.ring_chunks(lib, K.GET_ADD, out, CH_MAP, n, q, ring0=ring0, pos=pos, cnt=cnt, ring_a=ring_a, sched_a=sched_a,
                              gain_a=ga, ring_b=ring_b, sched_b=sched_b, gain_b=gb)
    ok(rc)
    eq(fused["out"], want_ab, "fused against the model")
    eq(fused["out"], add2["out"], "fused against get + add2 on the device")
    tail_kept(fused)

    rc, fused1 = K.ring_chunks(lib, K.GET_ADD, out, CH_MAP, n, q, ring0=ring0, pos=pos, cnt=cnt, ring_a=ring_a, sched_a=sched_a,
                               gain_a=ga)
    ok(rc)
    eq(fused1["out"], want_a, "fused without ring B")


@pytest.mark.parametrize("n_dst,n_tab,n", [(1, 0, 1), (2, 1, 257), (3, 64, BIG), (3, 5, 300)])
def test_gather(lib, n_dst, n_tab, n):
    rng = np.random.default_rng(n)
    src = rng.standard_normal((6, n + 2))
    strides, offs = (n + 5, n, n + 8)[:n_dst], (3, 0, 8)[:n_dst]
    tab = rng.integers(-(1 << 62), 1 << 62, n_tab)
    rc, o = K.ring_chunks(lib, K.GATHER, src, CH_MAP, n, 1, strides=strides, offs=offs, tab=tab if n_tab else None)
    ok(rc)
    for got, want in zip(o["dst"], M.rows_gather(src, CH_MAP, n, strides, offs)):
        eq(got, want, "destination")
    eq(o["tab"][:n_tab], tab, "table")
    assert K.untouched(o["tab"][n_tab:])
    eq(o["out"], src, "source")


# --------------------------------------------------------------------------------------------------------------- convproc mix
WET_POISON = [np.nan, np.inf, -np.inf, 1.0e300, -1.0e300, np.nextafter(1.0e300, 0.0), -0.0]
MIX_CASES = [(size, pos0, n) for size in (4, 1024) for pos0 in (0, size - 3, (1 << 40) + 5) for n in (1, 255, 257)] + \
            [(1024, 1021, BIG), (4, 0, BIG)]


@pytest.mark.parametrize("size,pos0,n", MIX_CASES, ids=[f"ring{s}-pos{p}-n{n}" for s, p, n in MIX_CASES])
def test_convproc_mix(lib, size, pos0, n):
    """S = 3 streams, d_new != d_old per stream; x_len in {0, 1, n / 2, n} and ramp_len - ramp_off in {< 0, 0, 1, n / 2, n}
    rotate over the streams and the two ramp_off values 0 and 7; wet_valid = 0 globally and via wet_on for the middle stream
    only; NaN, +-Inf, +-1e300 and the largest value below it in wet; in place and out of place give the same bits"""
    rng = np.random.default_rng(size * 7 + n + pos0 % 1000)
    S = 3
    wet = K.ff((2 * S, n + 2))
    wet[:, :n] = rng.standard_normal((2 * S, n))
    wet[:, :n].flat[rng.integers(0, 2 * S * n, 2 * len(WET_POISON))] = WET_POISON * 2
    ring = rng.standard_normal((2 * S, size))
    gains = rng.standard_normal((S, 2))
    d_new, d_old = [size - 1, 0, 2], [1, size - 1, 3]
    xs = [0, 1, n // 2, n]
    rs = [-3, 0, 1, n // 2, n]
    for k, ramp_off in enumerate((0, 7)):
        x_len = [xs[(k + s + n) % 4] for s in range(S)]
        ramp_len = [rs[(k + 2 * s + n) % 5] + ramp_off for s in range(S)]
        x_gains = rng.uniform(0, 1, (S, n))
        ramp_gains = rng.standard_normal((S, ramp_off + n + 1, 2))
        for wet_valid, wet_on in ((1, [1, 0, 1]), (1, None), (0, [1, 1, 1])):
            kw = dict(x_len=x_len, x_gains=x_gains, wet_valid=wet_valid, ramp_len=ramp_len, ramp_gains=ramp_gains, ramp_off=ramp_off,
                      wet_on=wet_on)
            want = M.convproc_mix(wet, n, gains, ring, pos0, d_new, d_old, **kw)
            rc, o = K.convproc_mix(lib, wet, n, gains, ring, pos0, d_new, d_old, **kw)
            ok(rc)
            eq(o["out"][:, :n], want, f"out of place x_len {x_len} ramp_len {ramp_len} off {ramp_off} valid {wet_valid} on {wet_on}")
            assert K.untouched(o["out"][:, n:])
            eq(o["ring"], ring, "ring")
            if wet_valid and wet_on is not None or n == BIG:
                rc, p = K.convproc_mix(lib, wet, n, gains, ring, pos0, d_new, d_old, in_place=1, **kw)
                ok(rc)
                eq(p["out"][:, :n], want, "in place")
                eq(p["out"][:, n:], wet[:, n:], "in place, behind n")
            if n == BIG:
                return


def test_convproc_mix_null_lengths(lib):
    rng = np.random.default_rng(5)
    n, S = 40, 3
    wet, ring, gains = rng.standard_normal((2 * S, n)), rng.standard_normal((2 * S, 16)), rng.standard_normal((S, 2))
    rc, a = K.convproc_mix(lib, wet, n, gains, ring, 3, [1, 2, 3], [4, 5, 6])
    ok(rc)
    rc, b = K.convproc_mix(lib, wet, n, gains, ring, 3, [1, 2, 3], [4, 5, 6], x_len=[0] * S, x_gains=np.full((S, 4), np.nan),
                           ramp_len=[0] * S, ramp_gains=np.full((S, 4, 2), np.nan))
    ok(rc)
    eq(a["out"], b["out"], "null lengths against zero lengths")
    eq(a["out"], M.convproc_mix(wet, n, gains, ring, 3, [1, 2, 3], [4, 5, 6]), "model")


@pytest.mark.parametrize("size,pos0,n", [(4, 3, 4), (1024, 1024 - 3, 300), (1024, (1 << 40) + 1000, 257)])
def test_put_then_mix(lib, size, pos0, n):
    """ring_put wrapping the ring end, read back through d = 0 (dry-only) and d = 1"""
    rng = np.random.default_rng(size + n)
    ring, z = rng.standard_normal((4, size)), rng.standard_normal((4, n + 1))
    wet = rng.standard_normal((4, n))
    rc, o = K.convproc_mix(lib, wet, n, np.ones((2, 2)), ring, pos0, [0, 1], [0, 0], wet_valid=0, ring_in=z, n_put=n)
    ok(rc)
    want_ring = M.ring_put(ring, z, n, pos0)
    eq(o["ring"], want_ring, "ring after the put")
    eq(o["out"], M.convproc_mix(wet, n, np.ones((2, 2)), want_ring, pos0, [0, 1], [0, 0], wet_valid=0), "read back")
    eq(o["out"][:2], z[:2, :n], "d = 0 reads what was put")


@pytest.mark.parametrize("old,new", [(4, 4), (4, 16), (1024, 4096)])
@pytest.mark.parametrize("end", [0, 3, "old", "old+1", (1 << 40) + 1])
def test_ring_regrow(lib, old, new, end):
    end = {"old": old, "old+1": old + 1}.get(end, end)
    rng = np.random.default_rng(old + new + end % 97)
    old_ring = rng.standard_normal((4, old))
    wet = np.ones((4, 1))
    rc, o = K.convproc_mix(lib, wet, 0, np.ones((2, 2)), K.ff((4, new)), 0, [0, 0], [0, 0], old_ring=old_ring, regrow_end=end)
    ok(rc)
    eq(o["ring"], M.ring_regrow(old_ring, new, end), "regrown ring")
    for p in range(end - old, end):           # every retained absolute position reads back the same through the new mask
        assert (o["ring"][:, p % new] == old_ring[:, p % old]).all()
    assert int((o["ring"] != 0.0).sum()) <= 4 * old


# ---------------------------------------------------------------------------------------------------------------- tail reader
def layer_sets(B):
    return {"PL=B,oL<PL": [(B, B // 2, 0), (4 * B, B, 1)], "PL=4B,oL=PL": [(4 * B, 4 * B, 1), (8 * B, 8 * B, 3)],
            "PL=8B,oL>PL": [(8 * B, 11 * B, 3), (4 * B, 3 * B + B // 2, 0)], "one layer": [(4 * B, 3 * B, 1)]}


@pytest.mark.parametrize("B", [64, 1024])
@pytest.mark.parametrize("layers", list(layer_sets(64)))
@pytest.mark.parametrize("calls", [[1] * 20, [3, 1, 8, 2], [16]], ids=["1x20", "3-1-8-2", "16"])
def test_tail_schedule(lib, B, layers, calls):
    lay = layer_sets(B)[layers]
    for state in ([0, 0, 0, 0], [7, 5 * B, 2 * B + 3, 6 * B]):
        rc, o = K.tail_reader(lib, calls, B, lay, state)
        ok(rc)
        st, seen = list(state), 0
        for i, T in enumerate(calls):
            st, sched = M.tail_schedule(st, T, B, lay)
            eq(o["sched"][i], np.array(sched, dtype=np.int64), f"schedule of call {i}")
            eq(o["states"][i], np.array(st, dtype=np.int64), f"state after call {i}")
            seen += sum(v >= 0 for row in sched for v in row)
        assert seen > 0 or layers == "PL=8B,oL>PL"


def test_tail_one_call_equals_sixteen(lib):
    B, lay = 64, layer_sets(64)["PL=B,oL<PL"]
    _, one = K.tail_reader(lib, [16], B, lay, [0, 0, 0, 0])
    rc, many = K.tail_reader(lib, [1] * 16, B, lay, [0, 0, 0, 0])
    ok(rc)
    eq(np.concatenate(many["sched"], axis=1), one["sched"][0], "schedules")
    eq(many["states"][-1][:3], one["states"][0][:3], "callbacks and cursors")
    assert -1 in one["sched"][0] and one["sched"][0].max() > 0


@pytest.mark.parametrize("n,size", [(2048 + 300, 256), (2048 + 300, 2048), (2048, 2048), (2048 + 300, 4096)],
                         ids=["ring<n", "ring<n,2048", "ring=n", "ring>n"])
@pytest.mark.parametrize("cursor", ["behind", "inside", "beyond"])
def test_tail_append(lib, n, size, cursor):
    """n = 2048 + 300 samples (8 x 256 threads: a second trip); layer 1's read cursor R - g0 negative, inside the call and
    beyond it (then nothing is stored and its rings keep their contents), layer 2's always inside; 2 layers x 2 channels, a
    distinct poison value per ring.  The schedule in front of the append sets g0 = callbacks * B; with PL = B and oL = 0 the
    reader never finds B samples, so the cursors stay where this test puts them."""
    B, cb0 = 64, (1 << 27) + 1
    g0 = cb0 * B
    rng = np.random.default_rng(size + n)
    r1 = {"behind": g0 - 5, "inside": g0 + 700, "beyond": g0 + n + 1}[cursor]
    state, lay = [cb0, r1, g0 + n - 248, 0], [(B, 0, 0), (B, 0, 0)]
    layer_out = rng.standard_normal((2, 2, n))
    ring = np.arange(1.0, 5.0).reshape(2, 2, 1) * np.ones((2, 2, size))
    rc, o = K.tail_reader(lib, [1], B, lay, state, layer_out=layer_out, ring=ring)
    ok(rc)
    st, sched = M.tail_schedule(state, 1, B, lay)
    assert st == [cb0 + 1, r1, g0 + n - 248, g0] and sched == [[-1], [-1]]
    eq(o["states"][0], np.array(st, dtype=np.int64), "state")
    eq(o["ring"], M.tail_append(ring, layer_out, st, 2), "rings")
    if cursor == "beyond":
        eq(o["ring"][0], ring[0], "nothing stored for layer 1")
    else:
        assert not K.same_bits(o["ring"][0], ring[0])


# ----------------------------------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("n", [1, 257, BIG])
@pytest.mark.parametrize("src_off,dst_off", [(0, 1), (3, 4), (2, 0)])
def test_rows_copy(lib, n, src_off, dst_off):
    rng = np.random.default_rng(n + src_off)
    src, dst = rng.standard_normal((3, n + src_off + 2)), K.ff((3, n + dst_off + 3))
    rc, o = K.rows(lib, K.COPY, dst, n, src=src, src_off=src_off, dst_off=dst_off)
    ok(rc)
    want = dst.copy()
    want[:, dst_off:dst_off + n] = src[:, src_off:src_off + n]
    eq(o["dst"], want, "copy")


def test_rows_scale(lib):
    rng = np.random.default_rng(9)
    for n in (1, 257, BIG):
        data = rng.standard_normal((6, n + 2))
        data[:, 0] = [np.float64(-0.0)] * 6
        payload = np.array([0x7FF8000000ABCDEF], dtype=np.uint64).view(np.float64)[0]       # a NaN with a payload
        data[:2, n - 1] = payload
        rc, o = K.rows(lib, K.SCALE, data, n, gain=[1.0, 0.5, -1.0])
        ok(rc)
        eq(o["dst"], M.rows_scale(data, n, [1.0, 0.5, -1.0]), f"scale n {n}")
        eq(o["dst"][:2], data[:2], "gain 1 keeps the bits")
        eq(o["dst"][:, n:], data[:, n:], "behind n")


@pytest.mark.parametrize("n", [7, 257, BIG])
def test_bypass_blend(lib, n):
    rng = np.random.default_rng(n)
    for on in ([1, 0, 1], [0, 1, 1], [1, 1, 1], [1, 0], [0, 1], [1, 1]):
        S = len(on)
        for lens in ([0, 1, n - 1][:S], [n, n + 5, 0][:S], [n - 1, n, n + 5][-S:]):
            out, dry = rng.standard_normal((2 * S, n + 3)), rng.standard_normal((2 * S, n + 1))
            gains, g_end = rng.uniform(0, 1, (S, n + 5)), [0.0, 1.0, 0.25][-S:] if on[0] else [0.25, 0.0, 1.0][:S]
            rc, o = K.rows(lib, K.BLEND, out, n, src=dry, on=on, length=lens, g_end=g_end, gains=gains)
            ok(rc)
            want = M.bypass_blend(out, dry, n, on, lens, g_end, gains)
            eq(o["dst"], want, f"blend on {on} len {lens}")
            eq(o["dst"][:, n:], out[:, n:], "behind n")
        if n == BIG:
            break


def test_valid_base_sets_run(lib):
    """the valid argument sets of the refusal table (tests/test_host_and_abi_cpu.py walks its refusals) run for real"""
    res = K.valid_calls(lib)
    assert [k for k, rc, _, _ in res if rc != 0] == [] and len(res) == 15
    assert [r for r in K.walk_refusals(lib) if r[2] != K.INVALID_ARG] == []
