"""Edges of the cascade kernels (svf_kernels.hip) that the bulk parity tests pass over: the cold continuation of the unchained
span kernel at the headline size, the tier decisions of the output stage and the range check at their exact boundary values,
level independence and quiet signals (where an absolute bound on a full-scale signal cannot see a leak), and the digital
silence of the OutputFilter's DF-II-T sections.  Against the oracle's EQProcessor / OutputFilter restatements, or against
the engine itself where the property needs no reference (bit equality under power-of-two scaling, clean channels unchanged
by dirty neighbours)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 512
SPAN = 8192
ULP_UP, ULP_DN = np.nextafter(4.5, np.inf), np.nextafter(4.5, 0.0)
# band outputs at the output stage's decisions: the fastTanh clip threshold 4.5 (the small-signal stage is chosen by a
# high-word compare against it), values inside the first float step above it, and the +-100 clamp
HOT = [4.5, -4.5, ULP_DN, ULP_UP, -ULP_UP, 4.6, -4.6, 100.0, -100.0, np.nextafter(100.0, 0.0), np.nextafter(100.0, 1e3), 130.0, -250.0]


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def _copy_params(po, pa):
    for i in range(20):
        b, o = pa.bands[i], po.bands[i]
        b.frequency, b.gain, b.q, b.enabled, b.type, b.channel_mode = o.frequency, o.gain, o.q, o.enabled, o.type, o.channelMode
    pa.total_gain_db, pa.agc_enabled, pa.nonlinear_saturation, pa.filter_structure = po.totalGainDb, po.agcEnabled, po.nonlinearSaturation, po.filterStructure
    return pa


def _pass_params(O, sat, mode):
    # one enabled 0 dB peaking band: an input sample IS the band output the output stage decides on
    # (premise checked on the CPU: test_oracle_cpu.py::test_pass_band_is_bit_exact)
    return O.eq_params_pass_band(sat, mode)


def _bench_params(O, sat, mode):
    p = O.eq_params_bench(sat)
    p.bands[6].channelMode = mode
    p.totalGainDb = 0.75
    return p


# kernel paths: blocks per call, EQ mode.  chained: 3 whole spans per call on k_svf_cascade_tpv<8, true> (4 channels chain);
# unchained: one span per call, which never chains (k_svf_cascade_tpv<8, false>); tpv0: one span of two whole waves
# (k_svf_cascade_tpv<0, false, false>); partial: 2560 samples = three waves, the last one half padding (<0, false, true>);
# short: one 512-sample callback (k_svf_cascade_short<8>); sequential: k_svf_cascade
PATHS = {"chained": (48, "auto"), "unchained": (16, "auto"), "tpv0": (4, "auto"), "partial": (5, "auto"),
         "short": (1, "auto"), "sequential": (5, "sequential")}


def _edge_positions(path, n):
    """sample indices inside one call at which the output stage's decision changes: one per wave (the decision is taken per
    wave and band), alternating between the first and the last sample of the wave's segment"""
    if path in ("chained", "unchained"):
        return [sp * SPAN + w * 1024 + (0 if (w + sp) % 2 == 0 else 1023) for sp in range(n // SPAN) for w in range(8)]
    if path == "tpv0":
        return [0, 2047]
    if path in ("partial", "sequential"):
        return [1023, 1024, 2559]           # last sample of wave 0, first of wave 1, last valid sample of the partial span
    return [0]                              # short: one wave per call; the position walks the chunk edges from call to call


SHORT_EDGES = [0, 7, 8, 255, 256, 263, 503, 504, 511]


def _engine(amd, path, S, pos, kind="eq"):
    T, mode = PATHS[path]
    eng = amd.BatchedEngine(S, max_ir_len=512, max_blocks_per_call=T)
    if kind == "eq":
        for s in range(S):
            eng.set_eq_params(s, _copy_params(pos[s], amd.eq_params_default()))
    eng.set_eq_mode(amd.CPQ_EQ_MODE_SEQUENTIAL if mode == "sequential" else amd.CPQ_EQ_MODE_AUTO)
    return eng, T * B


def _run(eng, x, n, kind="eq"):
    fn = eng.eq_process if kind == "eq" else eng.outfilter_process
    return np.concatenate([fn(x[:, o:o + n]) for o in range(0, x.shape[1], n)], axis=1)


def _check_path(eng, path, calls):
    launches, gave_up = eng.eq_chain_status()
    assert gave_up == 0
    assert launches == (calls if path == "chained" else 0)


def _oracle_eq(O, x, pos):
    ref = np.empty_like(x)
    for s in range(len(pos)):
        ref[2 * s], ref[2 * s + 1], _ = O.eq_process_stereo(x[2 * s], x[2 * s + 1], pos[s])
    return ref


def _state_envelope(O, xl, xr, fn, piece=B, window=SPAN):
    """max |band state| of the oracle at every piece boundary within the last `window` samples (and the piece itself), per
    sample: the scale of the rounding a time-parallel evaluation may commit behind states far above the signal"""
    n = len(xl)
    st = None
    ends = []
    for o in range(0, n, piece):
        _, _, st = fn(xl[o:o + piece], xr[o:o + piece], st)
        ends.append(np.nanmax(np.abs(st)))
    ends = np.array(ends)
    env = np.empty(n)
    for i in range(len(ends)):
        lo = max(0, i - window // piece)
        env[i * piece:(i + 1) * piece] = ends[lo:i + 1].max()
    return env


# ---------------------------------------------------------------------------------------------------------------- A
def _dirty_headline_inputs(O, S, n, calls, checked):
    rng = np.random.default_rng(2024)
    x = 0.25 * (2.0 * rng.random((2 * S, calls * n)) - 1.0)
    for c in checked:
        x[c] = O.gen_pcm(calls * n, stream=c // 2, channel=c % 2)
    clean = x.copy()
    x[130, n + 0] = np.nan                          # call 1, sample 0 of span 0: both spans of the call guarded
    x[263, SPAN - 1] = np.inf                       # call 0, last sample of span 0
    x[400, BIG_AT] = BIG                            # call 1, end of span 1: out-of-range states into the remainder and call 2
    x[37, 2 * n + 2 * SPAN + 1000] = np.nan         # call 2, in the 4096-sample remainder
    return x, clean


DIRTY = (130, 263, 400, 37)
# 200 samples before the end of call 1's second span.  Band states of 1.6e13 (EQ) / 2.3e13 (OutputFilter) behind it, still
# 3e11 / 1.7e10 at the start of call 2: the remainder of call 1 and the first span of call 2 leave the fast path through the
# state check, not through their input (a 1e12 sample leaves states below 1e9 by call 2)
BIG, BIG_AT = 1.0e16, 40 * B + 2 * SPAN - 200


@pytest.mark.parametrize("kind", ["eq", "outfilter"])
def test_unchained_cold_continuation_at_the_headline_size(amd, oracle, kind):
    """256 streams = 512 channels: one workgroup per channel (k_svf_cascade_tpv<8, false>), calls of 40 blocks = two whole
    spans + a 4096-sample remainder on k_svf_cascade_tpv<0, false, false>, three calls.  A span that fails the range check
    leaves the fast loop and every later span of the channel in the call runs on the guarded recurrence; a span whose
    carried states are out of range leaves it through the state check.  Dirty channels, their pair-mates and the edges of
    the grid against the oracle; every clean channel bit-equal to the same engine on the all-clean input."""
    O = oracle
    S, T, calls = 256, 40, 3
    n = T * B
    checked = sorted({0, 1, 511} | {c for d in DIRTY for c in (d, d ^ 1)})
    assert BIG_AT == n + 2 * SPAN - 200
    x, clean = _dirty_headline_inputs(O, S, n, calls, checked)
    if kind == "eq":
        pos = [_bench_params(O, 0.2, 1 if s % 3 == 1 else 0) for s in range(S)]
        ref_fn = lambda s: (lambda a, b, st=None: O.eq_process_stereo(a, b, pos[s], state=st))
    else:
        q = O.outfilter_design(1, 1, 0, 1, 48000.0)
        ref_fn = lambda s: (lambda a, b, st=None: O.outfilter_process_stereo(a, b, q, state=st))

    def make():
        eng = amd.BatchedEngine(S, max_ir_len=512, max_blocks_per_call=T)
        if kind == "eq":
            for s in range(S):
                eng.set_eq_params(s, _copy_params(pos[s], amd.eq_params_default()))
        else:
            eng.set_outfilter_params(amd.CPQ_ALL_STREAMS, 1, 1, 0, 1)
        return eng

    eng = make()
    y = _run(eng, x, n, kind)
    launches, gave_up = eng.eq_chain_status()
    assert launches == 0 and gave_up == 0          # this engine must not chain: the test is about the unchained kernel
    eng.close()
    eng = make()
    y_clean = _run(eng, clean, n, kind)
    eng.close()

    for s in sorted({c // 2 for c in checked}):
        f = ref_fn(s)
        rl, rr, _ = f(x[2 * s], x[2 * s + 1])
        for ch, r in ((2 * s, rl), (2 * s + 1, rr)):
            g = y[ch]
            if kind == "outfilter" and ch in (130, 263, 37):
                # the OutputFilter has no guard: from the non-finite sample on, the reference's output is non-finite
                bad = ~np.isfinite(r)
                assert np.array_equal(~np.isfinite(g), bad) and np.array_equal(g[bad], r[bad], equal_nan=True), ch
                assert np.abs(g[~bad] - r[~bad]).max() <= 5e-12, ch
                continue
            assert np.all(np.isfinite(g)), ch
            d = np.abs(g - r)
            if ch == 400:
                # the carried states reach the paths named above: out of range at the start of call 1's remainder and of call 2
                _, _, st = f(x[400, :n + 2 * SPAN], x[401, :n + 2 * SPAN])
                at_rem = np.abs(st).max()
                _, _, st = f(x[400, n + 2 * SPAN:2 * n], x[401, n + 2 * SPAN:2 * n], st)
                at_call2 = np.abs(st).max()
                assert at_rem >= 1e9 and at_call2 >= 1e9, (at_rem, at_call2)
                # behind the big sample: the states are far above the signal and the fast path's rounding is relative to them
                big = BIG_AT
                env = _state_envelope(O, x[400], x[401], f)
                print(kind, "ch 400: max |state| at the remainder %.3g, at call 2 %.3g" % (at_rem, at_call2),
                      "max err / env behind the sample", (d[big:] / env[big:]).max())
                assert d[:big].max() <= (1e-13 if kind == "eq" else 5e-12)
                assert np.all(d[big:] <= 5e-12 + 1e-13 * env[big:])
            else:
                worst = d.max()
                assert worst <= (1e-13 if kind == "eq" else 5e-12), (ch, worst)
    # the dirty channels are each a channel of their own: every other channel is the one the all-clean input gives
    others = np.ones(2 * S, dtype=bool)
    others[list(DIRTY)] = False
    assert np.array_equal(y[others], y_clean[others])

    # the cliff of the cold continuation, for the record: one 128-block call, clean against one NaN at span 0 of one channel
    T2 = 128
    eng = amd.BatchedEngine(S, max_ir_len=512, max_blocks_per_call=T2)
    if kind == "eq":
        eng.set_eq_params(amd.CPQ_ALL_STREAMS, _copy_params(pos[0], amd.eq_params_default()))
    else:
        eng.set_outfilter_params(amd.CPQ_ALL_STREAMS, 1, 1, 0, 1)
    x2 = clean[:, :T2 * B] if clean.shape[1] >= T2 * B else np.tile(clean[:, :n], (1, 4))[:, :T2 * B]
    eng.profile_enable(True)
    times = []
    for dirty in (False, False, True):
        xx = x2.copy()
        if dirty:
            xx[300, 0] = np.nan
        eng.profile_reset()
        _run(eng, xx, T2 * B, kind)
        times.append(eng.profile_read()["k_svf_cascade_tp" if kind == "eq" else "k_outfilter_cascade"][1])
    print(kind, "128-block call at 256 streams: clean %.3f ms, one NaN at span 0 of one channel %.3f ms" % (times[1], times[2]))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("sat", [0.0, 0.2])
@pytest.mark.parametrize("params", ["pass", "bench"])
@pytest.mark.parametrize("path", list(PATHS))
def test_output_stage_decisions_at_wave_edges(amd, oracle, path, params, sat):
    """One hot sample per wave on a quiet signal, at the first or last sample of the wave's 1024-sample segment (at the last
    valid sample of a partial span, at chunk edges of the short kernel), carrying the exact boundary values: 4.5, 4.5 -+ one
    ulp, 4.6, +-100 and its neighbours, beyond the clamp.  Stream 0 takes the stereo output stage, stream 1 the scalar one
    (Left mode).  With the pass band the hot value is the band output itself."""
    O = oracle
    T, _ = PATHS[path]
    n = T * B
    S = 2
    mk = _pass_params if params == "pass" else _bench_params
    pos = [mk(O, sat, 0), mk(O, sat, 1)]
    edges = _edge_positions(path, n)
    calls = len(SHORT_EDGES) * 2 if path == "short" else max(3, math.ceil(2 * len(HOT) / len(edges)))
    x = np.stack([O.gen_pcm(calls * n, stream=c // 2, channel=c % 2) for c in range(2 * S)])
    k = 0
    for call in range(calls):
        ps = [SHORT_EDGES[call % len(SHORT_EDGES)]] if path == "short" else edges
        for p in ps:
            for c in range(2 * S):
                x[c, call * n + p] = HOT[(k + 3 * c) % len(HOT)]
            k += 1
    eng, n = _engine(amd, path, S, pos)
    eng.profile_enable(True)
    y = _run(eng, x, n)
    _check_path(eng, path, calls)
    prof = eng.profile_read()
    assert (prof["k_svf_cascade"][0] > 0) == (path == "sequential") and (prof["k_svf_cascade_tp"][0] > 0) == (path != "sequential")
    eng.close()
    ref = _oracle_eq(O, x, pos)
    d = np.abs(y - ref)
    print(path, params, "sat", sat, "max abs diff", d.max())
    assert np.all(np.isfinite(y)) and np.all(d <= 1e-13 * (1.0 + np.abs(ref)))


@pytest.mark.parametrize("path", list(PATHS))
def test_range_check_at_its_bound(amd, oracle, path):
    """Bursts of exactly +-1e9 (outside the range the host proved guard-free: the guarded path) and of nextafter(1e9, 0)
    (inside: the fast path, which omits the reference's 1e15 state and output guards), their signs those of the first band's
    impulse response read backwards, so that the band's state and output reach the band's l1 gain times the bound.  The burst
    lies in the first span of the first call: the guarded path starts there from the exact (zero) states and runs the
    reference's operations, so the +-1e9 channels are bit-equal to the oracle over that span, and the fast path's
    rounding-level differences show on the nextafter channels -- a range check off by one ulp in either direction fails.
    Behind the burst, states of about 1e9 are carried on the fast path in parity with the oracle, relative to their size.
    (The bench preset's first band peaks near 1.2e9 here, five decades below the guard: this checks the range check and the
    carrying of large states, not the margin of the host's guard-freedom proof.)"""
    O = oracle
    T, mode = PATHS[path]
    S = 2
    pos = [_bench_params(O, 0.2, 0), _bench_params(O, 0.2, 1)]
    p0 = O.eq_params_default()
    for i in range(20):
        p0.bands[i].enabled = 0
    b0, o0 = p0.bands[0], pos[0].bands[0]
    b0.frequency, b0.gain, b0.q, b0.enabled, b0.type, b0.channelMode = o0.frequency, o0.gain, o0.q, 1, o0.type, 0
    p0.nonlinearSaturation = 0.0
    n = T * B
    span0 = {"chained": SPAN, "unchained": SPAN, "tpv0": 2048, "partial": 2560, "short": 512, "sequential": 2560}[path]
    L = min(4096, span0 - 64)
    imp = np.zeros(L)
    imp[0] = 1e-3
    h, _, _ = O.eq_process_stereo(imp, imp, p0)
    sign = np.where(h[::-1] >= 0.0, 1.0, -1.0)
    calls = 4 if path != "short" else 24
    x = np.stack([O.gen_pcm(calls * n, stream=c // 2, channel=c % 2) for c in range(2 * S)])
    bound = [1.0e9, np.nextafter(1.0e9, 0.0)]
    end = L + 32                                    # the burst ends here, inside the first span of call 0
    for c in range(2 * S):
        x[c, end - L:end] = bound[c % 2] * sign * (1.0 if c < 2 else -1.0)
    eng, n = _engine(amd, path, S, pos)
    y = _run(eng, x, n)
    _check_path(eng, path, calls)
    eng.close()
    for s in range(S):
        f = lambda a, b, st=None, s=s: O.eq_process_stereo(a, b, pos[s], state=st)
        rl, rr, _ = f(x[2 * s], x[2 * s + 1])
        env = _state_envelope(O, x[2 * s], x[2 * s + 1], f)
        for ch, r in ((2 * s, rl), (2 * s + 1, rr)):
            d = np.abs(y[ch] - r)
            print(path, "ch", ch, "bound", abs(x[ch, end - 1]), "max |state|", env.max(), "first span max diff", d[:span0].max(),
                  "max err / env", (d / env).max())
            assert np.all(np.isfinite(y[ch]))
            if ch % 2 == 0 or mode == "sequential":
                assert np.array_equal(y[ch, :span0], r[:span0])         # guarded (or sequential): the reference's operations
            else:
                assert d[:span0].max() > 0.0                            # fast path: time-parallel rounding
            assert d[:end - L].max() <= 1e-13
            assert np.all(d <= 1e-12 + 1e-13 * env)


# ---------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("path", list(PATHS))
def test_level_independence_by_powers_of_two(amd, path, oracle):
    """Saturation 0 and no clamp hit: every stage of every path is linear in the signal (the fast and small-signal output
    stages are the identity, the guards are idle), and a power-of-two scale is exact -- gpu(x 2^-k) == gpu(x) 2^-k bit for bit,
    with the states carried across calls.  Any additive leak (a stale state, a padding sample, another channel) breaks it."""
    O = oracle
    T, _ = PATHS[path]
    n = T * B
    calls = 3 if path != "short" else 6
    po = _bench_params(O, 0.0, 1)
    S = 3
    base = np.stack([O.gen_pcm(calls * n, stream=0, channel=c) for c in range(2)])
    base[:, n // 3:n // 3 + 700] *= 24.0                  # hot: the general output stage in some waves (|y| < 100: no clamp)
    scales = [1.0, 2.0 ** -30, 2.0 ** -60]
    x = np.concatenate([base * k for k in scales])
    eng, n = _engine(amd, path, S, [po] * S)
    y = _run(eng, x, n)
    _check_path(eng, path, calls)
    eng.close()
    assert np.abs(y[:2]).max() < 100.0
    for i in (1, 2):
        assert np.array_equal(y[2 * i:2 * i + 2], y[:2] * scales[i]), (path, i, np.abs(y[2 * i:2 * i + 2] - y[:2] * scales[i]).max())


@pytest.mark.parametrize("path", list(PATHS))
def test_quiet_signal_parity(amd, oracle, path):
    """The bench preset at saturation 0.2 on PCM at 1e-6 of full scale (-120 dB): parity with the oracle to 1e-12 of the
    signal level, where the full-scale tests' absolute bounds would pass an error a million times larger."""
    O = oracle
    T, _ = PATHS[path]
    n = T * B
    calls = 3 if path != "short" else 6
    S = 2
    level = 1e-6
    pos = [_bench_params(O, 0.2, 0), _bench_params(O, 0.2, 1)]
    x = level * np.stack([O.gen_pcm(calls * n, stream=c // 2, channel=c % 2) for c in range(2 * S)])
    eng, n = _engine(amd, path, S, pos)
    y = _run(eng, x, n)
    _check_path(eng, path, calls)
    eng.close()
    d = np.abs(y - _oracle_eq(O, x, pos))
    print(path, "quiet: max abs diff", d.max(), "relative to the level", d.max() / level)
    assert d.max() <= 1e-12 * level


@pytest.mark.parametrize("path,T", [("chained", 40), ("unchained", 20), ("short", 1)])
def test_output_filter_digital_silence(amd, oracle, path, T):
    """One span of PCM, then exact zeros (AUTO mode).  The reference flushes every DF-II-T state below 1e-20 to zero
    (OutputFilter.cpp:154-162), so its output becomes exactly 0.0 once the states have decayed; the time-parallel path must
    get there too -- once the oracle has been silent for a whole span, so is the GPU, bit for bit.  chained: 2 spans per call
    on the chained kernel + a 4096-sample remainder; unchained: 1 span + 2048; short: 512-sample calls."""
    O = oracle
    S = 2
    n = T * B
    total = 9 * SPAN
    calls = -(-total // n)
    x = np.zeros((2 * S, calls * n))
    for c in range(2 * S):
        x[c, :SPAN] = O.gen_pcm(SPAN, stream=c // 2, channel=c % 2)
    q = O.outfilter_design(1, 1, 0, 1, 48000.0)
    eng = amd.BatchedEngine(S, max_ir_len=512, max_blocks_per_call=T)
    eng.set_outfilter_params(amd.CPQ_ALL_STREAMS, 1, 1, 0, 1)
    y = _run(eng, x, n, "outfilter")
    launches, gave_up = eng.eq_chain_status()
    assert gave_up == 0 and (launches > 0) == (path == "chained")
    eng.close()
    for s in range(S):
        rl, rr, _ = O.outfilter_process_stereo(x[2 * s], x[2 * s + 1], q)
        for ch, r in ((2 * s, rl), (2 * s + 1, rr)):
            nz = np.nonzero(r)[0]
            quiet = nz[-1] + 1 if len(nz) else 0
            assert quiet + 2 * SPAN <= x.shape[1], quiet        # the oracle falls silent with spans to spare
            late = np.nonzero(y[ch, quiet + SPAN:])[0]
            print(path, "ch", ch, "oracle silent from", quiet, "GPU nonzero samples a span later", len(late),
                  "max", np.abs(y[ch, quiet + SPAN:]).max())
            assert len(late) == 0
            assert np.abs(y[ch] - r).max() <= 5e-12


@pytest.mark.parametrize("path,T", [("chained", 40), ("unchained", 20), ("short", 1)])
def test_output_filter_quiet_signal_parity(amd, oracle, path, T):
    """The OutputFilter at 1e-6 of full scale against the oracle: the full-scale bounds of test_output_filter_df2t_cascade
    (5e-12 max, 1e-12 RMS) relative to the level."""
    O = oracle
    S = 2
    n = T * B
    calls = -(-3 * SPAN // n)
    level = 1e-6
    x = level * np.stack([O.gen_pcm(calls * n, stream=c // 2, channel=c % 2) for c in range(2 * S)])
    q = O.outfilter_design(1, 1, 0, 1, 48000.0)
    eng = amd.BatchedEngine(S, max_ir_len=512, max_blocks_per_call=T)
    eng.set_outfilter_params(amd.CPQ_ALL_STREAMS, 1, 1, 0, 1)
    y = _run(eng, x, n, "outfilter")
    eng.close()
    err2, worst = 0.0, 0.0
    for s in range(S):
        rl, rr, _ = O.outfilter_process_stereo(x[2 * s], x[2 * s + 1], q)
        worst = max(worst, np.abs(y[2 * s] - rl).max(), np.abs(y[2 * s + 1] - rr).max())
        err2 += np.sum((y[2 * s] - rl) ** 2) + np.sum((y[2 * s + 1] - rr) ** 2)
    r = float(np.sqrt(err2 / y.size))
    print(path, "outfilter quiet: max", worst / level, "rms", r / level, "relative to the level")
    assert worst <= 5e-12 * level and r <= 1e-12 * level
