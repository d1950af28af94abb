"""The EQ call path -- bypass fades, band resets, the total-gain ramp, the AGC reset, the output filter's pass-through toggle -- pinned
bit for bit between engines of one build that are handed the same samples in different cuts.

The parity suites compare these paths with the oracle at a tolerance; a piece boundary or a reset that moved by a callback could
hide below it.  Here every comparison is np.array_equal: in CPQ_EQ_MODE_SEQUENTIAL the arithmetic of a sample does not depend on
how the stretch is cut into calls, so one call of 48 callbacks, the same stretch cut once at an odd callback and one call per
callback must agree in every bit -- and leave the same EQ and output-filter state, which a following call of one callback shows.

3 streams, block 64, 48 kHz: the 5 ms bypass fade (240 samples) ends inside the fourth callback, the 50 ms gain ramp (2400
samples) inside the 38th.  A scenario is a list of phases (setup, callbacks, cut): the setup runs in front of the phase, and only
phases marked `cut` are cut -- the others are one call each on every engine.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, B, RATE, CBS = 3, 64, 48000.0, 48
CUTS = [None, 17, "each"]       # one call; two calls, cut at an odd callback; one call per callback


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def eq_params(amd, O, gain_db=-2.0, agc=False):
    po = O.eq_params_bench(0.2)
    pa = amd.eq_params_default()
    for i in range(20):
        b, o = pa.bands[i], po.bands[i]
        b.frequency, b.gain, b.q, b.enabled, b.type, b.channel_mode = o.frequency, o.gain, o.q, o.enabled, o.type, o.channelMode
    pa.bands[5].gain = 0.0                  # a flat band: drops out of the basic path's band nodes while a fade runs
    pa.total_gain_db, pa.agc_enabled = gain_db, int(agc)
    pa.nonlinear_saturation, pa.filter_structure = po.nonlinearSaturation, po.filterStructure
    return pa


def signal(O, n_callbacks, silent=()):
    """rows of every channel with a level step (the AGC gain moves); silent: (stream, callback) blocks set to zero"""
    n = n_callbacks * B
    x = np.stack([O.gen_pcm(n, stream=c // 2, channel=c % 2) for c in range(2 * S)])
    x[:, n // 3:n // 2] *= 4.0
    for s, t in silent:
        x[2 * s:2 * s + 2, t * B:(t + 1) * B] = 0.0
    return x


def new_engine(amd, **kw):
    eng = amd.BatchedEngine(S, block_size=B, max_ir_len=512, max_blocks_per_call=CBS, sample_rate=RATE, partition_size=B, **kw)
    eng.set_eq_mode(amd.CPQ_EQ_MODE_SEQUENTIAL)
    return eng


def play(eng, fn, x, phases, cut):
    ys, pos = [], 0
    for setup, callbacks, cuttable in phases:
        if setup:
            setup(eng)
        sizes = [callbacks]
        if cuttable and cut == "each":
            sizes = [1] * callbacks
        elif cuttable and cut is not None:
            sizes = [cut, callbacks - cut]
        for k in sizes:
            ys.append(getattr(eng, fn)(np.ascontiguousarray(x[:, pos:pos + k * B])))
            pos += k * B
    assert pos == x.shape[1]
    return np.concatenate(ys, axis=1)


def assert_cut_invariant(amd, x, phases, fn="eq_process", first=None):
    outs = []
    for cut in CUTS:
        eng = new_engine(amd)
        if first:
            first(eng)
        outs.append(play(eng, fn, x, phases, cut))
        eng.close()
    for y in outs[1:]:
        assert np.array_equal(outs[0], y)
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 1e-3
    return outs[0]


def test_bypass_requested_mid_run_on_one_stream(amd, oracle):
    pa = eq_params(amd, oracle)
    phases = [(lambda e: e.set_eq_params(amd.CPQ_ALL_STREAMS, pa), 8, False),
              (lambda e: e.set_eq_bypass(1, True), CBS, True),
              (None, 1, False)]
    x = signal(oracle, 8 + CBS + 1)
    y = assert_cut_invariant(amd, x, phases)
    at = (8 + 4) * B                    # the fade has ended: stream 1 is the dry signal, the others are not
    assert np.array_equal(y[2:4, at:], x[2:4, at:]) and not np.array_equal(y[0:2, at:], x[0:2, at:])


def test_bypass_released(amd, oracle):
    pa = eq_params(amd, oracle)
    phases = [(lambda e: e.set_eq_params(amd.CPQ_ALL_STREAMS, pa), 4, False),
              (lambda e: e.set_eq_bypass(1, True), 8, False),
              (lambda e: e.set_eq_bypass(1, False), CBS, True),
              (None, 1, False)]
    x = signal(oracle, 4 + 8 + CBS + 1)
    y = assert_cut_invariant(amd, x, phases)
    assert np.array_equal(y[2:4, 8 * B:12 * B], x[2:4, 8 * B:12 * B])       # bypassed ...
    assert not np.array_equal(y[2:4, 20 * B:], x[2:4, 20 * B:])             # ... and back


def test_band_reset_taken_by_a_silent_callback(amd, oracle):
    pa = eq_params(amd, oracle)
    phases = [(lambda e: e.set_eq_params(amd.CPQ_ALL_STREAMS, pa), 8, False),
              (lambda e: e.request_band_reset(1, 0x00000F0F), CBS, True),
              (None, 1, False)]
    x = signal(oracle, 8 + CBS + 1, silent=[(1, 8 + 5)])
    y = assert_cut_invariant(amd, x, phases)
    # the reset was heard: without the request the filters ring on through the silent block and beyond
    phases[1] = (None, CBS, True)
    eng = new_engine(amd)
    plain = play(eng, "eq_process", x, phases, None)
    eng.close()
    assert np.array_equal(y[:, :(8 + 5) * B], plain[:, :(8 + 5) * B]) and np.array_equal(y[[0, 1, 4, 5]], plain[[0, 1, 4, 5]])
    assert not np.array_equal(y[2:4, (8 + 5) * B:], plain[2:4, (8 + 5) * B:])


def test_band_reset_pending_across_a_call_without_silence(amd, oracle):
    pa = eq_params(amd, oracle)
    phases = [(lambda e: e.set_eq_params(amd.CPQ_ALL_STREAMS, pa), 8, False),
              (lambda e: e.request_band_reset(1, 0x00000F0F), CBS, True),
              (None, 1, False),
              (None, 3, False)]         # its first callback is silent on stream 1: the reset is taken here
    x = signal(oracle, 8 + CBS + 1 + 3, silent=[(1, 8 + CBS + 1)])
    y = assert_cut_invariant(amd, x, phases)
    phases[1] = (None, CBS, True)
    eng = new_engine(amd)
    plain = play(eng, "eq_process", x, phases, None)
    eng.close()
    at = (8 + CBS + 1) * B
    assert np.array_equal(y[:, :at], plain[:, :at])                         # pending: nothing cleared while the stream plays
    assert not np.array_equal(y[2:4, at:], plain[2:4, at:])


@pytest.mark.parametrize("agc", [False, True])
def test_total_gain_change_on_one_stream(amd, oracle, agc):
    pa, louder = eq_params(amd, oracle), eq_params(amd, oracle, gain_db=4.0)
    with_agc = eq_params(amd, oracle, agc=True)

    def setup(e):
        e.set_eq_params(amd.CPQ_ALL_STREAMS, pa)
        if agc:
            e.set_eq_params(2, with_agc)

    phases = [(setup, 8, False), (lambda e: e.set_eq_params(0, louder), CBS, True), (None, 1, False)]
    x = signal(oracle, 8 + CBS + 1)
    y = assert_cut_invariant(amd, x, phases)
    phases[1] = (None, CBS, True)
    eng = new_engine(amd)
    plain = play(eng, "eq_process", x, phases, None)
    eng.close()
    assert np.array_equal(y[2:], plain[2:]) and not np.array_equal(y[0:2, 8 * B:], plain[0:2, 8 * B:])


def test_agc_reset(amd, oracle):
    pa = eq_params(amd, oracle, agc=True)
    phases = [(lambda e: e.set_eq_params(amd.CPQ_ALL_STREAMS, pa), 8, False),
              (lambda e: e.request_agc_reset(1), CBS, True),
              (None, 1, False)]
    x = signal(oracle, 8 + CBS + 1)
    y = assert_cut_invariant(amd, x, phases)
    phases[1] = (None, CBS, True)
    eng = new_engine(amd)
    plain = play(eng, "eq_process", x, phases, None)
    eng.close()
    assert np.array_equal(y[[0, 1, 4, 5]], plain[[0, 1, 4, 5]]) and not np.array_equal(y[2:4, 8 * B:], plain[2:4, 8 * B:])


def test_everything_together(amd, oracle):
    pa, louder, with_agc = eq_params(amd, oracle), eq_params(amd, oracle, gain_db=4.0), eq_params(amd, oracle, agc=True)

    def setup(e):
        e.set_eq_params(amd.CPQ_ALL_STREAMS, pa)
        e.set_eq_params(2, with_agc)

    def change(e):
        e.set_eq_bypass(1, True)
        e.request_band_reset(0, 0x000000F0)
        e.request_band_reset(2, 0x00000003)         # no silent block on stream 2: stays pending
        e.set_eq_params(0, louder)
        e.request_agc_reset(2)

    def back(e):
        e.set_eq_bypass(1, False)
        e.set_eq_bypass(2, True)                    # the fade takes stream 2's reset

    phases = [(setup, 8, False), (change, CBS, True), (back, CBS, True), (None, 1, False)]
    x = signal(oracle, 8 + 2 * CBS + 1, silent=[(0, 8 + 5)])
    assert_cut_invariant(amd, x, phases)


def test_whole_chain_with_the_output_filter_toggling_pass_through(amd, oracle):
    """Convolver bypassed: the output filter of a stream runs while its EQ does, and rests -- state kept -- while the EQ bypass is
    requested (DSPCoreDouble.cpp:453-463).  The tables toggle in front of the call that sees the request."""
    pa = eq_params(amd, oracle)

    def first(e):
        e.set_eq_params(amd.CPQ_ALL_STREAMS, pa)
        e.set_outfilter_params(amd.CPQ_ALL_STREAMS, False)
        e.enable_output_filter(True)
        e.set_conv_bypass(True)

    phases = [(None, 8, False),
              (lambda e: e.set_eq_bypass(1, True), CBS, True),
              (lambda e: e.set_eq_bypass(1, False), CBS, True),
              (None, 1, False)]
    x = signal(oracle, 8 + 2 * CBS + 1)
    y = assert_cut_invariant(amd, x, phases, fn="process", first=first)
    dry = slice((8 + 4) * B, (8 + CBS) * B)
    assert np.array_equal(y[2:4, dry], x[2:4, dry])             # neither EQ nor filter on the bypassed stream
    assert not np.array_equal(y[0:2, dry], x[0:2, dry])


def test_short_last_callback(amd, oracle):
    """CPQ_CALLS_ANY, quantum 64.  Nothing per-callback in play: 100 + 92 samples are the cascade over 192 samples, in any cut.
    While a total-gain ramp runs the engine's own cut of a ragged call -- whole callbacks, then ONE callback of the rest -- makes
    a call of 100 samples the calls of 64 and 36, ramp and all.  (enqueueEq cuts every such call before enqueueEqRange sees it,
    so the range's "must be whole callbacks" refusals cannot be reached through an entry point: the call succeeds.)"""
    pa, louder = eq_params(amd, oracle), eq_params(amd, oracle, gain_db=4.0)
    x = signal(oracle, 9)[:, :192 + 100 + 128]
    outs = []
    for sizes, ramp_sizes in [([100, 92], [100]), ([192], [64, 36]), ([64, 64, 64], [64, 36])]:
        eng = amd.BatchedEngine(S, block_size=B, max_ir_len=512, max_blocks_per_call=CBS, sample_rate=RATE, call_mode=amd.CPQ_CALLS_ANY)
        eng.set_eq_mode(amd.CPQ_EQ_MODE_SEQUENTIAL)
        eng.set_eq_params(amd.CPQ_ALL_STREAMS, pa)
        ys, pos = [], 0
        for k, n in enumerate(sizes + ramp_sizes + [128]):
            if k == len(sizes):
                eng.set_eq_params(0, louder)        # the ramp starts with the next callback
            ys.append(eng.eq_process(np.ascontiguousarray(x[:, pos:pos + n])))
            pos += n
        outs.append(np.concatenate(ys, axis=1))
        eng.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert np.abs(outs[0]).max() > 1e-3
