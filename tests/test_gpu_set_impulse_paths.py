"""cpq_conv_set_impulse on every path an IR can take -- uniform, layered (time-varying), plan group -- and the plan groups' chunk-wise
read, pinned bit for bit between two engines of one build.

The parity suites compare with the oracle at 1e-13: a spectrum row left over from a longer IR, a history that was not cleared or a
changed rounding in the ring read can hide below that.  Here both sides of every comparison are engines of this build that run the
same kernels on the same data, so the comparison is np.array_equal.  Shapes are the smallest that reach the code: 2 streams,
block 64 / 512 (1024 for layered mode, which needs a tail partition longer than the IR in front of it), a handful of calls.

The identity "one long call == the same samples in block_size calls" for plans of 1, 2 and 3 layers is asserted here
(test_tail_layer_counts_on_the_plan_group_read_path): tests/test_gpu_ragged.py compares such calls with the oracle, not with each other.

tests/golden/set_impulse_scale_signs.npz: np.signbit of every output sample of scale_case() per mode, packed with np.packbits,
recorded on an MI355X from the build in front of the change that split cpq_conv_set_impulse into steps.  The native path zeroes
the head taps and then scales them, the other two scale and then zero: at a negative scale the zeroed taps are -0.0 on the one
and +0.0 on the others, and the record holds what that does to the output's zeros.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "set_impulse_scale_signs.npz")
MODES = ["uniform", "any", "layered"]


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def pcm(O, streams, n, first=0):
    return np.stack([O.gen_pcm(n, stream=first + c // 2, channel=c % 2) for c in range(2 * streams)])


def stereo_ir(O, taps, stream):
    return [O.gen_ir(taps, stream=stream, channel=ch) for ch in range(2)]


def run(eng, x, sizes):
    ys, pos = [], 0
    for n in sizes:
        ys.append(eng.conv_process(np.ascontiguousarray(x[:, pos:pos + n])))
        pos += n
    assert pos == x.shape[1]
    return np.concatenate(ys, axis=1)


def engine(amd, mode, streams, max_ir_len, blocks_per_call):
    """uniform: block 64, whole blocks; any: block 64, CPQ_CALLS_ANY (every stream in a plan group); nuc: the reference's schedule;
    layered: block 1024, where the default tail start makes an IR above 5760 taps time-varying"""
    block = 1024 if mode == "layered" else 64
    kw = {}
    if mode == "any":
        kw["call_mode"] = amd.CPQ_CALLS_ANY
    if mode == "nuc":
        kw["schedule"] = amd.CPQ_SCHED_REFERENCE_NUC
    return amd.BatchedEngine(streams, block_size=block, max_ir_len=max_ir_len, max_blocks_per_call=blocks_per_call, **kw), block


def call_sizes(mode, block, calls, blocks_per_call):
    if mode == "any":           # ragged: part chunks, a one-sample call
        return ([blocks_per_call * block, block + 37, 1, block - 38] * calls)[:calls]
    return [blocks_per_call * block] * calls


@pytest.mark.parametrize("mode", MODES)
def test_reload_over_a_longer_ir(amd, oracle, mode):
    """A 1-partition IR loaded over a 3-partition one sounds like the short IR alone: the stale partitions are gone.  Layered mode
    takes one IR length per engine, so there the second IR has the first one's length and other taps (its slot is cleared whole)."""
    O = oracle
    S = 2
    if mode == "layered":
        long_len = short_len = 6000
        assert amd.nuc_plan(long_len, 1024).lti_valid == 0 and amd.nuc_plan(long_len, 1024).num_layers == 2
    else:
        long_len, short_len = 3 * 64 - 10, 50
    outs = []
    for reload_first in (True, False):
        eng, block = engine(amd, mode, S, long_len, 2)
        for s in range(S):
            if reload_first:
                eng.set_impulse(s, *stereo_ir(O, long_len, 40 + s))
            eng.set_impulse(s, *stereo_ir(O, short_len, 50 + s))
        sizes = call_sizes(mode, block, 6, 2)
        outs.append(run(eng, pcm(O, S, sum(sizes)), sizes))
        eng.close()
    assert np.array_equal(outs[0], outs[1])
    assert np.abs(outs[0]).max() > 1e-3


@pytest.mark.parametrize("mode", ["uniform", "any"])
def test_one_stream_reloaded_while_the_other_plays(amd, oracle, mode):
    """Stream 1 is loaded again (same IR) after two calls: stream 0 does not notice, stream 1 starts over like a new convolver."""
    O = oracle
    S, taps = 2, 200
    irs = [stereo_ir(O, taps, 60 + s) for s in range(S)]
    eng, block = engine(amd, mode, S, 400, 2)
    sizes = call_sizes(mode, block, 6, 2)
    x = pcm(O, S, sum(sizes))
    split = sum(sizes[:2])

    def loaded(ir0=None):
        e, _ = engine(amd, mode, S, 400, 2)
        e.set_impulse(0, *(ir0 or irs[0]))
        e.set_impulse(1, *irs[1])
        return e

    for s in range(S):
        eng.set_impulse(s, *irs[s])
    y_a = run(eng, x[:, :split], sizes[:2])
    eng.set_impulse(1, *irs[1])
    y_b = run(eng, x[:, split:], sizes[2:])
    eng.close()
    plain = loaded()
    y_plain = run(plain, x, sizes)
    plain.close()
    assert np.array_equal(np.concatenate([y_a, y_b], axis=1)[:2], y_plain[:2])
    # the fresh engine's stream 0 has another IR length: in a plan-group engine stream 1 then sits in a group of its own, as
    # it does after the reload (same kernels on both sides)
    fresh = loaded(stereo_ir(O, taps + 100, 60))
    y_fresh = run(fresh, x[:, split:], sizes[2:])
    fresh.close()
    assert np.array_equal(y_b[2:], y_fresh[2:])
    assert not np.array_equal(y_b[2:], y_plain[2:, split:])        # the reload was heard


def test_plan_group_to_main_path_and_back(amd, oracle):
    """A FilterSpec plan with a tail layer puts the stream in a plan group; the next load without a spec returns it to the main path,
    which then sounds as if the first load had never happened."""
    O = oracle
    S, taps, block = 2, 3000, 64
    spec = amd.FilterSpec.defaults()
    with_spec, without = amd.nuc_plan(taps, block, False, spec), amd.nuc_plan(taps, block)
    assert with_spec.num_layers == 2 and with_spec.part_size[1] == 512          # tail layer: plan group
    assert without.lti_valid == 1 and without.part_size[0] == block            # legal on the uniform path
    outs = []
    for spec_first in (True, False):
        eng, _ = engine(amd, "uniform", S, taps, 4)
        for s in range(S):
            if spec_first:
                eng.set_impulse(s, *stereo_ir(O, taps, 70 + s), spec=spec)
            eng.set_impulse(s, *stereo_ir(O, taps, 70 + s))
        sizes = [4 * block] * 6
        outs.append(run(eng, pcm(O, S, sum(sizes)), sizes))
        eng.close()
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("mode", ["uniform", "any"])
def test_shared_ir_equals_per_stream_loading(amd, oracle, mode):
    O = oracle
    S, taps = 3, 150
    ir = stereo_ir(O, taps, 80)
    outs = []
    for shared in (True, False):
        eng, block = engine(amd, mode, S, taps, 2)
        if shared:
            eng.set_impulse(amd.CPQ_ALL_STREAMS, *ir)
        else:
            for s in range(S):
                eng.set_impulse(s, *ir)
        sizes = call_sizes(mode, block, 5, 2)
        outs.append(run(eng, pcm(O, S, sum(sizes)), sizes))
        eng.close()
    assert np.array_equal(outs[0], outs[1])


def scale_case(amd, O, mode):
    """scale -0.5 with the direct head on an IR that is all head (24 taps; layered mode needs 6000, of which 32 are head), native = the reference's own schedule:
    (output rows, IRs, input, block).  The first call is silence, so that zeros of either sign can show."""
    S = 2
    taps = 6000 if mode == "layered" else 24
    eng, block = engine(amd, "nuc" if mode == "native" else mode, S, taps, 2)
    irs = [stereo_ir(O, taps, 90 + s) for s in range(S)]
    for s in range(S):
        eng.set_impulse(s, *irs[s], scale=-0.5, direct_head=True)
    sizes = [2 * block] * 6
    x = pcm(O, S, sum(sizes))
    x[:, :sizes[0]] = 0.0
    y = run(eng, x, sizes)
    eng.close()
    return y, irs, x, block


@pytest.mark.parametrize("mode", ["uniform", "native", "layered"])
def test_negative_scale_with_the_direct_head(amd, oracle, mode):
    O = oracle
    y, irs, x, block = scale_case(amd, O, mode)
    for c in range(y.shape[0]):
        nuc = O.Nuc()
        assert nuc.set_impulse(irs[c // 2][c % 2], block, scale=-0.5, direct=True)
        ref = nuc.run(x[c], block)
        nuc.close()
        err = float(np.sqrt(np.mean(np.square(y[c] - ref))))
        assert err <= 1e-13 and np.abs(ref).max() > 1e-3, err
    with np.load(GOLDEN) as g:
        signs = np.unpackbits(g[mode])[:y.size].reshape(y.shape).astype(bool)
    assert np.array_equal(np.signbit(y), signs)


# taps: the shortest IRs whose plans at block 512 have 1, 2 and 3 layers (layer 0 ends at 5760 taps, layer 1 at 5760 + 64 * 4096);
# call x calls: enough input for the last layer's first block (4096, 32768 samples) to come out of its delay line
@pytest.mark.parametrize("first", [0, 300])
@pytest.mark.parametrize("layers,taps,call,calls", [(1, 3000, 2048, 4), (2, 6000, 2048, 6), (3, 268000, 8192, 5)])
def test_tail_layer_counts_on_the_plan_group_read_path(amd, oracle, layers, taps, call, calls, first):
    """One call of many blocks == the same samples in block_size calls, for every count of tail layers.  first = 0: whole blocks on
    an empty ring, layer 0's inverse transform stores the output rows (and adds the tails' blocks); first = 300: a ragged call in
    front, after which every call goes through the output ring and the chunk-wise read-add.  mac_tile = 4: left to itself the
    engine picks the multiply-accumulate kernel by the blocks in the call, and the kernels do not promise each other's rounding."""
    O = oracle
    S, block = 2, 512
    assert amd.nuc_plan(taps, block).num_layers == layers
    irs = [stereo_ir(O, taps, 30 + s) for s in range(S)]
    head = [first] if first else []
    x = pcm(O, S, first + call * calls)
    outs = []
    for sizes in (head + [call] * calls, head + [block] * (call * calls // block)):
        eng = amd.BatchedEngine(S, block_size=block, max_ir_len=taps, max_blocks_per_call=call // block, call_mode=amd.CPQ_CALLS_ANY,
                                mac_tile=4)
        for s in range(S):
            eng.set_impulse(s, *irs[s])
        outs.append(run(eng, x, sizes))
        eng.close()
    assert np.array_equal(outs[0], outs[1])
    assert np.abs(outs[0][:, -call:]).max() > 1e-3
