"""The launch sequences a plan group's call can take (convopeq_amd/csrc/nuc_replay.hpp decides, engine_native.cpp carries out), each
pinned twice: by the number of launches per profile scope in every call, and by the output against the oracle at the bar
tests/test_gpu_ragged.py uses for the same path (1e-13 RMS, the reference's zero-filled samples exactly zero).

2 streams with private IRs, block_size 512 (the partition size at which layer 0's forward transform can carry the other layers'
accumulation and the call's table, and its inverse transform can add the tails), CPQ_CALLS_ANY, IRs of 3000 / 6000 / 268000 taps
for plans of 1 / 2 / 3 layers, at most 8 blocks per call (16 with 3 layers, whose last layer needs 32768 samples for its first
block).  One engine per scenario:
  fresh-1          whole-block calls on a fresh group: layer 0 straight from the input and held back, its launch carries the table,
                   the inverse transform writes the output rows (direct, hold0, the table rides)
  ragged-first-1/2 the same calls after a first call of 300 samples: the ring is not empty -- gather launch, ring write and chunk-wise
                   read; with a tail layer the read waits for the tails' read-add (getDeferred)
  fresh-2/3        tail layers and no direct head: the tails run ahead of layer 0, whose transform adds their blocks (addTails)
  head-2/3         the same with the direct head on: the tails run behind it, their read-add is a pass of its own
  fresh-3, head-3  their 16-block calls have 66 table entries, more than ride with a launch: the table goes out as a staged upload
  isolate-2        processor level: one stream bypassed for a call and released, which moves it to a group of its own with the
                   state it had

EXPECTED holds, per call, the launches of (k_rfft_fwd_ols, k_fdl_mac, k_fdl_mac_dcnyq, k_rfft_inv_ols, k_convproc_mix).  The
figures were measured, not derived: this file was run on an MI355X against the build in front of the change that moved the plan
of a call into nuc_replay.hpp, and the counts it showed were recorded here; the build with that change shows the same.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 512
SCOPES = ("k_rfft_fwd_ols", "k_fdl_mac", "k_fdl_mac_dcnyq", "k_rfft_inv_ols", "k_convproc_mix")
TAPS = {1: 3000, 2: 6000, 3: 268000}
TWO = [4096, 2048, 4096, 4096]                          # layer 1 straight from the input, accumulating, a block from the accumulator
THREE = [4096, 4096, 8192, 8192, 8192, 8192]            # the last call holds layer 2's first block
SCENARIOS = {
    "fresh-1": dict(layers=1, calls=[2048, 4096, 512]),
    "ragged-first-1": dict(layers=1, calls=[300, 2048, 4096]),
    "ragged-first-2": dict(layers=2, calls=[300] + TWO),
    "fresh-2": dict(layers=2, calls=TWO),
    "fresh-3": dict(layers=3, calls=THREE),
    "head-2": dict(layers=2, calls=TWO, direct=True),
    "head-3": dict(layers=3, calls=THREE, direct=True),
    "isolate-2": dict(layers=2, calls=[4096] * 4, bypass=[False, True, False, False]),
}
EXPECTED = {
    "fresh-1": [(1, 1, 0, 1, 1), (1, 1, 0, 1, 1), (1, 1, 0, 1, 1)],
    "ragged-first-1": [(0, 0, 0, 0, 3), (1, 1, 0, 1, 3), (1, 1, 0, 1, 3)],
    "ragged-first-2": [(0, 0, 0, 0, 2), (2, 2, 0, 2, 3), (1, 1, 0, 1, 2), (2, 2, 0, 2, 3), (2, 2, 0, 2, 3)],
    "fresh-2": [(2, 2, 0, 2, 0), (1, 1, 0, 1, 0), (2, 2, 0, 2, 1), (2, 2, 0, 2, 1)],
    "fresh-3": [(2, 2, 0, 2, 0), (2, 2, 0, 2, 0), (2, 2, 1, 2, 0), (2, 2, 1, 2, 0), (3, 3, 1, 3, 0), (2, 2, 1, 2, 0)],
    "head-2": [(2, 2, 0, 2, 3), (1, 1, 0, 1, 3), (2, 2, 0, 2, 4), (2, 2, 0, 2, 4)],
    "head-3": [(2, 2, 0, 2, 3), (2, 2, 0, 2, 3), (2, 2, 1, 2, 3), (2, 2, 1, 2, 3), (3, 3, 1, 3, 3), (2, 2, 1, 2, 3)],
    "isolate-2": [(2, 2, 0, 2, 2), (2, 2, 0, 2, 4), (4, 4, 0, 4, 6), (4, 4, 0, 4, 6)],
}


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def inputs(O, name):
    sc = SCENARIOS[name]
    taps = TAPS[sc["layers"]]
    irs = [[O.gen_ir(taps, stream=40 + s, channel=ch) for ch in range(2)] for s in range(2)]
    x = np.stack([O.gen_pcm(sum(sc["calls"]), stream=40 + c // 2, channel=c % 2) for c in range(4)])
    return irs, x


def play(amd, O, name):
    """-> the output rows and, per call, the launches of every scope"""
    sc = SCENARIOS[name]
    irs, x = inputs(O, name)
    direct = sc.get("direct", False)
    eng = amd.BatchedEngine(2, block_size=BLOCK, max_ir_len=TAPS[sc["layers"]], max_blocks_per_call=16 if sc["layers"] == 3 else 8,
                            call_mode=amd.CPQ_CALLS_ANY)
    for s in range(2):
        eng.set_impulse(s, irs[s][0], irs[s][1], direct_head=direct)
    assert eng.plan().num_layers == sc["layers"]
    if "bypass" in sc:
        eng.set_convproc_params(amd.CPQ_ALL_STREAMS, mix=1.0)
    eng.profile_enable(True)
    ys, counts, pos = [], [], 0
    for k, n in enumerate(sc["calls"]):
        seg = np.ascontiguousarray(x[:, pos:pos + n])
        eng.profile_reset()
        if "bypass" in sc:
            eng.set_convproc_params(1, mix=1.0, bypassed=sc["bypass"][k])
            ys.append(eng.convproc_process(seg))
        else:
            ys.append(eng.conv_process(seg))
        prof = eng.profile_read()
        counts.append(tuple(int(prof[scope][0]) for scope in SCOPES))
        pos += n
    eng.close()
    return np.concatenate(ys, axis=1), counts


def reference(O, name):
    """Add + Get per chunk of BLOCK samples inside every call; a bypassed stream's convolver is not called and its output is the
    dry signal behind the algorithm latency (tests/test_gpu_ragged.py::test_per_stream_bypass_rests_one_convolver)"""
    sc = SCENARIOS[name]
    irs, x = inputs(O, name)
    direct = sc.get("direct", False)
    ref = np.empty_like(x)
    wet_g = O.lib().orc_equal_power_sin(1.0) if "bypass" in sc else 1.0
    for c in range(4):
        nuc = O.Nuc()
        assert nuc.set_impulse(irs[c // 2][c % 2], BLOCK, direct=direct)
        dry = np.concatenate([np.zeros(BLOCK), x[c][:-BLOCK]])
        pos = 0
        for k, n in enumerate(sc["calls"]):
            if "bypass" in sc and c // 2 == 1 and sc["bypass"][k]:
                ref[c, pos:pos + n] = dry[pos:pos + n]
            else:
                for o in range(0, n, BLOCK):
                    m = min(BLOCK, n - o)
                    nuc.add(x[c, pos + o:pos + o + m])
                    out, _ = nuc.get(m)
                    ref[c, pos + o:pos + o + m] = out * wet_g
            pos += n
        nuc.close()
    return ref


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_launches_per_call_and_output(amd, oracle, name):
    y, counts = play(amd, oracle, name)
    print(f"{name}: {counts}")
    assert counts == EXPECTED[name]
    ref = reference(oracle, name)
    for c in range(4):
        err = float(np.sqrt(np.mean(np.square(y[c] - ref[c]))))
        print(f"{name} channel {c}: rms err {err:.3e}")
        assert err <= 1e-13, (c, err)
        if "bypass" not in SCENARIOS[name]:                         # (the processor level's own test asks for the RMS alone)
            zeros = ref[c] == 0.0
            assert np.array_equal(y[c][zeros], ref[c][zeros])       # zero-filled samples stay exactly zero
    assert np.abs(ref[:, -BLOCK:]).max() > 1e-3
