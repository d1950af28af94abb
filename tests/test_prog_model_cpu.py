"""The numpy model of the programme loudness (tests/prog_model.py) alone: the EBU compliance signals it must read correctly, and
the properties of the GPU tests' inputs (tests/prog_inputs.py) that keep a device comparison from flipping a decision.

EBU Tech 3341 / 3342 bars are EBU's own.  The K-weighting is the reference's cookbook design (cpq_meter_kweighting), not
BS.1770's coefficient table; what that leaves at 1 kHz is printed by the tests and recorded in DESIGN.md 4.15."""
import math

import numpy as np

import prog_inputs as I
import prog_model as P


def _figures(x, rate):
    return P.finish(P.hop_sums(x, rate)[0], P.hop_len(rate))


def test_ebu_3341_case_1():
    """stereo 1 kHz sine at -23 dBFS per channel, 20 s at 48 kHz: -23.0 +- 0.1 LUFS"""
    r = _figures(I.ebu_3341_1(48000, 20), 48000)
    print(f"EBU 3341 case 1: integrated {r['integrated']:.4f} LUFS (momentary max {r['momentary_max']:.4f})")
    assert abs(r["integrated"] + 23.0) <= 0.1


def test_ebu_3341_case_3():
    """-36 dBFS for 10 s, -23 dBFS for 60 s, -36 dBFS for 10 s: -23.0 +- 0.1 LUFS (the relative gate drops the quiet ends)"""
    r = _figures(I.ebu_3341_3(48000, 10, 60), 48000)
    print(f"EBU 3341 case 3: integrated {r['integrated']:.4f} LUFS, gate {r['relative_gate']:.4f}, {r['n_rel']} of {r['n_abs']} blocks")
    assert abs(r["integrated"] + 23.0) <= 0.1
    assert r["n_rel"] < r["n_abs"] == r["n_blocks"]


def test_ebu_3342_case_1():
    """20 s at -20 dBFS, then 20 s at -30 dBFS: LRA 10 +- 1 LU"""
    r = _figures(I.ebu_3342_1(48000, 20), 48000)
    print(f"EBU 3342 case 1: LRA {r['range']:.4f} LU from {r['n_short_kept']} short-term blocks")
    assert abs(r["range"] - 10.0) <= 1.0


def test_percentile_rounding_and_empty_sets():
    H = 800
    assert P.finish(np.zeros(3), H)["n_blocks"] == 0 and P.finish(np.zeros(3), H)["integrated"] == -math.inf
    quiet = P.finish(np.zeros(50), H)
    assert quiet["n_blocks"] == 47 and quiet["n_abs"] == 0 and quiet["integrated"] == -math.inf and quiet["range"] == 0.0
    assert quiet["momentary_max"] == -math.inf and quiet["relative_gate"] == -math.inf
    # 11 kept short-term values that rise: indices round(0.1 * 10) = 1 and round(0.95 * 10) = 9.5 -> 10 (half up)
    E = (1.0 + 0.01 * np.arange(130)) * H
    r = P.finish(E, H)
    zs = P.blocks(E, 30, H)[0::10]
    assert r["n_short_kept"] == 11 == len(zs) and r["z_lo"] == zs[1] and r["z_hi"] == zs[10]
    # 21 of them: round(2.0) = 2 and round(19.0) = 19
    r = P.finish((1.0 + 0.01 * np.arange(230)) * H, H)
    zs = P.blocks((1.0 + 0.01 * np.arange(230)) * H, 30, H)[0::10]
    assert r["n_short_kept"] == 21 and r["z_lo"] == zs[2] and r["z_hi"] == zs[19]


def test_gpu_inputs_stand_clear_of_the_gates():
    """every block of every GPU input lies at least 0.5 LU from the gates that decide about it, so that a hop sum that differs
    from the model's in its last bits cannot move a block across; the range inputs' kept short-term values are further apart
    than any device difference (1e-6 LU; the device bar on a loudness is below 1e-11 LU)"""
    ref = I.reference()
    for name, v in ref.items():
        r = P.finish(v["E"], I.H)
        print(f"{name}: {r['n_hops']} hops, blocks {r['n_blocks']} / {r['n_abs']} / {r['n_rel']}, kept {r['n_short_kept']}, "
              f"I {r['integrated']:.3f}, LRA {r['range']:.3f}, gate margin {r['gate_margin']:.3f} LU, short gap {r['short_gap']:.3g} LU")
        assert r["gate_margin"] >= 0.5, name
    for name in ("ramp40", "main60"):
        assert P.finish(ref[name]["E"], I.H)["short_gap"] >= 1e-3, name
    assert P.finish(ref["ramp40"]["E"], I.H)["n_short_kept"] == 40
    assert P.finish(ref["short_399ms"]["E"], I.H)["n_blocks"] == 0
    assert P.finish(ref["hops_4"]["E"], I.H)["n_blocks"] == 1 and P.finish(ref["hops_30"]["E"], I.H)["n_short_kept"] == 1
    for name in ("silence", "tone_minus80"):
        r = P.finish(ref[name]["E"], I.H)
        assert r["n_blocks"] > 0 and r["n_abs"] == 0
    # the shortened EBU signals behave as the full ones do.  At 8000 Hz the cookbook K-weighting reads a 1 kHz tone 0.18 LU low
    # (DESIGN.md 4.15), so case 3 is held to case 1 at that rate, not to -23.0: the gate drops the quiet ends, and the six blocks
    # that straddle a level change (of 103 kept, none below a quarter of the plateau's power) lower the mean by less than 0.2 LU
    one, three = P.finish(ref["ebu_3341_1"]["E"], I.H), P.finish(ref["ebu_3341_3"]["E"], I.H)
    assert abs(one["integrated"] + 23.0) <= 0.25 and abs(three["integrated"] - one["integrated"]) <= 0.2 and three["n_rel"] < three["n_abs"]
    assert abs(P.finish(ref["ebu_3342_1"]["E"], I.H)["range"] - 10.0) <= 1.0


def test_fp64_model_against_long_double():
    """d_ref per input: the largest distance of the fp64 sequential model's hop sums from the long-double run's.  The recurrence's
    rounding is amplified by the RLB poles (radius 0.995 at 48 kHz), so d_ref is a multiple of 2^-53 E, but a small one:
    asserted below 1e-10 of the input's largest hop sum."""
    refs = dict(I.reference())
    for rate in (44100, 48000):
        refs[f"rate_{rate}"] = I.rate_reference(rate)
    for name, v in refs.items():
        top = float(np.max(v["E"])) if len(v["E"]) else 0.0
        print(f"{name}: d_ref {v['d_ref']:.3e}, largest hop sum {top:.3e}, ratio {v['d_ref'] / top if top else 0.0:.3e}")
        assert np.isfinite(v["d_ref"]) and v["d_ref"] <= 1e-10 * top
        # the figures of the two runs agree far inside the EBU bars
        hop = int(name[5:]) // 10 if name.startswith("rate_") else I.H
        a, b = P.finish(v["E"], hop), P.finish(v["E_ld"], hop, np.longdouble)
        for key in ("n_blocks", "n_abs", "n_rel", "n_short_kept"):
            assert a[key] == b[key], (name, key)
        if a["n_rel"]:
            assert abs(a["integrated"] - b["integrated"]) <= 1e-9
