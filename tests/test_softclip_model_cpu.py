"""CPU tests of the soft clipper's statements: tests/softclip_model.py (numpy, both arithmetic paths) and the host restatement
(softclip_design.cpp through cpq_soft_clip_host) against tests/golden/softclip_ref.npz, which holds what the reference's own
softClipBlockAVX2 computed -- bit for bit, a NaN matching a NaN; and softclip_design.cpp under the address and
undefined-behaviour sanitizers as a program of its own.

The recording: four amounts, block lengths 1, 2, 3, 4, 5, 7, 8, 64 and 882 over one input of 949 samples per amount (at 882 a
whole block and a ragged one of 64 body + 3 tail samples): noise at +-2 with, three times over (from sample 0, from sample 400
and up to the last sample), both signs of the curve's three corners and their neighbours one ulp either side, tanh arguments at
4.5, beside it and far beyond, zeros, denormals, infinities, and a NaN."""
import os
import subprocess

import numpy as np
import pytest

import softclip_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(HERE, "golden", "softclip_ref.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def cases(ref):
    for k, amount in enumerate(ref["amounts"]):
        for block in ref["blocks"]:
            yield k, float(amount), int(block), ref[f"input_{k}"], ref[f"output_{k}_{int(block)}"]


def test_the_recording_holds_what_it_should(ref):
    assert [float(a) for a in ref["amounts"]] == [0.0, float(np.float32(0.2)), 0.5, 1.0]
    assert [int(b) for b in ref["blocks"]] == [1, 2, 3, 4, 5, 7, 8, 64, 882]
    for k, amount in enumerate(ref["amounts"]):
        x = ref[f"input_{k}"]
        thr, knee, _ = ref[f"params_{k}"]
        finite = x[np.isfinite(x)]
        assert x.size == 949 and 1.9 < np.abs(x[60:400]).max() <= 2.0 and x[60:400].min() < -1.9       # the noise between the planted runs
        for v in (thr - knee, thr, thr + knee):                # exactly at and one ulp either side, both signs
            for w in (np.nextafter(v, 0.0), v, np.nextafter(v, 4.0)):
                assert np.count_nonzero(x == w) >= 3 and np.count_nonzero(x == -w) >= 3
        for arg in ((np.abs(finite) - thr) / knee, (np.abs(finite) - thr) * (1.0 / knee)):     # as the tail and as the body form it
            # the nine doubles around threshold + 4.5 knee: the closest arguments either side of 4.5 there are, and 4.5 itself
            # where a sample gives it (|x| moves in steps of an ulp, the argument in steps of ulp / knee: only amount 1.0 hits it)
            assert np.count_nonzero((arg > 4.5 - 2e-14) & (arg < 4.5)) >= 4 and np.count_nonzero((arg > 4.5) & (arg < 4.5 + 2e-14)) >= 4
            assert np.count_nonzero(arg == 4.5) >= (1 if float(amount) == 1.0 else 0) and np.count_nonzero(arg > 4.6) >= 10
        assert np.isnan(x).sum() == 3 and np.isposinf(x).sum() == 3 and np.isneginf(x).sum() == 3
        assert np.count_nonzero((x == 0.0) & np.signbit(x)) == 3 and np.count_nonzero((x == 0.0) & ~np.signbit(x)) == 3
        assert np.count_nonzero((np.abs(x) > 0.0) & (np.abs(x) < 2.2250738585072014e-308)) >= 12


def test_parameters(ref, amd):
    for k, amount in enumerate(ref["amounts"]):
        assert list(M.params(amount)) == list(ref[f"params_{k}"]) == list(amd.soft_clip_params(float(amount)))


def test_model_against_the_recording(ref):
    n = 0
    for k, amount, block, x, want in cases(ref):
        assert M.same(M.clip(x, block, amount), want), (amount, block)
        n += 1
    assert n == 36


def test_host_restatement_against_the_recording(ref, amd):
    for k, amount, block, x, want in cases(ref):
        assert M.same(amd.soft_clip_host(x, block, amount), want), (amount, block)


def test_below_the_clip_start_samples_come_back_identical(ref):
    for k, amount, block, x, want in cases(ref):
        thr, knee, _ = ref[f"params_{k}"]
        quiet = np.abs(x) <= thr - knee
        assert quiet.sum() > 50
        assert np.array_equal(want[quiet].view(np.uint64), x[quiet].view(np.uint64))        # -0.0 and denormals included
        loud = np.isfinite(x) & (np.abs(x) > thr + 0.01)        # at the threshold itself tanh(0) = 0 gives the sample back
        assert loud.sum() > 100 and np.all(np.abs(want[loud]) < np.abs(x[loud]))
    for amount in (0.0, 0.3, 1.0):
        thr, knee, _ = M.params(amount)
        x = np.linspace(-(thr - knee), thr - knee, 1001)
        assert np.array_equal(M.body(x, amount), x) and np.array_equal(M.tail(x, amount), x)


def test_body_and_tail_differ_in_bits(ref):
    """the two paths are really two: all-tail blocks (1, 2, 3) against all-body blocks (4, 8, 64) of the same recorded input"""
    for k, amount in enumerate(ref["amounts"]):
        x = ref[f"input_{k}"]
        tails, bodies = ref[f"output_{k}_1"], ref[f"output_{k}_4"][:948]
        assert M.same(tails, ref[f"output_{k}_2"]) and M.same(tails, ref[f"output_{k}_3"])
        assert M.same(bodies, ref[f"output_{k}_8"][:948]) and M.same(bodies[:896], ref[f"output_{k}_64"][:896])
        both = ~np.isnan(tails[:948]) & ~np.isnan(bodies)
        differ = both & (tails[:948] != bodies)
        print(f"amount {float(amount):.1f}: body and tail differ on {differ.sum()} of {both.sum()} recorded samples")
        assert differ.sum() >= 1
        assert M.same(M.tail(x, amount), tails) and M.same(M.body(x[:948], amount), bodies)
        # beyond 4.5 the scalar tanh is 1 and the vector one the Pade value at 4.5: the tail reaches threshold + knee, the body not
        thr, knee, _ = ref[f"params_{k}"]
        far = np.isfinite(x[:948]) & ((np.abs(x[:948]) - thr) / knee > 4.5) & (x[:948] > 0.0)
        assert far.sum() >= 5 and np.all(tails[:948][far] == thr + knee) and np.all(bodies[far] < thr + knee)


def test_the_block_walk_picks_the_path_by_the_index_in_the_callback():
    assert M.tail_mask(11, 8).tolist() == [False] * 8 + [True] * 3
    assert M.tail_mask(13, 5).tolist() == ([False] * 4 + [True]) * 2 + [True] * 3
    assert M.tail_mask(8, 4).tolist() == [False] * 8 and M.tail_mask(3, 64).tolist() == [True] * 3
    assert M.tail_mask(7, 7).tolist() == [False] * 4 + [True] * 3


def test_softclip_design_under_sanitizers(tmp_path):
    exe = tmp_path / "softclip_design_check"
    csrc = os.path.join(ROOT, "convopeq_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "sanitize", "softclip_design_check.cpp"), os.path.join(csrc, "softclip_design.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 failed checks" in r.stdout and "FAILED" not in r.stdout
