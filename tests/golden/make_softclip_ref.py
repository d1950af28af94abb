"""Records tests/golden/softclip_ref.npz from the reference's own soft clipper through softclip_probe.cpp.
    python tests/golden/make_softclip_ref.py <reference source tree>
musicalSoftClipScalar and softClipBlockAVX2 sit in an anonymous namespace of a translation unit that needs the whole engine, so
the stretch of that file from musicalSoftClipScalar to the end of softClipBlockAVX2 is cut into a temporary directory, where the
probe includes it.  The cut, the probe binary and the directory are not kept; only inputs, parameters and outputs are."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join("src", "audioengine", "AudioEngine.Processing.DSPCoreDouble.cpp")
AMOUNTS = (0.0, 0.2, 0.5, 1.0)
BLOCKS = (1, 2, 3, 4, 5, 7, 8, 64, 882)          # every residue mod 4; all tail, all body and both
N = 882 + 64 + 3                                  # at block 882: one whole block and a ragged one of 64 body + 3 tail samples


def cut_stretch(ref):
    """the lines from musicalSoftClipScalar's first to the closing brace of softClipBlockAVX2"""
    lines = open(os.path.join(ref, SOURCE), encoding="utf-8").read().split("\n")
    first = next(i for i, l in enumerate(lines) if l.startswith("inline double musicalSoftClipScalar("))
    block = next(i for i, l in enumerate(lines) if l.startswith("void softClipBlockAVX2("))
    assert first < block
    depth, seen, last = 0, False, None
    for i in range(block, len(lines)):
        depth += lines[i].count("{") - lines[i].count("}")
        seen = seen or "{" in lines[i]
        if seen and depth == 0:
            last = i
            break
    assert last is not None
    return "\n".join(lines[first:last + 1]) + "\n"


def params(amount):
    sat = float(np.float32(amount))
    return 0.95 - 0.45 * sat, 0.05 + 0.35 * sat, 0.10 * sat


def make_input(amount, seed):
    """noise at +-2 with, from sample 0 and again up to the last sample, both signs of: the three corners of the curve and their
    neighbours one ulp either side, tanh arguments at 4.5, just either side of it and far beyond, zeros, denormals, NaN, Inf"""
    thr, knee, _ = params(amount)
    x = np.random.default_rng(seed).uniform(-2.0, 2.0, N)
    pos = []
    for v in (thr - knee, thr, thr + knee):
        pos += [np.nextafter(v, 0.0), v, np.nextafter(v, 4.0)]
    edge = thr + 4.5 * knee                          # the nine doubles around it: (|x| - thr) / knee and (|x| - thr) * (1 / knee)
    for _ in range(4):                               # each land on 4.5 itself for some of them, and either side for the others
        edge = np.nextafter(edge, 0.0)
    for _ in range(9):
        pos.append(edge)
        edge = np.nextafter(edge, 4.0)
    pos += [thr + 4.4999 * knee, thr + 4.5001 * knee, thr + 5.0 * knee, thr + 40.0 * knee, 100.0, 1.0e300,
            0.0, 5.0e-324, 1.0e-310, 2.2250738585072014e-308, np.inf]
    special = np.array([s * v for v in pos for s in (1.0, -1.0)] + [np.nan])
    x[:special.size] = special
    x[N - special.size:] = special[::-1]
    x[400:400 + special.size] = special          # at block 882 these are body samples, the ones at the end tail samples
    return x


def main(ref):
    out = {"amounts": np.array(AMOUNTS, dtype=np.float32), "blocks": np.array(BLOCKS, dtype=np.int32)}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "softclip_cut.inc"), "w", encoding="utf-8") as f:
            f.write(cut_stretch(ref))
        exe = os.path.join(tmp, "softclip_probe")
        subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-msse4.1", "-mavx2", "-mfma",
                        "-I" + os.path.join(HERE, "juce_shim"), "-I" + os.path.join(ref, "src"), "-I" + tmp,
                        os.path.join(HERE, "softclip_probe.cpp"), "-o", exe], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        for k, amount in enumerate(AMOUNTS):
            x = make_input(amount, 100 + k)
            x.tofile(fin)
            out[f"input_{k}"] = x
            for block in BLOCKS:
                subprocess.run([exe, repr(float(np.float32(amount))), str(block), fin, fout, str(N)], check=True)
                y = np.fromfile(fout)
                assert y.size == 3 + N
                if block == BLOCKS[0]:
                    out[f"params_{k}"] = y[:3].copy()
                assert np.array_equal(out[f"params_{k}"], y[:3])
                out[f"output_{k}_{block}"] = y[3:].copy()
    np.savez_compressed(os.path.join(HERE, "softclip_ref.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
