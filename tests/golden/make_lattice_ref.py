"""Records tests/golden/lattice_ref.npz from the reference's own LatticeNoiseShaper.h through lattice_probe.cpp.
    python tests/golden/make_lattice_ref.py <reference source tree>
The probe binary is built into a temporary directory and is not kept.  The input rows and the two call lengths are those of
make_dither_ref.py.  Per case the file holds the codes, the mask of non-finite outputs and the mask of negative zeros."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_dither_ref import N1, N2, make_input  # noqa: E402

BITS = (8, 16, 24)
DEFAULT = [-0.003796, -0.006752, 0.008418, -0.010546, 0.004716, -0.007624, -0.020750, -0.002049, -0.003632]
# (b): nine values within +-0.3 from numpy's default_rng(9), kept as literals so that the fixture does not hang on a generator
RANDOM = [0.2220616868, -0.2014177601, 0.1318403887, -0.0561205147, 0.0247398019, 0.2788726754, -0.1462038231, 0.0935117622, -0.2652193170]
STRONG = [0.82, -0.68, 0.55, -0.43, 0.33, -0.25, 0.18, -0.12, 0.07]      # states onto the +-2 clamp, outputs onto the rails
ODD = [1.5, -3.0, float("nan"), float("inf"), 0.25, -0.125]              # clampCoeff and the zero fill: n = 6
# case -> (set of call 1, set applied with applyMatchedCoefficients before call 2 or None)
CASES = {"a": (DEFAULT, None), "b": (RANDOM, None), "c": (STRONG, None), "d": (ODD, None), "e": (DEFAULT, RANDOM)}


def words(v):
    return [str(len(v))] + [repr(float(c)) for c in v]


def main(ref):
    x = make_input()
    out = {"input": x, "calls": np.array([N1, N2]), "headroom": np.array(0.8912509381337456)}
    for name, (first, second) in CASES.items():
        out["set1_" + name] = np.array(first)
        out["set2_" + name] = np.array(second if second is not None else [])
        out["swap_" + name] = np.array(second is not None)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "lattice_probe")
        subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-msse4.1", "-mavx2", "-mfma", "-I" + os.path.join(HERE, "juce_shim"),
                        "-I" + os.path.join(ref, "src"), os.path.join(HERE, "lattice_probe.cpp"), "-o", exe], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        x.tofile(fin)
        for name, (first, second) in CASES.items():
            for bits in BITS:
                subprocess.run([exe, str(bits), fin, fout, str(N1), str(N2)] + words(first) + (words(second) if second is not None else []), check=True)
                y = np.fromfile(fout).reshape(2, N1 + N2)
                key = f"{name}_{bits}"
                bad = ~np.isfinite(y)
                assert np.array_equal(bad, np.isnan(y)), key                        # the code clamp leaves no infinity
                codes = np.where(bad, 0.0, y) * float(1 << (bits - 1))
                assert np.array_equal(codes, np.rint(codes)) and codes.min() >= -(1 << (bits - 1)) and codes.max() <= (1 << (bits - 1)) - 1, key
                out["codes_" + key] = codes.astype(np.int32)
                out["bad_" + key] = np.packbits(bad, axis=1)
                out["negzero_" + key] = np.packbits((y == 0.0) & np.signbit(y), axis=1)      # a code of 0 cannot carry the sign
    np.savez_compressed(os.path.join(HERE, "lattice_ref.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
