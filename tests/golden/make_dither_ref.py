"""Records tests/golden/dither_ref.npz from the reference's own noise-shaper headers through dither_probe.cpp.
    python tests/golden/make_dither_ref.py <reference source tree>
The probe binary is built into a temporary directory and is not kept."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N1, N2 = 1000, 1051
SHAPERS, BITS, RATES = (1, 2), (8, 16, 24), (44100.0, 48000.0, 64000.0, 1.0e6)
M64 = (1 << 64) - 1


def splitmix_noise(n, stream, channel, seed=0xC0FFEE):
    """the project's counter noise (oracle/cpq_oracle.c, orc_gen_pcm): 0.25 * uniform(-1, 1)"""
    out = np.empty(n)
    for i in range(n):
        x = ((seed ^ (stream << 40) ^ (channel << 32) ^ i) + 0x9E3779B97F4A7C15) & M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
        x ^= x >> 31
        out[i] = 0.25 * (float(x >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0)
    return out


def make_input():
    n = N1 + N2
    x = np.stack([splitmix_noise(n, 0, 0), splitmix_noise(n, 0, 1)])
    x[:, 200:260] = 0.0                                     # zeros
    x[0, 300:340], x[1, 300:340] = 1.5, -1.5                # clamped
    x[0, 340:360], x[1, 340:360] = -1.5, 1.5
    x[:, 400:440] = 1.0e-9
    x[0, 500], x[1, 505], x[0, 510], x[1, 515] = np.nan, np.inf, -np.inf, np.nan
    x[0, 990:1003] = np.inf                                 # across the two calls
    x[1, 1500], x[1, 1501] = -np.inf, np.nan
    return x


def main(ref):
    x = make_input()
    out = {"input": x, "calls": np.array([N1, N2]), "headroom": np.array(0.8912509381337456)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dither_probe")
        subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-msse4.1", "-mavx2", "-I" + os.path.join(HERE, "juce_shim"),
                        "-I" + os.path.join(ref, "src"), os.path.join(HERE, "dither_probe.cpp"), "-o", exe], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        x.tofile(fin)
        for sh in SHAPERS:
            for bits in BITS:
                for rate in RATES:
                    subprocess.run([exe, str(sh), str(bits), repr(rate), fin, fout, str(N1), str(N2)], check=True)
                    y = np.fromfile(fout).reshape(2, N1 + N2)
                    key = f"{sh}_{bits}_{int(rate)}"
                    bad = ~np.isfinite(y)
                    codes = np.where(bad, 0.0, y) * float(1 << (bits - 1))
                    assert np.array_equal(codes, np.rint(codes)) and np.abs(codes).max() <= (1 << (bits - 1)) + 1, key     # the 4-tap shaper does not clamp its codes
                    out["codes_" + key] = codes.astype(np.int32)
                    out["bad_" + key] = np.packbits(bad, axis=1)
                    out["negzero_" + key] = np.packbits((y == 0.0) & np.signbit(y), axis=1)      # a code of 0 cannot carry the sign
    np.savez_compressed(os.path.join(HERE, "dither_ref.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
