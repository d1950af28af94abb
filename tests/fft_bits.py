"""What tests/test_gpu_fft_bits.py compares: SHA-256 of the bytes that cpq_diag_partition_fft returns for the inputs of
tests/test_gpu_fft.py, per partition size.  The kernels have no atomics and the library is built with -ffp-contract=off, so
the bytes are a function of the source alone.

Run as a program, on the MI355X and from a build of the commit that the digests are to pin, this module writes
tests/golden/fft_bits.json:  python tests/fft_bits.py <commit hash>.  The file is a record of THAT commit: a change to the
FFT kernels that is meant to keep every rounding is checked against it and never regenerates it."""
import hashlib
import json
import os
import sys

import numpy as np

SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fft_bits.json")


def inputs(P):
    """x [3][T][P] of tests/test_gpu_fft.py: seeded noise, one silent block, one impulse"""
    n_ch, T = 3, 5 if P <= 4096 else 3
    x = np.random.default_rng(1000 + P).standard_normal((n_ch, T, P))
    x[1, 1] = 0.0
    x[2, 0, :] = 0.0
    x[2, 0, 17] = 1.0
    return np.ascontiguousarray(x)


def digests(lib, P):
    """(sha256 of spec [3][T][P][2], sha256 of out [3][T][P]) as cpq_diag_partition_fft fills them"""
    from fft_layout import dp
    x = inputs(P)
    n_ch, T, _ = x.shape
    spec, out = np.full((n_ch, T, P, 2), -7.0), np.full((n_ch, T, P), -7.0)
    rc = lib.cpq_diag_partition_fft(P, n_ch, T, dp(x), dp(spec), dp(out))
    if rc != 0:
        raise RuntimeError(f"cpq_diag_partition_fft(P = {P}) returned {rc}")
    return hashlib.sha256(spec.tobytes()).hexdigest(), hashlib.sha256(out.tobytes()).hexdigest()


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    from convopeq_amd import _capi
    lib = _capi.load()
    rec = {"commit": sys.argv[1], "entry": "cpq_diag_partition_fft", "inputs": "tests/fft_bits.py inputs(P)", "sha256": {}}
    for P in SIZES:
        s, o = digests(lib, P)
        rec["sha256"][str(P)] = {"spec": s, "out": o}
        print(P, s[:16], o[:16])
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
