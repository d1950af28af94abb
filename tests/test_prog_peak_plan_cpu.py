"""The true-peak and gain part of csrc/prog_plan.hpp without a GPU: k_prog_peak and k_prog_apply restated as host loops under
sanitizers (tests/sanitize/prog_peak_check.cpp), held bit for bit against the numpy model's recorded values
(tests/golden/prog_peak_cases.txt, written by record_cases() below), and cpq_loudness_peaks_host against the model."""
import os
import subprocess

import numpy as np

import prog_peak_model as PK

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "golden", "prog_peak_cases.txt")
LENGTHS = (1, 10, 11, 12, 4095, 4096, 4097, 8193)
RATES = (8000, 96000, 192000)                      # four phases, two, none
ROWS = 2


def case_rows(rows, n, seed):
    """the generator of prog_peak_check.cpp's caseRows: a 64-bit congruential generator, 24 bits a sample in [-0.5, 0.5), with
    values the scrub takes out planted"""
    x = np.empty(rows * n)
    s = seed
    for i in range(rows * n):
        s = (s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        v = ((s >> 40) - 8388608) / 16777216.0
        if i % 97 == 5:
            v = np.nan
        if i % 101 == 7:
            v = 1.0e300
        if i % 103 == 3:
            v = -np.inf
        x[i] = v
    return x.reshape(rows, n)


def cases():
    for rate in RATES:
        for n in LENGTHS:
            yield f"r{rate}_n{n}", rate, ROWS, n, 1000 * (rate // 1000) + n


def record_cases(path=CASES):
    with open(path, "w") as f:
        for name, rate, rows, n, seed in cases():
            tp, sp = PK.peaks(case_rows(rows, n, seed), rate)
            f.write(f"case {name} {rate} {rows} {n} {seed}\n")
            f.write("want " + " ".join(f"{float(tp[r]).hex()} {float(sp[r]).hex()}" for r in range(rows)) + "\n")


def read_cases(path=CASES):
    lines = open(path).read().split("\n")
    for i in range(0, len(lines) - 1, 2):
        _, name, rate, rows, n, seed = lines[i].split()
        want = lines[i + 1].split()
        assert want[0] == "want" and len(want) == 1 + 2 * int(rows)
        yield name, int(rate), int(rows), int(n), int(seed), np.array([float.fromhex(t) for t in want[1:]]).reshape(int(rows), 2)


def test_the_record_is_the_models():
    """the numpy model on the generated rows gives the recorded values to the bit: the file cannot drift from the model"""
    got = list(read_cases())
    assert [g[:5] for g in got] == list(cases())
    for name, rate, rows, n, seed, want in got:
        tp, sp = PK.peaks(case_rows(rows, n, seed), rate)
        assert np.array_equal(tp.view(np.uint64), want[:, 0].copy().view(np.uint64)), name
        assert np.array_equal(sp.view(np.uint64), want[:, 1].copy().view(np.uint64)), name
        assert np.all(sp > 0.0) and (np.array_equal(tp, sp) if rate >= 176400 else not np.array_equal(tp, sp)), name


def test_kernels_as_host_loops_under_sanitizers(tmp_path):
    """calls of 1, 10, 11, 12, 4095, 4096, 4097 and 8193 samples, equal and random splits, the three phase sets, k_prog_apply's
    wide and scalar paths with odd n and odd strides, in place and not: on exactly sized heap blocks"""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "convopeq_amd", "csrc")
    exe = tmp_path / "prog_peak_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + csrc, "-I" + os.path.join(root, "include"),
                    os.path.join(HERE, "sanitize", "prog_peak_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), CASES], capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failed checks" in r.stdout and "FAILED" not in r.stdout


def test_peaks_host_is_the_model_bit_for_bit():
    import convopeq_amd as amd
    rng = np.random.default_rng(11)
    x = 0.4 * rng.standard_normal((5, 9001))
    x[1, 17] = np.nan
    x[2, :] = 0.0
    x[3, 4500] = -3.0
    x[4] *= 1e-310                                  # denormals
    for rate in (8000, 48000, 96000, 192000):
        tp, sp = amd.loudness_peaks_host(x, rate)
        want_tp, want_sp = PK.peaks(x, rate)
        assert np.array_equal(tp.view(np.uint64), want_tp.view(np.uint64)), rate
        assert np.array_equal(sp.view(np.uint64), want_sp.view(np.uint64)), rate
    assert tp[2] == 0.0 and sp[3] == 3.0 and sp[4] > 0.0
    for name, rate, rows, n, seed, want in read_cases():
        tp, sp = amd.loudness_peaks_host(case_rows(rows, n, seed), rate)
        assert np.array_equal(tp.view(np.uint64), want[:, 0].copy().view(np.uint64)), name
        assert np.array_equal(sp.view(np.uint64), want[:, 1].copy().view(np.uint64)), name
