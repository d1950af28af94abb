"""csrc/prog_plan.hpp without a GPU: the plan of a call and both kernels of prog_kernels.hip restated as host loops, under
sanitizers (tests/sanitize/prog_plan_check.cpp), with the host finish held against the numpy model's recorded values
(tests/golden/prog_finish_cases.txt, written by record_cases() below from tests/prog_inputs.py's programmes) and, to the bit,
against its values on the planted ties and padded programmes of tests/prog_finish_inputs.py (prog_finish_edge_cases.txt)."""
import os
import subprocess

import numpy as np

import prog_inputs as I
import prog_model as P

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "golden", "prog_finish_cases.txt")
EDGE_CASES = os.path.join(HERE, "golden", "prog_finish_edge_cases.txt")
Z_KEYS = ("z_gate", "z_int", "z_mom_max", "z_short_max", "z_lo", "z_hi")
N_KEYS = ("n_blocks", "n_abs", "n_rel", "n_short_kept")


def record_cases(path=CASES):
    """one case per programme: the fp64 model's hop sums and the numpy finish's counts and mean squares on them"""
    with open(path, "w") as f:
        for name, v in I.reference().items():
            r = P.finish(v["E"], I.H)
            f.write(f"case {name} {I.H} {len(v['E'])}\n")
            f.write(" ".join(float(e).hex() for e in v["E"]) + "\n")
            f.write("want " + " ".join(str(r[k]) for k in N_KEYS) + " " + " ".join(float(r[k]).hex() for k in Z_KEYS) + "\n")


def read_cases(path=CASES):
    lines = open(path).read().split("\n")
    for i in range(0, len(lines) - 2, 3):
        _, name, hop, n = lines[i].split()
        E = np.array([float.fromhex(t) for t in lines[i + 1].split()])
        want = lines[i + 2].split()
        assert len(E) == int(n) and want[0] == "want"
        yield name, int(hop), E, [int(t) for t in want[1:5]], [float.fromhex(t) for t in want[5:]]


def test_the_record_is_the_models():
    """the numpy finish on the recorded hop sums gives the recorded values: the file cannot drift from tests/prog_model.py"""
    names = []
    for name, hop, E, counts, zs in read_cases():
        r = P.finish(E, hop)
        assert [r[k] for k in N_KEYS] == counts, name
        assert np.allclose([float(r[k]) for k in Z_KEYS], zs, rtol=2.0 ** -50, atol=0.0), name
        names.append(name)
    assert names == list(I.inputs())


def test_plan_and_kernels_as_host_loops_under_sanitizers(tmp_path):
    """calls of 1, H - 1, H, H + 1, 2048 and 2049 samples at 8000, 44100 and 48000 Hz, random splits, a hop that straddles three
    calls, the max_hops refusal, and k_prog_finish's lanes, tree and bitonic network on exactly sized heap blocks"""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "convopeq_amd", "csrc")
    exe = tmp_path / "prog_plan_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + csrc, "-I" + os.path.join(root, "include"),
                    os.path.join(HERE, "sanitize", "prog_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), CASES, EDGE_CASES], capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failed checks" in r.stdout and "FAILED" not in r.stdout
    assert "recorded cases in " + CASES in r.stdout and "recorded cases in " + EDGE_CASES in r.stdout
