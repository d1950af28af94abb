"""minphase_plan.hpp -- the HIP-free plan of cpq_ir_minimum_phase_batch (FFT size, factorisation, groups, chunks under the
workspace cap, launch list, twiddle tables) -- and the three steps cpq_ir_prepare is split into (ir_ingest.hpp), as a program of
their own under the address and undefined-behaviour sanitizers: tests/sanitize/minphase_plan_check.cpp."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_plan_and_prepare_steps_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "convopeq_amd", "csrc")
    exe = tmp_path / "minphase_plan_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "sanitize", "minphase_plan_check.cpp"), os.path.join(csrc, "ir_ingest.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failed checks" in r.stdout and "FAILED" not in r.stdout
