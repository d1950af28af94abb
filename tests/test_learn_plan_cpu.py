"""csrc/learn_plan.hpp without a GPU: both kernels of learn_kernels.hip restated as host loops over workgroups, phases and lanes,
under sanitizers (tests/sanitize/learn_plan_check.cpp), on exactly sized heap blocks."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_kernels_as_host_loops_under_sanitizers(tmp_path):
    """1, 63, 64, 65 and 129 learners over three generations, some inactive, with ties, NaN and DBL_MAX fitness, fewer than six
    finite values, covariances on the Cholesky floors and candidates on the safety margin: the lane-dealt ask and tell equal the
    header's learnAsk and learnTell bit for bit; a dead generator ends"""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "convopeq_amd", "csrc")
    exe = tmp_path / "learn_plan_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + csrc, "-I" + os.path.join(root, "include"),
                    os.path.join(HERE, "sanitize", "learn_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failed checks" in r.stdout and "FAILED" not in r.stdout
