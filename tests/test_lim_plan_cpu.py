"""lim_plan.hpp -- the definition of cpq_limiter, the plan of a call and the launch of its two kernels -- as a program of its own
under the address and undefined-behaviour sanitizers: tests/sanitize/lim_plan_check.cpp restates k_lim_apply and k_lim_keep as host
loops on exactly sized heap blocks and holds them to cpq::LimHost bit for bit, at windows 8, 9, 72, 1023 and 1024, on the calls of
tests/test_gpu_limiter_windows.py's sweep at 14 of its windows, and on its rows of 256 and 257 tiles with the partials at the
stride the object keeps."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_kernels_as_host_loops_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "convopeq_amd", "csrc")
    exe = tmp_path / "lim_plan_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "sanitize", "lim_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failed checks" in r.stdout and "FAILED" not in r.stdout
