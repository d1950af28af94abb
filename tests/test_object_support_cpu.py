"""The scaffold of the objects beside the engine (convopeq_amd/csrc/object_support.hpp) on the paths no test on hardware
reaches: a small host program includes the header alone, links the HIP runtime only and defines cpqi::fail itself.  Without a
device every runtime call fails, which is what the first half wants: one fail into the sink or the global (cut at 511), the HIP
macro's code and text, an event owner that holds nothing after a failed create, a row stage that is empty after an impossible
request, and std::exception as CPQ_ERR_OOM.  Where a device is visible the program also grows a stage, sends a strided block up
and back to the bit with sentinels in every padding, and reads an elapsed time; elsewhere those parts are printed as skipped."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_scaffold_reports_once_and_leaves_nothing_behind(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "object_support_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "convopeq_amd", "csrc"),
                    os.path.join(HERE, "sanitize", "object_support_check.cpp"),
                    "-L" + os.path.join(rocm, "lib"), "-Wl,-rpath," + os.path.join(rocm, "lib"), "-lamdhip64",
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout)         # which parts ran: "devices visible", "skipped: ..."
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 failed checks" in r.stdout, r.stdout[-2000:]
    assert "FAILED" not in r.stdout
