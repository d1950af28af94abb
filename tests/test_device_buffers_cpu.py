"""The owners of the engine's device memory (convopeq_amd/csrc/device_buffers.hpp) on their failure paths, which no test
on hardware can reach without exhausting a shared machine's memory: a small host program includes the header, links the
HIP runtime only, and asks for a group whose second member is an impossible size (2^60 bytes).  Without a device every
request fails and the runtime leaves the caller's pointer as it was, so the same path is taken there.  "No HIP error
left pending" is hipGetLastError() == hipSuccess where a device is visible; without one every runtime call, that one
included, returns hipErrorNoDevice whatever came before, and the driver checks for exactly that.  The parts that need
allocations to succeed run where a device is visible and are printed as skipped elsewhere."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_buffer_groups_are_all_or_nothing_and_leave_no_error_pending(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "device_buffers_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "convopeq_amd", "csrc"),
                    os.path.join(HERE, "sanitize", "device_buffers_check.cpp"),
                    "-L" + os.path.join(rocm, "lib"), "-Wl,-rpath," + os.path.join(rocm, "lib"), "-lamdhip64",
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout)         # which parts ran: "devices visible", "skipped: ..."
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 failed checks" in r.stdout, r.stdout[-2000:]
    assert "FAILED" not in r.stdout
