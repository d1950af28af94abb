"""The plan of a plan group's call (convopeq_amd/csrc/nuc_replay.hpp: the reference's Add / Get bookkeeping per layer replayed
over the chunks of a call, the chunk table that goes to the device, and the decisions that pick the launch sequence) is integer
arithmetic, so it is tested here without a GPU: a small host program includes that header alone -- no HIP, not the library --
and checks, with exact integer equality, that a stretch of input gives the same per-chunk entries and leaves the same layer
state however it is cut into calls, the reference's invariants per chunk, every decision on the smallest input that flips it,
and that the table never outgrows its bound.  Built with the address and undefined-behaviour sanitizers and run as a program
of its own."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_nuc_replay_split_invariance_invariants_decisions_and_capacity(tmp_path):
    exe = tmp_path / "nuc_replay_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "convopeq_amd", "csrc"),
                    os.path.join(HERE, "sanitize", "nuc_replay_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 failed checks" in r.stdout, r.stdout[-2000:]
    assert "FAILED" not in r.stdout
