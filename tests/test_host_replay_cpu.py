"""The ramps and fades the engine replays on the host before it launches anything (convopeq_amd/csrc/host_replay.hpp: the
reference's LinearRamp, the total-gain ramp, the EQ bypass fade, the mix smoother, the latency cross-fade) are plain integer
and double arithmetic, so they are tested here without a GPU: a small host program includes that header alone -- no HIP, not
the library -- and checks, exactly (== on doubles), the ramp's semantics, that N callbacks give the same outputs and leave the
same state however they are cut into calls, and that what the engine predicts on a copy of a ramp (which convolver rests in a
call) is what the replay then decides, with the original untouched.  The EQ's plan of a call
(gain segments, bypass classes, band resets, pieces) is the same header's and is checked the same way, for several streams
at once.  The processor-level stage's plan of a call (who rests, mix prefixes and gain pairs, latency ranges) and its arithmetic
are driven through the planners engine_proc.cpp itself calls.  Built with the address and
undefined-behaviour sanitizers and run as a program of its own."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_replay_semantics_split_invariance_and_predictions(tmp_path):
    exe = tmp_path / "host_replay_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "convopeq_amd", "csrc"),
                    os.path.join(HERE, "sanitize", "host_replay_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 failed checks" in r.stdout, r.stdout[-2000:]
    assert "FAILED" not in r.stdout
