"""The layout arithmetic of the packed PCM entry points (convopeq_amd/csrc/pcm_layout.hpp: bytes per sample, pitches, widths,
the chunk copies of a call, byte ranges and the overlap test) is plain 64-bit integer arithmetic, so it is tested here without a
GPU: a small host program includes that header alone -- no HIP, not the library -- and checks, exactly, pitches and widths of
every format x layout, that the chunk copies of a call touch every byte of both buffers once, the overlap test on touching,
nested and equal ranges, and that nothing wraps at 1024 streams x 524288 samples.  Built with the address and
undefined-behaviour sanitizers and run as a program of its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_pcm_layout_arithmetic(tmp_path):
    exe = tmp_path / "pcm_layout_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "convopeq_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "sanitize", "pcm_layout_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 failed checks" in r.stdout, r.stdout[-2000:]
    assert "FAILED" not in r.stdout
