"""quant_host.hpp -- the definition of cpq_quantizer, its byte layout, its refusals, the host object and the slot arithmetic of the
device kernel's store pass -- as a program of its own under the address and undefined-behaviour sanitizers:
tests/sanitize/quant_host_check.cpp runs cpq::QuantHost on exactly sized heap blocks (odd S24 byte phases, pitch gaps, n = 1),
holds it to the definition sample by sample and to every split into calls, and restates k_quantize's image and store pass as host
loops that must give the same bytes."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_host_object_and_store_pass_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "convopeq_amd", "csrc")
    exe = tmp_path / "quant_host_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "sanitize", "quant_host_check.cpp"), os.path.join(csrc, "dither_design.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failed checks" in r.stdout and "FAILED" not in r.stdout
