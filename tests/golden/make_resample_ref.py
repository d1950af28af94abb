"""Records tests/golden/resample_ref.npz from the reference's sample-rate converter (r8brain's CDSPResampler, configured as
ConvolverProcessorInternal::resampleIR configures it) through resample_probe.cpp.
    python tests/golden/make_resample_ref.py <reference source tree>
The probe binary is built into a temporary directory and is not kept.  The inputs are the closed forms of tests/resample_model.py:
0.04 s of a Gaussian envelope on five pass-band tones (band-limited analytically; the edges are about 1e-22), so the analytic
signal sampled at the output rate is what an ideal converter returns, and d_ref = max |r8brain - analytic| is the reference's own
error: the yardstick of the tests.  Two more cases: the envelope on a 30 kHz carrier, 96000 -> 48000 (everything r8brain lets
through is leak), and a unit impulse."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample_model as M  # noqa: E402


def run_probe(exe, tmp, x, in_rate, out_rate):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    np.ascontiguousarray(x, dtype=np.float64).tofile(fin)
    subprocess.run([exe, str(in_rate), str(out_rate), fin, fout], check=True, capture_output=True, text=True)
    o = np.fromfile(fout)
    max_out = int(o[0])
    assert len(o) == max_out + 1
    return o[1:], max_out


def main(ref):
    out = {"pairs": np.array(M.PAIRS), "tones": np.array(M.TONES)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "resample_probe")
        subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ref, "r8brain-free-src"), os.path.join(HERE, "resample_probe.cpp"),
                        "-o", exe, "-lpthread"], check=True)
        for in_rate, out_rate in M.PAIRS:
            key = M.pair_key(in_rate, out_rate)
            n = M.input_len(in_rate)
            x = M.passband_signal(n, in_rate)
            y, max_out = run_probe(exe, tmp, x, in_rate, out_rate)
            n_out = M.out_len(n, in_rate, out_rate)
            want = M.passband_signal(n_out, out_rate)
            d_ref = float(np.max(np.abs(y[:n_out] - want)))
            print(f"{key}: n {n} -> {n_out} (getMaxOutLen {max_out}), peak {np.max(np.abs(x)):.4f}, d_ref {d_ref:.3e}")
            out["x_" + key], out["y_" + key] = x, y
            out["max_out_" + key], out["d_ref_" + key] = np.array(max_out), np.array(d_ref)
        in_rate, out_rate = M.STOP_PAIR
        x = M.stopband_signal(M.input_len(in_rate), in_rate)
        y, max_out = run_probe(exe, tmp, x, in_rate, out_rate)
        leak = float(np.max(np.abs(y[:M.out_len(len(x), in_rate, out_rate)])))
        print(f"stop band: peak {np.max(np.abs(x)):.4f}, leak {leak:.3e}")
        out["x_stop"], out["y_stop"], out["leak_stop"] = x, y, np.array(leak)
        in_rate, out_rate = M.IMPULSE_PAIR
        x = np.zeros(M.IMPULSE_LEN)
        x[M.IMPULSE_AT] = 1.0
        y, max_out = run_probe(exe, tmp, x, in_rate, out_rate)
        print(f"impulse: peak at output {int(np.argmax(np.abs(y)))}")
        out["x_impulse"], out["y_impulse"], out["max_out_impulse"] = x, y, np.array(max_out)
    path = os.path.join(HERE, "resample_ref.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
