"""cpq_ir_resample_host (the device path's summation order on the host, no GPU) against the analytic signals and r8brain's recorded
outputs of tests/golden/resample_ref.npz, against the longdouble model of tests/resample_model.py, and the call's other behaviour.

The call cuts every channel's tail as the reference does (-160 dB of the peak, 8 samples in a row): the fixture's Gaussian falls
below that well before its end, so the host path is compared on what it keeps and the model, which has no trim and the same table,
on every output."""
import numpy as np
import pytest

import convopeq_amd as amd
from convopeq_amd import _capi as K
import resample_model as M


@pytest.fixture(scope="module")
def golden():
    return np.load(M.GOLDEN)


def reference_trim(y):
    """resampleIR's effectiveLen (ResampleAndFallback.cpp:66-87)"""
    peak = np.max(np.abs(y))
    if peak < 1e-12:
        return 1
    thr = peak * 10.0 ** (-160.0 / 20.0)
    run = 0
    for i in range(len(y) - 1, -1, -1):
        if abs(y[i]) > thr:
            run += 1
            if run >= 8:
                return i + 8
        else:
            run = 0
    return 1


@pytest.mark.parametrize("pair", M.PAIRS, ids=lambda p: M.pair_key(*p))
def test_accuracy_against_the_analytic_signal(golden, pair):
    a, b = pair
    key = M.pair_key(a, b)
    x, d_ref = golden["x_" + key], float(golden["d_ref_" + key])
    n_out = M.out_len(len(x), a, b)
    want = M.passband_signal(n_out, b)
    allowed = max(2.0 * d_ref, 64 * 2.0 ** -52 * np.max(np.abs(want)))
    design = amd.resample_design(a, b)
    model, bound = M.resample_rows(design, x)
    got = amd.ir_resample(x, a, b, host=True)
    assert got.shape[0] == 1 and got.shape[1] <= n_out
    kept = got.shape[1]
    err_model, err_host = float(np.max(np.abs(model - want))), float(np.max(np.abs(got[0] - want[:kept])))
    print(f"{key}: model {err_model:.3e}, host path {err_host:.3e} on {kept} of {n_out}, 2 d_ref {2 * d_ref:.3e}")
    assert len(model) == n_out and err_model <= allowed
    assert err_host <= allowed
    # pre-trim length within 1 of r8brain's, and the kept length is the reference's rule on the untrimmed row
    assert abs(n_out - int(golden["max_out_" + key])) <= 1
    assert kept == reference_trim(model.astype(np.float64))
    # the host path against the model, output by output: T roundings of an fma chain, gamma_T sum |h x| (Higham, Accuracy and
    # Stability of Numerical Algorithms, 3.1), plus the model's own longdouble sum and its rounding to double
    T = design["T"]
    u = 2.0 ** -53
    limit = (T * u / (1 - T * u)) * bound[:kept] + T * 2.0 ** -63 * bound[:kept]
    assert np.all(np.abs(got[0].astype(np.longdouble) - model[:kept]) <= limit)


def test_stop_band_leak(golden):
    a, b = M.STOP_PAIR
    x = golden["x_stop"]
    model, _ = M.resample_rows(amd.resample_design(a, b), x)
    leak_model = float(np.max(np.abs(model)))
    got = amd.ir_resample(x, a, b, host=True)
    leak = float(np.max(np.abs(got)))
    print(f"stop band: leak {leak:.3e} (model, untrimmed {leak_model:.3e}), r8brain {float(golden['leak_stop']):.3e}")
    assert leak <= 2.0 * float(golden["leak_stop"]) and leak_model <= 2.0 * float(golden["leak_stop"])


def test_impulse_peak_and_length(golden):
    a, b = M.IMPULSE_PAIR
    x = golden["x_impulse"]
    got = amd.ir_resample(x, a, b, host=True)[0]
    assert int(np.argmax(np.abs(got))) == 109 == int(np.argmax(np.abs(golden["y_impulse"])))
    assert abs(M.out_len(len(x), a, b) - int(golden["max_out_impulse"])) <= 1
    # the impulse reads the filter itself: taps of phase (j M) mod L at k = floor(j M / L) + T / 2 - 100
    d = amd.resample_design(a, b)
    for j in (0, 50, 109, 200):
        k = (j * d["M"]) // d["L"] + d["T"] // 2 - M.IMPULSE_AT
        assert got[j] == d["taps"][(j * d["M"]) % d["L"]][k]


def test_tail_trim_and_per_channel_zeroing():
    rng = np.random.default_rng(5)
    ir = np.zeros((2, 3000))
    ir[0, :2000] = rng.standard_normal(2000) * np.exp(-np.arange(2000) / 300.0)
    ir[1, :600] = rng.standard_normal(600) * np.exp(-np.arange(600) / 100.0)
    got = amd.ir_resample(ir, 44100, 48000, host=True)
    d = amd.resample_design(44100, 48000)
    rows = [M.resample_rows(d, ir[ch])[0].astype(np.float64) for ch in range(2)]
    lengths = [reference_trim(r) for r in rows]
    assert lengths[1] < lengths[0] < M.out_len(3000, 44100, 48000)
    assert got.shape == (2, max(lengths))
    for ch in range(2):
        assert np.allclose(got[ch, :lengths[ch]], rows[ch][:lengths[ch]], rtol=0, atol=1e-13)
        assert not np.any(got[ch, lengths[ch]:])
    alone = amd.ir_resample(ir[1], 44100, 48000, host=True)
    assert alone.shape == (1, lengths[1]) and np.array_equal(alone[0], got[1, :lengths[1]])


def test_refusals():
    x = np.ones((1, 64))
    cases = [(np.zeros((1, 0)), 44100, 48000, 0, K.CPQ_ERR_INVALID_ARG),           # no samples
             (np.zeros((0, 8)), 44100, 48000, 0, K.CPQ_ERR_INVALID_ARG),           # no channels
             (np.zeros((2, 64)), 44100, 48000, 0, K.CPQ_ERR_SILENT_IR),
             (np.full((1, 64), 9e-13), 44100, 48000, 0, K.CPQ_ERR_SILENT_IR),
             (x, 44100, 48000, K.CPQ_RESAMPLE_MINIMUM_PHASE, K.CPQ_ERR_UNSUPPORTED),
             (x, 44100, 48000, 7, K.CPQ_ERR_INVALID_ARG),
             (x, 44100.5, 48000, 0, K.CPQ_ERR_UNSUPPORTED),
             (x, 44100, 44101, 0, K.CPQ_ERR_UNSUPPORTED),
             (x, 0.0, 48000, 0, K.CPQ_ERR_INVALID_ARG),
             (x, 44100, float("nan"), 0, K.CPQ_ERR_INVALID_ARG)]
    for ir, a, b, phase, status in cases:
        with pytest.raises(amd.CpqError) as e:
            amd.ir_resample(ir, a, b, phase=phase, host=True)
        assert e.value.status == status, (a, b, phase)
    lib = K.load()
    assert lib.cpq_status_string(K.CPQ_ERR_SILENT_IR) == b"silent impulse response"
    assert lib.cpq_ir_resample_host(None, 48000.0, 0, K.IrBuffer()) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_ir_resample_host(K.IrBuffer(), 48000.0, 0, None) == K.CPQ_ERR_INVALID_ARG
    out = K.IrBuffer(3, 4, 5.0, None)                   # a refusal leaves the output zeroed
    assert lib.cpq_ir_resample_host(None, 48000.0, 0, out) == K.CPQ_ERR_INVALID_ARG
    assert (out.n_channels, out.n_samples, out.sample_rate, bool(out.data)) == (0, 0, 0.0, False)


def test_equal_rates_return_a_copy():
    rng = np.random.default_rng(6)
    ir = rng.standard_normal((2, 777))
    for target in (48000.0, 48000.0 + 5e-7):
        got = amd.ir_resample(ir, 48000.0, target, host=True)
        assert np.array_equal(got, ir)
    silent = np.zeros((1, 10))                          # the copy comes before the silence check, as in the reference
    assert np.array_equal(amd.ir_resample(silent, 48000.0, 48000.0, host=True), silent)
    assert np.array_equal(amd.ir_resample(ir, 12345.5, 12345.5, host=True), ir)       # and before the filter design


def test_result_passes_through_ir_prepare():
    ir, rate = amd.ir_load_wav(M.GOLDEN.replace("resample_ref.npz", "impulse_room_correction_hpf_lpf.wav"))
    assert rate == 48000.0
    head = ir[:, :4096]
    with pytest.raises(amd.CpqError) as e:              # still refused: the loader stage is a call of its own
        amd.ir_prepare(head, 48000.0, 44100.0, 0.5)
    assert e.value.status == K.CPQ_ERR_UNSUPPORTED
    got = amd.ir_resample(head, 48000.0, 44100.0, host=True)
    assert got.shape[0] == ir.shape[0] and got.shape[1] <= M.out_len(4096, 48000, 44100)
    prep = amd.ir_prepare(got, 44100.0, 44100.0, 0.5)
    assert prep["ir"].shape == (ir.shape[0], 22050) and prep["sample_rate"] == 44100.0 and np.any(prep["ir"])


def test_design_and_host_path_under_sanitizers(tmp_path):
    """tests/sanitize/resample_design_check.cpp: the design and the host path as a program of their own under ASan and UBSan"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "convopeq_amd", "csrc")
    exe = tmp_path / "resample_design_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + csrc, "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "sanitize", "resample_design_check.cpp"), os.path.join(csrc, "resample_design.cpp"),
                    os.path.join(csrc, "ir_ingest.cpp"), "-o", str(exe), "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failed checks" in r.stdout and "FAILED" not in r.stdout
