"""CPU tests of the oversampler's host design (no GPU): the half-band stages of CustomInputOversampler::prepareStage, the
round-trip latency and OversamplingPolicy::resolve, through the C ABI, against tests/os_model.py."""
import ctypes as C

import numpy as np
import pytest

import os_model as M

PAIRS = [(s, t) for t in (M.IIR, M.LINEAR_PHASE) for s in range(3)]


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


@pytest.mark.parametrize("stage,os_type", PAIRS)
def test_stage_shape_and_model(amd, stage, os_type):
    info, taps = amd.os_design_stage(stage, os_type)
    m = M.design_stage(stage, os_type)
    n = M.TAPS[os_type][stage]
    assert info["taps"] == n == len(taps)
    ct = (n - 1) // 2
    assert info["center_tap"] == ct and taps[ct] == 0.5 and info["center_coeff"] == 0.5
    assert info["center_parity"] == 1 and info["conv_parity"] == 0
    assert info["conv_count"] == (n + 1) // 2 == {511: 256, 127: 64, 31: 16, 1023: 512, 255: 128, 63: 32}[n]
    for k in ("center_delay_input", "history_up_keep", "history_down_keep", "conv_count", "attenuation_db"):
        assert info[k] == m[k], k
    # half-band zeros: every tap of the centre's parity except the centre
    odd = np.arange(n) % 2 == 1
    odd[ct] = False
    assert np.all(taps[odd] == 0.0)
    assert np.all(taps[~odd] != 0.0)
    assert np.max(np.abs(taps - taps[::-1])) <= 1e-15
    assert abs(taps.sum() - 1.0) <= 1e-14
    assert np.max(np.abs(taps - m["raw"])) <= 1e-15


# where each stage's stopband reaches its attenuation (cycles per sample at the stage's high rate), measured from the
# design rounded up: the long stages sit within 16 % of the Kaiser estimate of the transition band, (A - 7.95) /
# (2.285 (N - 1)) rad/sample about fs/4; the 31- and 63-tap stages need a wider band than that estimate
STOP_EDGE = {(0, M.IIR): 0.2600, (1, M.IIR): 0.2790, (2, M.IIR): 0.4200,
             (0, M.LINEAR_PHASE): 0.2561, (1, M.LINEAR_PHASE): 0.2690, (2, M.LINEAR_PHASE): 0.3430}


@pytest.mark.parametrize("stage,os_type", PAIRS)
def test_stage_stopband(amd, stage, os_type):
    """FFT of the taps: below -attenuation dB beyond the stage's transition band, DC gain 1, and the half-band
    complement H(f) + H(fs/2 - f) = 1 (real, zero-phase about the centre tap)."""
    _, taps = amd.os_design_stage(stage, os_type)
    att = M.ATTEN[os_type][stage]
    n = len(taps)
    nfft = 1 << 17
    H = np.fft.rfft(taps, nfft)
    f = np.arange(len(H)) / nfft
    Hz = (H * np.exp(2j * np.pi * f * ((n - 1) // 2))).real        # zero-phase response
    edge = STOP_EDGE[(stage, os_type)]
    assert 20 * np.log10(np.abs(Hz[f >= edge]).max()) <= -att
    kaiser = 0.25 + (att - 7.95) / (2.285 * (n - 1)) / (2 * np.pi) / 2
    assert kaiser <= edge <= (1.2 * (kaiser - 0.25) + 0.25 if n > 127 else 0.43)
    assert abs(Hz[0] - 1.0) <= 1e-14
    half = nfft // 2
    assert np.max(np.abs(Hz[:half + 1] + Hz[half::-1] - 1.0)) <= 1e-14


def test_latency(amd):
    assert amd.os_latency(8, M.IIR) == 290.25
    assert amd.os_latency(8, M.LINEAR_PHASE) == 582.25
    assert amd.os_latency(1, M.IIR) == 0.0
    for f in (2, 4, 8):
        for t in (M.IIR, M.LINEAR_PHASE):
            assert amd.os_latency(f, t) == M.latency(f, t)
    assert amd.os_latency(2, M.IIR) == 255.0 and amd.os_latency(4, M.LINEAR_PHASE) == 511.0 + 63.5


# OversamplingPolicy.h: allowed factors per input rate, Auto = the largest
POLICY = [(44100.0, 8), (48000.0, 8), (88200.0, 8), (96000.0, 8), (176400.0, 4), (192000.0, 4), (352800.0, 2),
          (384000.0, 2), (705600.0, 1), (768000.0, 1)]


@pytest.mark.parametrize("rate,max_f", POLICY)
def test_resolve_factor(amd, rate, max_f):
    assert amd.os_resolve_factor(rate, 0) == max_f
    for req in (1, 2, 4, 8):
        assert amd.os_resolve_factor(rate, req) == min(req, max_f)
    for odd in (3, 5, 16, -1):                       # not in {0, 1, 2, 4, 8}: Auto
        assert amd.os_resolve_factor(rate, odd) == max_f


def test_resolve_factor_above_768k(amd):
    assert amd.os_resolve_factor(768000.5, 0) == 0
    assert amd.os_resolve_factor(1.0e6, 2) == 0


def test_host_argument_errors(amd):
    from convopeq_amd import _capi
    lib = _capi.load()
    info = _capi.OsStageInfo()
    buf = np.zeros(2048)
    p = buf.ctypes.data_as(_capi.c_double_p)
    assert lib.cpq_os_design_stage(3, 0, C.byref(info), None, 0) == -1
    assert lib.cpq_os_design_stage(-1, 0, C.byref(info), None, 0) == -1
    assert lib.cpq_os_design_stage(0, 2, C.byref(info), None, 0) == -1
    assert lib.cpq_os_design_stage(0, 0, None, p, 510) == -1          # capacity below the tap count
    assert lib.cpq_os_design_stage(0, 1, None, p, 2048) == 1023
    assert lib.cpq_os_latency(3, 0) < 0 and lib.cpq_os_latency(8, 7) < 0
    assert lib.cpq_os_resolve_factor(0.0, 0) < 0 and lib.cpq_os_resolve_factor(-48000.0, 0) < 0
    assert lib.cpq_os_resolve_factor(float("nan"), 0) < 0
    assert lib.cpq_engine_set_oversampling(None, 2, 0) == -1
    assert lib.cpq_os_reset(None) == -1
    assert lib.cpq_os_up(None, p, p, 1) == -1 and lib.cpq_os_down(None, p, p, 1) == -1
    assert lib.cpq_os_read_telemetry(None, 0, None) == -1
    assert lib.cpq_kernel_name(8) == b"k_os_halfband"
    with pytest.raises(amd.CpqError):
        amd.os_design_stage(5)
