"""The refusals of cpq_loudness's true peak and normalisation that need no device, and what the host-only cpq_loudness_gain_limited
computes."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import convopeq_amd as amd
from convopeq_amd import _capi as K

HERE = os.path.dirname(os.path.abspath(__file__))


def _result(integrated):
    return K.LoudnessResult(integrated=integrated, n_rel=1 if math.isfinite(integrated) else 0)


def _peaks(tl=0.0, tr=0.0, sl=0.0, sr=0.0):
    return K.LoudnessPeaks((C.c_double * 2)(tl, tr), (C.c_double * 2)(sl, sr))


def _limited(integrated, pk, target=-23.0, ceiling=-1.0):
    g, lim = C.c_double(-1.0), C.c_int32(-1)
    rc = K.load().cpq_loudness_gain_limited(C.byref(_result(integrated)), C.byref(pk), target, ceiling, C.byref(g), C.byref(lim))
    return rc, g.value, lim.value


def test_the_header_announces_the_feature():
    header = open(os.path.join(os.path.dirname(HERE), "include", "convopeq_mi355x.h")).read()
    assert "#define CPQ_HAS_PROGRAMME_TRUE_PEAK 1" in header
    assert C.sizeof(K.LoudnessPeaks) == 32
    assert C.sizeof(K.LoudnessDesc) == 32           # the switch is a setter: the desc and its "flags must be 0" are as they were


def test_null_handles():
    lib = K.load()
    x = np.zeros((2, 16))
    g = np.ones(1)
    pk = _peaks()
    assert lib.cpq_loudness_set_true_peak(None, 1) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_read_peaks(None, C.byref(pk)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_apply_device(None, g.ctypes.data_as(K.c_double_p), x.ctypes.data, 16, x.ctypes.data, 16, 16) == K.CPQ_ERR_INVALID_ARG


def test_gain_limited_either_limit_wins():
    # -20 LUFS to -23: the loudness gain is -3 dB, and 0.5 -3 dB stays below -1 dBTP
    rc, g, lim = _limited(-20.0, _peaks(0.5, 0.4, 0.45, 0.3))
    assert rc == K.CPQ_OK and lim == 0 and g == 10.0 ** (-3.0 / 20.0)
    plain = C.c_double()
    assert K.load().cpq_loudness_gain(C.byref(_result(-20.0)), -23.0, C.byref(plain)) == K.CPQ_OK and plain.value == g
    # -35 LUFS to -23 is +12 dB; a peak of 0.5 may rise by 10^(-1 / 20) / 0.5 only
    rc, g, lim = _limited(-35.0, _peaks(0.5, 0.4, 0.45, 0.3))
    assert rc == K.CPQ_OK and lim == 1 and g == 10.0 ** (-1.0 / 20.0) / 0.5
    # the largest of the four decides, the sample peaks included
    for pk in (_peaks(0.1, 0.5, 0.1, 0.1), _peaks(0.1, 0.1, 0.5, 0.1), _peaks(0.1, 0.1, 0.1, 0.5)):
        assert _limited(-35.0, pk) == (K.CPQ_OK, 10.0 ** (-1.0 / 20.0) / 0.5, 1)
    # the two gains equal: the loudness gain is reported
    rc, g, lim = _limited(-23.0, _peaks(10.0 ** (-1.0 / 20.0)), ceiling=-1.0)
    assert rc == K.CPQ_OK and g == 1.0 and lim == 0


def test_gain_limited_silence_and_no_peak():
    # a silent programme: nothing passed the gates, no gain, the outputs are left alone
    assert _limited(-math.inf, _peaks()) == (K.CPQ_ERR_NOT_READY, -1.0, -1)
    assert K.load().cpq_loudness_last_error(None)
    # peak == 0 sets no limit
    rc, g, lim = _limited(-35.0, _peaks())
    assert rc == K.CPQ_OK and lim == 0 and g == 10.0 ** (12.0 / 20.0)


def test_gain_limited_refusals():
    lib = K.load()
    ok = _peaks(0.5, 0.5, 0.5, 0.5)
    for target, ceiling in ((math.nan, -1.0), (math.inf, -1.0), (-23.0, math.nan), (-23.0, -math.inf)):
        assert _limited(-20.0, ok, target, ceiling) == (K.CPQ_ERR_INVALID_ARG, -1.0, -1)
    for pk in (_peaks(math.nan), _peaks(0.1, math.inf), _peaks(0.1, 0.1, -0.5), _peaks(0.1, 0.1, 0.1, math.nan)):
        assert _limited(-20.0, pk) == (K.CPQ_ERR_INVALID_ARG, -1.0, -1)
    assert _limited(math.nan, ok)[0] == K.CPQ_ERR_NOT_READY
    g, lim, r = C.c_double(), C.c_int32(), _result(-20.0)
    assert lib.cpq_loudness_gain_limited(None, C.byref(ok), -23.0, -1.0, C.byref(g), C.byref(lim)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_gain_limited(C.byref(r), None, -23.0, -1.0, C.byref(g), C.byref(lim)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_gain_limited(C.byref(r), C.byref(ok), -23.0, -1.0, None, C.byref(lim)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_gain_limited(C.byref(r), C.byref(ok), -23.0, -1.0, C.byref(g), None) == K.CPQ_ERR_INVALID_ARG


def test_peaks_host_refusals():
    lib = K.load()
    x = np.zeros((2, 16))
    tp, sp = np.zeros(2), np.zeros(2)
    p = lambda a: a.ctypes.data_as(K.c_double_p)
    assert lib.cpq_loudness_peaks_host(p(x), 16, 2, 16, 48000.0, p(tp), p(sp)) == K.CPQ_OK
    for args in ((None, 16, 2, 16, 48000.0, p(tp), p(sp)), (p(x), 16, 2, 16, 48000.0, None, p(sp)), (p(x), 16, 2, 16, 48000.0, p(tp), None),
                 (p(x), 16, 0, 16, 48000.0, p(tp), p(sp)), (p(x), 15, 2, 16, 48000.0, p(tp), p(sp)), (p(x), 16, 2, -1, 48000.0, p(tp), p(sp))):
        assert lib.cpq_loudness_peaks_host(*args) == K.CPQ_ERR_INVALID_ARG, args
        assert lib.cpq_loudness_last_error(None)
    for rate in (44100.5, 7990.0, math.nan):
        assert lib.cpq_loudness_peaks_host(p(x), 16, 2, 16, rate, p(tp), p(sp)) == K.CPQ_ERR_UNSUPPORTED
    with pytest.raises(amd.CpqError) as e:
        amd.loudness_peaks_host(x, 44105.0)
    assert e.value.status == K.CPQ_ERR_UNSUPPORTED
