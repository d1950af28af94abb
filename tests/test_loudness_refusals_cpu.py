"""The refusals of cpq_loudness that need no device, and what the host-only entry points compute (cpq_loudness_finish_host,
cpq_loudness_gain)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import convopeq_amd as amd
from convopeq_amd import _capi as K

import prog_model as P

HERE = os.path.dirname(os.path.abspath(__file__))


def _create(n_streams=2, rate=48000.0, seconds=60.0, flags=0):
    h = C.c_void_p()
    rc = K.load().cpq_loudness_create(C.byref(K.LoudnessDesc(n_streams, rate, seconds, flags)), C.byref(h))
    return rc, h


def test_the_header_announces_the_object():
    header = open(os.path.join(os.path.dirname(HERE), "include", "convopeq_mi355x.h")).read()
    assert "#define CPQ_HAS_PROGRAMME_LOUDNESS 1" in header
    assert C.sizeof(K.LoudnessResult) == 64 and C.sizeof(K.LoudnessDesc) == 32


def test_create_refusals_come_before_the_question_of_a_device():
    lib = K.load()
    for kwargs, status in ((dict(n_streams=0), K.CPQ_ERR_INVALID_ARG), (dict(n_streams=32768), K.CPQ_ERR_INVALID_ARG),
                           (dict(flags=1), K.CPQ_ERR_INVALID_ARG), (dict(seconds=0.0), K.CPQ_ERR_INVALID_ARG),
                           (dict(seconds=math.nan), K.CPQ_ERR_INVALID_ARG), (dict(seconds=math.inf), K.CPQ_ERR_INVALID_ARG),
                           (dict(rate=math.nan), K.CPQ_ERR_INVALID_ARG), (dict(rate=-48000.0), K.CPQ_ERR_INVALID_ARG),
                           (dict(rate=44100.5), K.CPQ_ERR_UNSUPPORTED), (dict(rate=44105.0), K.CPQ_ERR_UNSUPPORTED),
                           (dict(rate=7990.0), K.CPQ_ERR_UNSUPPORTED), (dict(rate=768010.0), K.CPQ_ERR_UNSUPPORTED),
                           (dict(seconds=8195.0), K.CPQ_ERR_UNSUPPORTED)):
        rc, h = _create(**kwargs)
        assert rc == status and not h.value, kwargs
        assert lib.cpq_loudness_last_error(None)
    assert lib.cpq_loudness_create(None, C.byref(C.c_void_p())) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_create(C.byref(K.LoudnessDesc(1, 48000.0, 1.0, 0)), None) == K.CPQ_ERR_INVALID_ARG


def test_the_object_needs_a_device():
    """CPQ_ERR_NO_DEVICE where no gfx950 is visible (there is no host object); CPQ_OK where one is.  8194 s is the longest
    programme the range's sort holds."""
    lib = K.load()
    rc, h = _create(1, 8000.0, 8194.0)
    assert rc in (K.CPQ_OK, K.CPQ_ERR_NO_DEVICE)
    if rc == K.CPQ_OK:
        assert h.value
        lib.cpq_loudness_destroy(h)
    else:
        assert not h.value and lib.cpq_loudness_last_error(None)
        with pytest.raises(amd.CpqError) as e:
            amd.ProgrammeLoudness(2, 48000, 60)
        assert e.value.status == K.CPQ_ERR_NO_DEVICE


def test_null_handles():
    lib = K.load()
    x = np.zeros((2, 16))
    res = K.LoudnessResult()
    n = C.c_int64()
    assert lib.cpq_loudness_process(None, x.ctypes.data, 16, 16) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_process_device(None, x.ctypes.data, 16, 16) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_finish(None, C.byref(res)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_read_hops(None, 0, None, 0, C.byref(n)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_reset(None) == K.CPQ_ERR_INVALID_ARG and lib.cpq_loudness_set_stream(None, None) == K.CPQ_ERR_INVALID_ARG
    lib.cpq_loudness_destroy(None)


def test_finish_host_is_the_model_and_gain():
    lib = K.load()
    rng = np.random.default_rng(3)
    E = 800.0 * 10.0 ** rng.uniform(-3.0, -1.5, size=450)
    got, want = amd.loudness_finish_host(E, 8000), P.finish(E, 800)
    for key in ("n_hops", "n_blocks", "n_abs", "n_rel", "n_short_kept"):
        assert got[key] == want[key], key
    tol = 10.0 / math.log(10.0) * want["n_blocks"] * 2.0 ** -52
    for key in ("integrated", "relative_gate", "momentary_max", "short_term_max"):
        assert abs(got[key] - want[key]) <= tol, key
    assert abs(got["range"] - want["range"]) <= 2 * tol and got["range"] > 1.0
    empty = amd.loudness_finish_host(np.zeros(0), 8000)
    assert empty["n_hops"] == 0 and empty["integrated"] == -math.inf and empty["range"] == 0.0
    with pytest.raises(amd.CpqError) as e:
        amd.loudness_finish_host(E, 44100.5)
    assert e.value.status == K.CPQ_ERR_UNSUPPORTED
    g = C.c_double(-1.0)
    r = K.LoudnessResult(**got)
    assert lib.cpq_loudness_gain(C.byref(r), -23.0, C.byref(g)) == K.CPQ_OK
    assert abs(g.value / 10.0 ** ((-23.0 - got["integrated"]) / 20.0) - 1.0) <= 2.0 ** -50
    g.value = -1.0
    assert lib.cpq_loudness_gain(C.byref(K.LoudnessResult(**empty)), -23.0, C.byref(g)) == K.CPQ_ERR_NOT_READY and g.value == -1.0
    assert lib.cpq_loudness_gain(None, -23.0, C.byref(g)) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_loudness_gain(C.byref(r), -23.0, None) == K.CPQ_ERR_INVALID_ARG
