"""The refusals of cpq_scorer that need no device: malformed descs (refused before a device is looked for), null handles, and
the host-only entry points' argument rules.  A well-formed desc gives CPQ_ERR_NO_DEVICE where there is no gfx950 device -- there
is no CPU fallback -- and a scorer where there is one."""
import ctypes as C

import numpy as np
import pytest

OK, INVALID, NO_DEVICE = 0, -1, -2
GOOD = dict(n_learners=2, max_candidates=18, sample_rate_hz=48000.0, bit_depth=16, level_weights=(0.4, 0.3, 0.2, 0.1),
            coeff_safety_margin=0.85, stability_check=1, rng_mode=0)
BAD = [("n_learners", 0), ("n_learners", -3), ("max_candidates", 0), ("max_candidates", 1025), ("max_candidates", 1 << 20), ("sample_rate_hz", 0.0), ("sample_rate_hz", float("nan")),
       ("sample_rate_hz", float("inf")), ("bit_depth", 0), ("bit_depth", 33), ("level_weights", (0.4, -0.1, 0.2, 0.1)),
       ("level_weights", (0.4, float("nan"), 0.2, 0.1)), ("coeff_safety_margin", 0.0), ("coeff_safety_margin", 1.5),
       ("stability_check", 2), ("rng_mode", 2), ("rng_mode", -1)]


@pytest.fixture(scope="module")
def K():
    from convopeq_amd import _capi
    _capi.load()
    return _capi


def make_desc(K, **over):
    d = dict(GOOD, **over)
    return K.ScorerDesc(d["n_learners"], d["max_candidates"], d["sample_rate_hz"], d["bit_depth"], (C.c_double * 4)(*d["level_weights"]),
                        d["coeff_safety_margin"], d["stability_check"], d["rng_mode"])


@pytest.mark.parametrize("field,value", BAD)
def test_malformed_desc(K, field, value):
    lib, h = K.load(), C.c_void_p(1)
    desc = make_desc(K, **{field: value})
    assert lib.cpq_scorer_create(C.byref(desc), C.byref(h)) == INVALID and not h.value
    assert lib.cpq_scorer_last_error(None) != b""


def test_null_arguments_and_handles(K):
    lib, h = K.load(), C.c_void_p()
    desc = make_desc(K)
    assert lib.cpq_scorer_create(None, C.byref(h)) == INVALID and lib.cpq_scorer_create(C.byref(desc), None) == INVALID
    rc = lib.cpq_scorer_create(C.byref(desc), C.byref(h))
    assert rc in (OK, NO_DEVICE)                        # no fallback: a scorer only where the device is
    if rc == OK:
        lib.cpq_scorer_destroy(h)
    else:
        assert not h.value and b"no CPU fallback" in lib.cpq_scorer_last_error(None)
    x, n = np.zeros(4096), C.c_int32(7)
    xp = x.ctypes.data_as(K.c_double_p)
    assert lib.cpq_scorer_set_audio(None, 0, xp, xp, 4096, C.byref(n)) == INVALID
    assert lib.cpq_scorer_set_audio_device(None, 0, None, None, 0, None) == INVALID
    assert lib.cpq_scorer_score(None, xp, 1, xp, None) == INVALID and lib.cpq_scorer_score_raw(None, xp, 1, xp, None) == INVALID
    assert lib.cpq_scorer_get_segments(None, 0, None, None, None) == INVALID
    assert lib.cpq_scorer_read_thresholds(None, 0, 0, xp) == INVALID and lib.cpq_scorer_read_error(None, 0, 0, 0, xp, xp) == INVALID
    assert lib.cpq_scorer_set_rng_start(None, None) == INVALID and lib.cpq_scorer_last_timing(None, None, None) == INVALID
    lib.cpq_scorer_destroy(None)
    assert n.value == 7


def test_host_entry_points_refuse(K):
    lib = K.load()
    x = np.zeros(10)
    xp = x.ctypes.data_as(K.c_double_p)
    for rate in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.cpq_score_design(rate, None, None, None, None, None, None, None, None) == INVALID
    assert lib.cpq_score_design(48000.0, None, None, None, None, None, None, None, None) == OK
    n = C.c_int32(-1)
    assert lib.cpq_score_select_segments(xp, xp, -1, None, C.byref(n), None) == INVALID
    assert lib.cpq_score_select_segments(None, xp, 10, None, C.byref(n), None) == INVALID and n.value == -1
    assert lib.cpq_score_select_segments(xp, xp, 10, None, C.byref(n), None) == OK and n.value == 0
    assert lib.cpq_score_select_segments(None, None, 0, None, C.byref(n), None) == OK
    header = open(__import__("os").path.join(__import__("os").path.dirname(K.LIB_PATH), "..", "include", "convopeq_mi355x.h")).read()
    assert "#define CPQ_HAS_SHAPER_SCORING 1" in header and "FFT parity unpinned" in header
    assert K.CPQ_SCORE_RNG_FRESH == 0 and K.CPQ_SCORE_RNG_CHAINED == 1 and K.CPQ_SCORE_RECENT == 34816
