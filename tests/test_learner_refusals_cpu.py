"""The refusals of cpq_learner and of the host-only entries of the optimiser that need no device: null handles and arguments, and
values out of range.  Nothing here creates a scorer, so nothing here needs a gfx950."""
import ctypes as C
import os

import numpy as np
import pytest

OK, INVALID = 0, -1


@pytest.fixture(scope="module")
def K():
    from convopeq_amd import _capi
    _capi.load()
    return _capi


def dp(K, a):
    return a.ctypes.data_as(K.c_double_p)


def params(K, *v):
    v = v or (0.03, 0.30, 0.92, 0.0)
    return K.LearnParams(*v[:4], (C.c_double * 4)(*(v[4] if len(v) > 4 else (0.4, 0.3, 0.2, 0.1))))


def test_null_handles(K):
    lib, h = K.load(), C.c_void_p(1)
    st, p, x = K.LearnState(), params(K), np.zeros(162)
    n = C.c_int32(7)
    assert lib.cpq_learner_create(None, C.byref(h)) == INVALID and not h.value
    assert lib.cpq_learner_create(None, None) == INVALID and lib.cpq_last_error(None) != b""
    assert lib.cpq_learner_init(None, 0, dp(K, x), 1) == INVALID and lib.cpq_learner_set_params(None, C.byref(p)) == INVALID
    assert lib.cpq_learner_run(None, 1) == INVALID
    assert lib.cpq_learner_get_state(None, 0, C.byref(st)) == INVALID and lib.cpq_learner_set_state(None, 0, C.byref(st)) == INVALID
    assert lib.cpq_learner_read_generation(None, 0, None, None, None, None, None) == INVALID
    assert lib.cpq_learner_read_history(None, 0, None, C.byref(n)) == INVALID and n.value == 7
    assert lib.cpq_learner_published(None, 0, dp(K, x)) == INVALID and lib.cpq_learner_last_timing(None, None, None) == INVALID
    lib.cpq_learner_destroy(None)
    assert lib.cpq_learner_last_error(None) is not None


def test_host_entries_refuse_null_arguments(K):
    lib = K.load()
    st, p, x, o = K.LearnState(), params(K), np.zeros(162), np.zeros(18, dtype=np.int32)
    xp = dp(K, x)
    assert lib.cpq_learn_init_host(None, 1, None, C.byref(st)) == INVALID and lib.cpq_learn_init_host(xp, 1, None, None) == INVALID
    assert lib.cpq_learn_init_host(xp, 1, None, C.byref(st)) == OK
    assert lib.cpq_learn_normals_host(None, xp, None) == INVALID and lib.cpq_learn_normals_host(C.byref(st), None, None) == INVALID
    assert lib.cpq_learn_normals_host(C.byref(st), xp, None) == OK
    assert lib.cpq_learn_ask_host(None, xp, xp) == INVALID and lib.cpq_learn_ask_host(C.byref(st), None, xp) == INVALID
    assert lib.cpq_learn_ask_host(C.byref(st), xp, None) == INVALID
    for args in ((None, C.byref(p), xp, xp, xp), (C.byref(st), None, xp, xp, xp), (C.byref(st), C.byref(p), None, xp, xp),
                 (C.byref(st), C.byref(p), xp, xp, None)):
        assert lib.cpq_learn_tell_host(*args, None) == INVALID
    assert lib.cpq_learn_tell_host(C.byref(st), C.byref(p), xp, None, xp, o.ctypes.data_as(C.POINTER(C.c_int32))) == OK
    assert lib.cpq_learn_phase_params(0, 1, None, None) == INVALID
    assert lib.cpq_diag_learn_tell(1, None, C.byref(p), xp, xp, xp) == INVALID and lib.cpq_diag_learn_tell(0, (K.LearnState * 1)(), C.byref(p), xp, xp, xp) == INVALID


def test_values_out_of_range(K):
    lib = K.load()
    st, x = K.LearnState(), np.zeros(162)
    bad = np.zeros(9)
    bad[4] = float("nan")
    assert lib.cpq_learn_init_host(dp(K, bad), 1, None, C.byref(st)) == INVALID
    bad[4] = float("inf")
    assert lib.cpq_learn_init_host(dp(K, bad), 1, None, C.byref(st)) == INVALID
    nan = float("nan")
    for v in ((0.0, 0.3, 0.92, 0.0), (-0.1, 0.3, 0.92, 0.0), (0.4, 0.3, 0.92, 0.0), (0.03, nan, 0.92, 0.0), (0.03, 0.3, 1.5, 0.0),
              (0.03, 0.3, -0.1, 0.0), (0.03, 0.3, 0.92, -0.01), (0.03, 0.3, 0.92, float("inf")), (0.03, 0.3, 0.92, 0.0, (0.4, -0.1, 0.2, 0.1)),
              (0.03, 0.3, 0.92, 0.0, (0.4, nan, 0.2, 0.1))):
        p = params(K, *v)
        assert lib.cpq_learn_init_host(dp(K, x), 1, C.byref(p), C.byref(st)) == INVALID, v
        assert lib.cpq_learn_tell_host(C.byref(st), C.byref(p), dp(K, x), None, dp(K, x), None) == INVALID, v
    for mode in (-1, 6, 100):
        assert lib.cpq_learn_phase(mode, 1.0) == INVALID and lib.cpq_learn_phase_params(mode, 1, C.byref(K.LearnParams()), None) == INVALID
    for seconds in (nan, float("inf")):
        assert lib.cpq_learn_phase(0, seconds) == INVALID
    for ph in (0, 4, -1):
        assert lib.cpq_learn_phase_params(0, ph, C.byref(K.LearnParams()), None) == INVALID
    assert lib.cpq_learn_phase(5, 0.0) == 1 and lib.cpq_learn_phase_params(5, 3, C.byref(K.LearnParams()), None) == OK


def test_header_and_constants(K):
    header = open(os.path.join(os.path.dirname(K.LIB_PATH), "..", "include", "convopeq_mi355x.h")).read()
    assert "#define CPQ_HAS_SHAPER_LEARNING 1" in header and "(a + a) * 0.5 == a" in header
    assert "#define CPQ_ABI_REVISION 1" in header
    assert C.sizeof(K.LearnState) == 640 and C.sizeof(K.LearnParams) == 64
    assert (K.CPQ_LEARN_DIM, K.CPQ_LEARN_POPULATION, K.CPQ_LEARN_ELITE, K.CPQ_LEARN_MAX_GENERATIONS, K.CPQ_LEARN_MAX_TRIES) == (9, 18, 6, 4096, 32)
