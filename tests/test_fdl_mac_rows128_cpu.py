"""The rules of cpq_diag_fdl_mac for the 128-row variant id without a device (tests/mac_rows128_calls.py): every refusal is
CPQ_ERR_INVALID_ARG with the outputs and *variant_used as they were, and the good set gets past the checks."""
import pytest

from mac_fft_calls import INVALID_ARG, MAC_POINTERS, NO_DEVICE, mac_buffers, mac_call, mac_untouched
from mac_rows128_calls import ROWS128_BAD, ROWS128_GOOD, ROWS128_USED


@pytest.fixture(scope="module")
def lib():
    from convopeq_amd import _capi
    return _capi.load()


@pytest.mark.parametrize("rule", list(ROWS128_BAD))
def test_rows128_refusals(lib, rule):
    a = dict(ROWS128_GOOD, **ROWS128_BAD[rule])
    X, H, Y, used = mac_buffers(a)
    assert mac_call(lib, a, X, H, Y, used) == INVALID_ARG
    assert mac_untouched(Y, used)


def test_rows128_null_pointers(lib):
    for name in MAC_POINTERS:
        X, H, Y, used = mac_buffers(ROWS128_GOOD)
        assert mac_call(lib, ROWS128_GOOD, X, H, Y, used, null=name) == INVALID_ARG
        assert mac_untouched(Y, used)


def test_rows128_good_set_passes_the_checks(lib):
    import torch
    X, H, Y, used = mac_buffers(ROWS128_GOOD)
    rc = mac_call(lib, ROWS128_GOOD, X, H, Y, used)
    if torch.cuda.is_available():         # it then runs (what it computes: tests/test_gpu_fdl_mac_rows128.py)
        assert rc == 0 and used.value == ROWS128_USED
    else:
        assert rc == NO_DEVICE and mac_untouched(Y, used)
