"""The partition FFT kernels keep their bits (convopeq_amd/csrc/fft_kernels.hip): for every partition size of
tests/test_gpu_fft.py and that module's inputs, SHA-256 of the spectra and of the rows that cpq_diag_partition_fft returns
equals the digest recorded in tests/golden/fft_bits.json.  The file was written on an MI355X by tests/fft_bits.py from a build
of the commit it names -- the last one before the families' shared arithmetic (real-FFT split and its inverse, frame and IR
loads, radix stages) moved into one helper each -- and is not regenerated from the code under test: a digest that differs
means a rounding changed.  The kernels have no atomics and the build uses -ffp-contract=off, so there is no tolerance.

The other launch paths (ring, tail and add stores, side carry, moving head, IR spectra and gain, ragged P = 4096 split) are
tied bit for bit to this entry by tests/test_gpu_fft_variants.py and tests/test_gpu_fft_p4_frames.py."""
import pytest

import fft_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need a gfx950 device")
    from convopeq_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def golden():
    return fft_bits.golden()


def test_golden_file_covers_every_size(golden):
    assert len(golden["commit"]) == 40
    assert sorted(int(p) for p in golden["sha256"]) == fft_bits.SIZES


@pytest.mark.parametrize("P", fft_bits.SIZES)
def test_partition_fft_bits(lib, golden, P):
    spec, out = fft_bits.digests(lib, P)
    want = golden["sha256"][str(P)]
    assert spec == want["spec"], (P, "spectra differ from commit " + golden["commit"])
    assert out == want["out"], (P, "rows differ from commit " + golden["commit"])
