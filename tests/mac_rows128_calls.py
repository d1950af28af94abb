"""cpq_diag_fdl_mac with tile = ROWS128, the id that forces the cooperative kernel's 128-row workgroup at any T: the argument
sets it accepts and the ones it must refuse, shared by tests/test_gpu_fdl_mac_rows128.py (on the device) and
tests/test_fdl_mac_rows128_cpu.py (the refusals come before the device is looked for).  The caller and the buffers are those
of tests/mac_fft_calls.py; the sizing rules are the engines' and do not depend on the variant."""
from mac_fft_calls import MAC_GOOD

ROWS128 = -2                    # kMacTileRows128 (csrc/kernels.hpp)
ROWS128_USED = 128              # what *variant_used reports for it (kMacVariantRows128)

ROWS128_GOOD = dict(MAC_GOOD, tile=ROWS128)
ROWS128_BAD = {
    "ring not a power of two": dict(ring=96),
    "ring below the engines' rule": dict(ring=64),
    "ring below the rule at T = 128": dict(T=128, ring=128),          # nextPow2(32 + 32 + 128) = 256
    "h_rows below alignUp(K, 32) + 16": dict(h_rows=47),
    "ir_slot = n_ir_slots": dict(slots=(2, 0)),
    "head = ring_slots": dict(head=128),
    "P below 64": dict(P=32),
    "K zero": dict(K=0),
    "T zero": dict(T=0),
    "no channels": dict(n_ch=0),
    "the id below it": dict(tile=ROWS128 - 1),
}
