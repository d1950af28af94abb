"""Callers of the three FFT launch diagnostics (cpq_diag_fft_forward, cpq_diag_fft_inverse_store, cpq_diag_ir_spectra) and the
table of argument sets they must refuse, shared by tests/test_gpu_fft_variants.py (on the device) and
tests/test_host_and_abi_cpu.py (the refusals come before the device is looked for, so they are checked without one).

Every output array is filled with -7 here before the call: the entries return every buffer whole, so nothing of that
survives a successful call (what the launch left alone comes back as the entry's own 0xFF prefill)."""
import numpy as np

from fft_layout import dp, ip

INVALID_ARG, NO_DEVICE = -1, -2
TAB_MAX = 64
NAN_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)


def i64(v):
    return np.ascontiguousarray(v, dtype=np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def untouched(a):
    """every element still holds the entry's 0xFF prefill"""
    return bool((np.ascontiguousarray(a).view(np.uint64) == NAN_BITS).all())


def fft_forward(lib, P, n_ch, T, head, ring_slots, x, hist, side=0, n_side=0, strides=(), offs=(), tab=(), n_tab=None,
                tail_len=0, tail_stride=1, sized_as=None):
    """x: [n_ch][T * P + tail_len], hist: [n_ch][P].  sized_as: (P, n_ch, ring_slots, strides, tail_stride) for the output
    buffers when the arguments themselves are not to be trusted (refusal cases).  Returns (status, outputs)."""
    sP, sCh, sRing, sStrides, sTail = sized_as or (P, n_ch, ring_slots, strides, tail_stride)
    o = dict(ring=np.full((sCh, sRing, sP, 2), -7.0), xdn=np.full((sCh, sRing, 2), -7.0), hist_new=np.full((sCh, sP), -7.0),
             side=[np.full((sCh, int(s)), -7.0) for s in sStrides] + [np.full((1, 1), -7.0)] * (2 - len(sStrides)),
             tab=np.full(TAB_MAX, 7, dtype=np.int64), tail=np.full((sCh, max(int(sTail), 1)), -7.0))
    tab = i64(tab)
    n_tab = len(tab) if n_tab is None else n_tab
    st, of = i64(list(strides) + [0] * (3 - len(strides))), i64(list(offs) + [0] * (3 - len(offs)))
    rc = lib.cpq_diag_fft_forward(P, n_ch, T, head, ring_slots, tail_len, dp(x), dp(hist), side, n_side, ip(st), ip(of),
                                  ip(tab) if len(tab) else None, n_tab, tail_stride, dp(o["ring"]), dp(o["xdn"]), dp(o["hist_new"]),
                                  dp(o["side"][0]), dp(o["side"][1]), ip(o["tab"]), dp(o["tail"]))
    return rc, o


def fft_inverse_store(lib, mode, P, n_ch, T, spec, ring_a=None, pos_a=None, pos0=0, ring_b=None, pos_b=None, layer_out=None,
                      tail_ring=None, g0=0, sched=None, B=0, n_tail=0, g1=0.0, g2=0.0, sized_as=None):
    """spec: [n_ch][T][P][2]; ring_a / ring_b: [n_ch][size], copied, the copies come back in the outputs.
    Returns (status, dict(out=[n_ch][T * P], ring_a, ring_b))."""
    sP, sCh, sT = sized_as or (P, n_ch, T)
    o = dict(out=np.full((sCh, sT * sP), -7.0), ring_a=None if ring_a is None else ring_a.copy(),
             ring_b=None if ring_b is None else ring_b.copy())
    opt = lambda a, f: None if a is None else f(a)
    state = i64([0, 0, 0, g0])
    pos_a, pos_b, sched = opt(pos_a, i64), opt(pos_b, i64), opt(sched, i64)
    rc = lib.cpq_diag_fft_inverse_store(mode, P, n_ch, T, dp(spec), opt(o["ring_a"], dp), 0 if ring_a is None else ring_a.shape[1],
                                        opt(pos_a, ip), pos0, opt(o["ring_b"], dp), 0 if ring_b is None else ring_b.shape[1],
                                        opt(pos_b, ip), opt(layer_out, dp), opt(tail_ring, dp),
                                        0 if tail_ring is None else tail_ring.shape[2], ip(state), opt(sched, ip), B, n_tail,
                                        g1, g2, dp(o["out"]))
    return rc, o


def ir_spectra(lib, P, n_parts, heff, heff_len, gain=None, sized_as=None):
    """Returns (status, dict(h=[n_parts][P][2], hdn=[n_parts][2], h_gain, hdn_gain))."""
    sP, sParts = sized_as or (P, n_parts)
    o = dict(h=np.full((sParts, sP, 2), -7.0), hdn=np.full((sParts, 2), -7.0), h_gain=np.full((sParts, sP, 2), -7.0),
             hdn_gain=np.full((sParts, 2), -7.0))
    rc = lib.cpq_diag_ir_spectra(P, n_parts, dp(heff), heff_len, None if gain is None else dp(gain), dp(o["h"]), dp(o["hdn"]),
                                 dp(o["h_gain"]), dp(o["hdn_gain"]))
    return rc, o


# ---------------------------------------------------------------------------------------------------------------- refusals
# One valid call per entry (and per mode), small, and one override per refusal rule of include/convopeq_mi355x.h.

def _fwd_base():
    P, n_ch, T = 512, 2, 2
    return dict(P=P, n_ch=n_ch, T=T, head=3, ring_slots=4, x=np.ones((n_ch, T * P + 3)), hist=np.ones((n_ch, P)), side=1, n_side=2,
                strides=(4 * T * P + 8, 4 * T * P + 2), offs=(4, 2), tab=np.arange(5), tail_len=3, tail_stride=4)


def _plain_base():
    P, n_ch, T = 64, 2, 2
    return dict(P=P, n_ch=n_ch, T=T, head=3, ring_slots=4, x=np.ones((n_ch, T * P)), hist=np.ones((n_ch, P)))


FORWARD_REFUSALS = [          # (rule, base, override)
    ("partition not a power of two", _plain_base, dict(P=96)),
    ("partition below 64", _plain_base, dict(P=32)),
    ("partition above 131072", _plain_base, dict(P=262144)),
    ("no channel", _plain_base, dict(n_ch=0)),
    ("no block", _plain_base, dict(T=0)),
    ("ring_slots not a power of two", _plain_base, dict(ring_slots=6)),
    ("ring_slots below n_blocks", _plain_base, dict(ring_slots=1, head=0)),
    ("head negative", _plain_base, dict(head=-1)),
    ("head == ring_slots", _plain_base, dict(head=4)),
    ("ring above 2^28 elements", _plain_base, dict(P=131072, n_ch=2048, ring_slots=2, head=0)),
    ("tail without the side launch", _plain_base, dict(tail_len=1)),
    ("side carry at a partition other than 512", _fwd_base, dict(P=1024, x=np.ones((2, 2 * 1024 + 3)), hist=np.ones((2, 1024)))),
    ("three side destinations", _fwd_base, dict(n_side=3)),
    ("negative side count", _fwd_base, dict(n_side=-1)),
    ("odd side offset", _fwd_base, dict(offs=(4, 3))),
    ("odd side stride", _fwd_base, dict(strides=(4104, 4099))),
    ("negative side offset", _fwd_base, dict(offs=(-2, 2))),
    ("blocks beyond a side row", _fwd_base, dict(offs=(4, 3076))),
    ("table of 65 entries", _fwd_base, dict(tab=np.arange(65))),
    ("negative table length", _fwd_base, dict(n_tab=-1)),
    ("tail longer than its row", _fwd_base, dict(tail_len=5, x=np.ones((2, 2 * 512 + 5)))),
    ("tail_stride 0", _fwd_base, dict(tail_len=0, tail_stride=0, x=np.ones((2, 2 * 512)))),
    ("negative tail", _fwd_base, dict(tail_len=-1)),
]


def _spec(P, n_ch, T):
    return np.ones((n_ch, T, P, 2))


def _ring_base():
    P, n_ch, T = 64, 2, 2
    return dict(mode=1, P=P, n_ch=n_ch, T=T, spec=_spec(P, n_ch, T), ring_a=np.zeros((n_ch, 4 * P)), pos_a=[5, -1])


def _tail_base():
    P, n_ch, T = 64, 2, 2
    return dict(mode=2, P=P, n_ch=n_ch, T=T, spec=_spec(P, n_ch, T), layer_out=np.ones((2, n_ch, T * P)), tail_ring=np.ones((2, n_ch, 128)),
                g0=256, sched=[[256, -1], [3, 320]], B=64, n_tail=2, g1=1.0, g2=0.5)


def _add_base():
    P, n_ch, T = 512, 2, 2
    return dict(mode=3, P=P, n_ch=n_ch, T=T, spec=_spec(P, n_ch, T), ring_a=np.ones((n_ch, 1024)), pos_a=[3, -1],
                ring_b=np.ones((n_ch, 512)), pos_b=[-1, 8], g1=1.0, g2=0.5)


INVERSE_REFUSALS = [
    ("mode 0", _ring_base, dict(mode=0)),
    ("mode 4", _ring_base, dict(mode=4)),
    ("partition not a power of two", _ring_base, dict(P=96)),
    ("no channel", _ring_base, dict(n_ch=0)),
    ("no block", _ring_base, dict(T=0)),
    ("rows above 2^28 elements", _ring_base, dict(P=131072, n_ch=2048, T=2)),
    ("ring smaller than a block", _ring_base, dict(ring_a=np.zeros((2, 32)))),
    ("ring size not a power of two", _ring_base, dict(ring_a=np.zeros((2, 192)))),
    ("no ring", _ring_base, dict(ring_a=None)),
    ("two blocks on the same elements", _ring_base, dict(pos_a=[5, 40])),
    ("two blocks that meet across the ring end", _ring_base, dict(pos_a=[5, 4 * 64 - 20])),
    ("consecutive blocks that lap the ring", _ring_base, dict(pos_a=None, pos0=0, ring_a=np.zeros((2, 64)))),
    ("negative pos0", _ring_base, dict(pos_a=None, pos0=-64)),
    ("position above 2^62", _ring_base, dict(pos_a=[5, (1 << 62) + 64])),
    ("tail store above 4096", _tail_base, dict(P=8192)),
    ("three tail layers", _tail_base, dict(n_tail=3)),
    ("no tail layer", _tail_base, dict(n_tail=0)),
    ("callback size not a power of two", _tail_base, dict(B=48)),
    ("callback size not dividing the call", _tail_base, dict(B=256)),
    ("callback size 0", _tail_base, dict(B=0)),
    ("tail ring size not a power of two", _tail_base, dict(tail_ring=np.ones((2, 2, 96)))),
    ("tail ring of one element", _tail_base, dict(tail_ring=np.ones((2, 2, 1)))),
    ("schedule entry beyond the call", _tail_base, dict(sched=[[256, -1], [3, 321]])),
    ("negative g0", _tail_base, dict(g0=-64, sched=[[-1, -1], [-1, -1]])),
    ("no schedule", _tail_base, dict(sched=None)),
    ("no layer rows", _tail_base, dict(layer_out=None)),
    ("add store at a partition other than 512", _add_base, dict(P=1024)),
    ("ring A smaller than a block", _add_base, dict(ring_a=np.ones((2, 256)))),
    ("ring B not a power of two", _add_base, dict(ring_b=np.ones((2, 768)))),
    ("ring B without a schedule", _add_base, dict(pos_b=None)),
    ("no schedule A", _add_base, dict(pos_a=None)),
    ("position above 2^62", _add_base, dict(pos_a=[3, (1 << 62) + 1])),
]


def _ir_base():
    return dict(P=64, n_parts=2, heff=np.ones(128), heff_len=100, gain=np.ones(65))


IR_REFUSALS = [
    ("partition not a power of two", _ir_base, dict(P=96)),
    ("partition below 64", _ir_base, dict(P=32)),
    ("no partition", _ir_base, dict(n_parts=0)),
    ("empty h_eff", _ir_base, dict(heff_len=0)),
    ("h_eff longer than the partitions", _ir_base, dict(heff_len=129)),
    ("buffer above 2^28 elements", _ir_base, dict(P=131072, n_parts=4096)),
]


def _sizes(kind, b):
    if kind == "forward":
        return (b["P"], b["n_ch"], b["ring_slots"], b.get("strides", ()), b.get("tail_stride", 1))
    if kind == "inverse":
        return (b["P"], b["n_ch"], b["T"])
    return (b["P"], b["n_parts"])


CALLERS = {"forward": fft_forward, "inverse": fft_inverse_store, "ir": ir_spectra}
REFUSALS = {"forward": FORWARD_REFUSALS, "inverse": INVERSE_REFUSALS, "ir": IR_REFUSALS}
VALID = {"forward": [_plain_base, _fwd_base], "inverse": [_ring_base, _tail_base, _add_base], "ir": [_ir_base]}


def walk_refusals(lib):
    """every refusal rule once: [(entry, rule, status)], the output buffers sized for the valid base"""
    res = []
    for kind, rules in REFUSALS.items():
        for rule, base, override in rules:
            b = base()
            args = dict(b, **override)
            rc, _ = CALLERS[kind](lib, sized_as=_sizes(kind, b), **args)
            res.append((kind, rule, rc))
    return res


def valid_calls(lib):
    """the base argument sets themselves: [(entry, status)]"""
    return [(kind, CALLERS[kind](lib, **base())[0]) for kind, bases in VALID.items() for base in bases]
