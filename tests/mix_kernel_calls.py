"""Callers of the mix-kernel diagnostics (cpq_diag_direct_head, _agc, _ring_chunks, _convproc_mix, _tail_reader, _rows) and the
table of argument sets they must refuse, shared by tests/test_gpu_mix_kernels.py (on the device, where every valid base set
runs for real) and tests/test_host_and_abi_cpu.py (the refusals come before the device is looked for).

Every caller copies its in-and-out arrays, fills pure outputs with -7 (the entries return every buffer whole, so nothing of
that survives a successful call: what a launch leaves alone comes back as the entry's 0xFF prefill) and returns
(status, dict of outputs)."""
import ctypes as C

import numpy as np

INVALID_ARG, NO_DEVICE = -1, -2
TAB_MAX = 64
FF = np.uint64(0xFFFFFFFFFFFFFFFF)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _p(a):
    if a is None:
        return None
    t = {np.dtype(np.float64): C.c_double, np.dtype(np.int32): C.c_int32, np.dtype(np.int64): C.c_int64}[a.dtype]
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(t))


def _opt(a, conv):
    return None if a is None else conv(a)


def ff(shape):
    """float64 array of the 0xFF prefill (a NaN with every bit set)"""
    a = np.empty(shape, dtype=np.uint64)
    a[...] = FF
    return a.view(np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    return bool(np.array_equal(a, b))


def untouched(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return bool((a.view(np.uint64) == FF).all())
    return bool((a == -1).all())


def direct_head(lib, x, ir_rev, taps, ir_slot, hist_old, n=None, wet_on=None, out=None, n_ch=None, n_slots=None, in_stride=None,
                out_stride=None):
    """x: [n_ch][in_stride]; outputs dout [n_ch][n], hist_new [n_ch][32], out (copy) or None"""
    x, ir_rev, taps, ir_slot, hist_old = f64(x), f64(ir_rev), i32(taps), i32(ir_slot), f64(hist_old)
    wet_on, o_out = _opt(wet_on, i32), _opt(out, lambda a: f64(a).copy())
    n_ch = x.shape[0] if n_ch is None else n_ch
    n = x.shape[1] if n is None else n
    o = dict(dout=np.full((x.shape[0], max(n, 1)), -7.0), hist_new=np.full((x.shape[0], 32), -7.0), out=o_out)
    rc = lib.cpq_diag_direct_head(n_ch, n, x.shape[1] if in_stride is None else in_stride, len(taps) if n_slots is None else n_slots,
                                  _p(x), _p(ir_rev), _p(taps), _p(ir_slot), _p(hist_old), _p(wet_on), _p(o["dout"]), _p(o["hist_new"]),
                                  _p(o_out), (0 if out is None else o_out.shape[1]) if out_stride is None else out_stride)
    return rc, o


def agc(lib, op, data, B, T, rms_in=None, rms_out=None, state=None, on=None, gains=None, coef=(0.0, 0.0, 0.0), n_ch=None,
        ch_stride=None):
    """op 0 rms, 1 apply, 2 gain ramp, 3 silence.  data: [n_ch][ch_stride]"""
    data = f64(data).copy()
    nc = data.shape[0]
    S = max(nc // 2, 1)
    Tn = max(T, 1)
    o = dict(data=data, rms=np.full((nc, Tn), -7.0), silent=np.full((S, Tn), -7, dtype=np.int32),
             state=_opt(state, lambda a: f64(a).copy()), gains=f64(gains).copy() if op == 2 else np.full((S, Tn, 2), -7.0))
    rc = lib.cpq_diag_agc(op, nc if n_ch is None else n_ch, B, T, data.shape[1] if ch_stride is None else ch_stride, _p(data),
                          _p(_opt(rms_in, f64)), _p(_opt(rms_out, f64)), _p(o["state"]), _p(_opt(on, i32)), _p(o["gains"]),
                          coef[0], coef[1], coef[2], _p(o["rms"]), _p(o["silent"]))
    return rc, o


GATHER, GET, ADD, ADD2, GET_ADD = range(5)


def ring_chunks(lib, op, out, ch_map, n, q, ring0=None, pos=None, cnt=None, ring_a=None, sched_a=None, gain_a=1.0, ring_b=None,
                sched_b=None, gain_b=1.0, strides=(), offs=(), tab=None, n_tab=None, rows=None, n_dst=None, out_stride=None):
    """out: [rows][out_stride] (the source of the gather).  Outputs: out (copy), dst (list), tab"""
    o_out, ch_map = f64(out).copy(), i32(ch_map)
    nc = len(ch_map)
    ring0, ring_a, ring_b = _opt(ring0, f64), _opt(ring_a, f64), _opt(ring_b, f64)
    pos, cnt, sched_a, sched_b = _opt(pos, i64), _opt(cnt, i64), _opt(sched_a, i64), _opt(sched_b, i64)
    dst = [np.full((nc, max(int(s), 1)), -7.0) for s in strides] + [None] * (3 - len(strides))
    st, of = i64(list(strides) + [0] * (3 - len(strides))), i64(list(offs) + [0] * (3 - len(offs)))
    tab = _opt(tab, i64)
    tab_out = np.full(TAB_MAX, 7, dtype=np.int64)
    size = lambda r: 0 if r is None else r.shape[1]
    rc = lib.cpq_diag_ring_chunks(op, o_out.shape[0] if rows is None else rows, nc, n, q, o_out.shape[1] if out_stride is None else out_stride,
                                  _p(o_out), _p(ch_map), _p(ring0), size(ring0), _p(pos), _p(cnt), _p(ring_a), size(ring_a), _p(sched_a),
                                  gain_a, _p(ring_b), size(ring_b), _p(sched_b), gain_b, len(strides) if n_dst is None else n_dst,
                                  _p(st), _p(of), _p(dst[0]), _p(dst[1]), _p(dst[2]), _p(tab),
                                  (0 if tab is None else len(tab)) if n_tab is None else n_tab, _p(tab_out))
    return rc, dict(out=o_out, dst=dst, tab=tab_out)


def convproc_mix(lib, wet, n, gains, ring, pos0, d_new, d_old, x_len=None, x_gains=None, wet_valid=1, ramp_len=None, ramp_gains=None,
                 ramp_off=0, wet_on=None, in_place=0, old_ring=None, regrow_end=0, ring_in=None, n_put=0, n_ch=None, ring_size=None,
                 x_cap=None, ramp_cap=None, old_size=None, ch_stride=None):
    """wet: [n_ch][ch_stride]; ring: [n_ch][size].  Outputs: out [n_ch][ch_stride], ring (copy)"""
    wet, gains, o_ring = f64(wet), f64(gains), f64(ring).copy()
    x_gains, ramp_gains, old_ring, ring_in = _opt(x_gains, f64), _opt(ramp_gains, f64), _opt(old_ring, f64), _opt(ring_in, f64)
    o = dict(out=np.full(wet.shape, -7.0), ring=o_ring)
    rc = lib.cpq_diag_convproc_mix(wet.shape[0] if n_ch is None else n_ch, n, wet.shape[1] if ch_stride is None else ch_stride, _p(wet), _p(o["out"]), in_place, _p(gains),
                                   _p(o_ring), o_ring.shape[1] if ring_size is None else ring_size, pos0, _p(i32(d_new)), _p(i32(d_old)),
                                   _p(_opt(x_len, i32)), _p(x_gains),
                                   (0 if x_gains is None else x_gains.shape[1]) if x_cap is None else x_cap, wet_valid,
                                   _p(_opt(ramp_len, i32)), _p(ramp_gains),
                                   (0 if ramp_gains is None else ramp_gains.shape[1]) if ramp_cap is None else ramp_cap, ramp_off,
                                   _p(_opt(wet_on, i32)), _p(old_ring),
                                   (0 if old_ring is None else old_ring.shape[1]) if old_size is None else old_size, regrow_end,
                                   _p(ring_in), 0 if ring_in is None else ring_in.shape[1], n_put)
    return rc, o


def tail_reader(lib, T, B, layers, state, layer_out=None, ring=None, n_tail=None, n_calls=None, ring_size=None, n_ch=None,
                n_samples=None):
    """T: callbacks per call; layers: [(PL, oL, D)].  Outputs: sched (list per call of [n_tail][T[i]]), states [calls][4], ring"""
    T, state = i32(T), i64(state)
    nt = len(layers) if n_tail is None else n_tail
    lay = list(layers) + [(0, 0, 0)] * (2 - len(layers))
    total = int(np.clip(T, 0, None).sum())
    sched = np.full(max(2 * total, 1), 7, dtype=np.int64)
    states = np.full((len(T), 4), 7, dtype=np.int64)
    layer_out, o_ring = _opt(layer_out, f64), _opt(ring, lambda a: f64(a).copy())
    rc = lib.cpq_diag_tail_reader(len(T) if n_calls is None else n_calls, _p(T), B, nt, lay[0][0], lay[0][1], lay[0][2], lay[1][0], lay[1][1],
                                  lay[1][2], _p(state), _p(sched), _p(states),
                                  (0 if layer_out is None else layer_out.shape[1]) if n_ch is None else n_ch,
                                  (0 if layer_out is None else layer_out.shape[2]) if n_samples is None else n_samples, _p(layer_out), _p(o_ring),
                                  (0 if o_ring is None else o_ring.shape[2]) if ring_size is None else ring_size)
    per_call, at = [], 0
    for t in T:
        t = max(int(t), 0)
        per_call.append(sched[at: at + nt * t].reshape(nt, t) if 1 <= nt <= 2 else None)
        at += max(nt, 0) * t
    return rc, dict(sched=per_call, states=states, ring=o_ring)


COPY, SCALE, BLEND = range(3)


def rows(lib, op, dst, n, src=None, src_off=0, dst_off=0, gain=None, on=None, length=None, g_end=None, gains=None, n_ch=None, cap=None,
         src_stride=None, dst_stride=None):
    o_dst, src, gains = f64(dst).copy(), _opt(src, f64), _opt(gains, f64)
    rc = lib.cpq_diag_rows(op, o_dst.shape[0] if n_ch is None else n_ch, n, _p(src),
                           (0 if src is None else src.shape[1]) if src_stride is None else src_stride, src_off, _p(o_dst),
                           o_dst.shape[1] if dst_stride is None else dst_stride, dst_off, _p(_opt(gain, f64)), _p(_opt(on, i32)), _p(_opt(length, i32)), _p(_opt(g_end, f64)),
                           _p(gains), (0 if gains is None else gains.shape[1]) if cap is None else cap)
    return rc, dict(dst=o_dst)


# ---------------------------------------------------------------------------------------------------------------- refusals
# One valid call per entry and op, small, and one override per refusal rule of include/convopeq_mi355x.h.

def _head_base():
    return dict(x=np.ones((4, 12)), n=9, ir_rev=np.ones((3, 32)), taps=[32, 0, 5], ir_slot=[2, 0, 0, 1], hist_old=np.ones((4, 32)),
                wet_on=[1, 0], out=np.ones((4, 11)))


def _agc_base(op):
    def base():
        b = dict(op=op, data=np.ones((4, 13)), B=3, T=4)
        if op == 1:
            b.update(rms_in=np.ones((4, 4)), rms_out=np.ones((4, 4)), state=np.array([[0.0, 0.0, 1.0]] * 2), on=[1, 0], coef=(0.5, 0.25, 0.125))
        if op == 2:
            b.update(gains=np.ones((2, 4, 2)), on=[0, 1])
        return b
    return base


def _chunks_base(op):
    def base():
        n, q = 11, 4
        b = dict(op=op, out=np.ones((6, 13)), ch_map=[2, -1, 5, 0], n=n, q=q)
        if op == GATHER:
            b.update(strides=(12, 14, 11), offs=(0, 3, 0), tab=np.arange(5))
        if op in (GET, GET_ADD):
            b.update(ring0=np.ones((4, 8)), pos=[6, 0, 1 << 40], cnt=[4, 0, 3])
        if op in (ADD, ADD2, GET_ADD):
            b.update(ring_a=np.ones((4, 4)), sched_a=[3, -1, 9], gain_a=0.5)
        if op in (ADD2, GET_ADD):
            b.update(ring_b=np.ones((4, 2)), sched_b=[-1, 1, 2], gain_b=1.0)
        return b
    return base


def _mix_base():
    return dict(wet=np.ones((4, 9)), n=8, gains=np.ones((2, 2)), ring=np.ones((4, 8)), pos0=5, d_new=[3, 0], d_old=[7, 1], x_len=[8, 0],
                x_gains=np.ones((2, 8)), ramp_len=[9, 2], ramp_gains=np.ones((2, 10, 2)), ramp_off=1, wet_on=[1, 0],
                old_ring=np.ones((4, 4)), regrow_end=6, ring_in=np.ones((4, 9)), n_put=8)


def _tail_base():
    return dict(T=[3, 1], B=64, layers=[(256, 64, 1), (512, 704, 0)], state=[0, 0, 0, 0], layer_out=np.ones((2, 2, 64)),
                ring=np.ones((2, 2, 32)))


def _rows_base(op):
    def base():
        if op == COPY:
            return dict(op=op, dst=np.ones((3, 12)), n=7, src=np.ones((3, 10)), src_off=3, dst_off=5)
        if op == SCALE:
            return dict(op=op, dst=np.ones((4, 12)), n=7, gain=[1.0, 0.5])
        return dict(op=op, dst=np.ones((4, 12)), n=7, src=np.ones((4, 9)), on=[1, 0], length=[10, 0], g_end=[0.0, 1.0], gains=np.ones((2, 10)))
    return base


REFUSALS = {
    "direct_head": [          # (rule, base, override)
        ("no channel", _head_base, dict(n_ch=0)),
        ("no slot", _head_base, dict(n_slots=0)),
        ("n == 0", _head_base, dict(n=0)),
        ("n above in_stride", _head_base, dict(n=13, out=np.ones((4, 13)))),
        ("33 taps", _head_base, dict(taps=[33, 0, 5])),
        ("negative taps", _head_base, dict(taps=[32, -1, 5])),
        ("slot out of range", _head_base, dict(ir_slot=[3, 0, 0, 1])),
        ("negative slot", _head_base, dict(ir_slot=[2, -1, 0, 1])),
        ("odd channel count with wet_on", _head_base, dict(n_ch=3)),
        ("out_stride below n", _head_base, dict(out_stride=8)),
        ("rows above 2^28 elements", _head_base, dict(in_stride=1 << 27)),
    ],
    "agc": [
        ("op 4", _agc_base(0), dict(op=4)),
        ("no channel", _agc_base(0), dict(n_ch=0)),
        ("B == 0", _agc_base(0), dict(B=0)),
        ("T == 0", _agc_base(0), dict(T=0)),
        ("ch_stride below B * T", _agc_base(0), dict(ch_stride=11)),
        ("B * T above 2^28", _agc_base(0), dict(B=1 << 20, T=1 << 9, ch_stride=1 << 29)),
        ("odd channel count in apply", _agc_base(1), dict(n_ch=3)),
        ("ch_stride below B * T in apply", _agc_base(1), dict(ch_stride=11)),
        ("apply without a state", _agc_base(1), dict(state=None)),
        ("one channel in the ramp", _agc_base(2), dict(n_ch=1)),
        ("ramp ch_stride below B * T", _agc_base(2), dict(B=4)),
        ("odd channel count in the silence test", _agc_base(3), dict(n_ch=3)),
    ],
    "ring_chunks": [
        ("op 5", _chunks_base(GET), dict(op=5)),
        ("no row", _chunks_base(GET), dict(rows=0)),
        ("n == 0", _chunks_base(GET), dict(n=0)),
        ("q == 0", _chunks_base(GET), dict(q=0)),
        ("out_stride below n", _chunks_base(GET), dict(out_stride=10)),
        ("ch_map entry == rows", _chunks_base(GET), dict(ch_map=[2, -1, 6, 0])),
        ("ch_map entry below -1", _chunks_base(GET), dict(ch_map=[2, -2, 5, 0])),
        ("a row named twice", _chunks_base(GET), dict(ch_map=[2, -1, 2, 0])),
        ("ring size not a power of two", _chunks_base(GET), dict(ring0=np.ones((4, 6)))),
        ("ring of one element", _chunks_base(GET), dict(ring0=np.ones((4, 1)))),
        ("cnt above q", _chunks_base(GET), dict(cnt=[5, 0, 3])),
        ("negative cnt", _chunks_base(GET), dict(cnt=[4, -1, 3])),
        ("position above 2^62", _chunks_base(GET), dict(pos=[6, (1 << 62) + 1, 0])),
        ("negative position", _chunks_base(GET), dict(pos=[6, -1, 0])),
        ("no ring", _chunks_base(GET), dict(ring0=None)),
        ("schedule entry above 2^62", _chunks_base(ADD), dict(sched_a=[3, -1, (1 << 62) + 1])),
        ("add ring size not a power of two", _chunks_base(ADD), dict(ring_a=np.ones((4, 12)))),
        ("no schedule", _chunks_base(ADD), dict(sched_a=None)),
        ("two-layer add without ring B", _chunks_base(ADD2), dict(ring_b=None)),
        ("ring B of one element", _chunks_base(ADD2), dict(ring_b=np.ones((4, 1)))),
        ("schedule B above 2^62", _chunks_base(ADD2), dict(sched_b=[-1, (1 << 62) + 1, 2])),
        ("fused: cnt above q", _chunks_base(GET_ADD), dict(cnt=[4, 0, 5])),
        ("fused: ring B without a schedule", _chunks_base(GET_ADD), dict(sched_b=None)),
        ("fused: ring A missing", _chunks_base(GET_ADD), dict(ring_a=None)),
        ("gather: no destination", _chunks_base(GATHER), dict(n_dst=0)),
        ("gather: four destinations", _chunks_base(GATHER), dict(n_dst=4)),
        ("gather: table of 65 entries", _chunks_base(GATHER), dict(tab=np.arange(65))),
        ("gather: negative table length", _chunks_base(GATHER), dict(n_tab=-1)),
        ("gather: window beyond its row", _chunks_base(GATHER), dict(offs=(0, 4, 0))),
        ("gather: negative offset", _chunks_base(GATHER), dict(offs=(-1, 3, 0))),
        ("gather: ch_map entry == rows", _chunks_base(GATHER), dict(ch_map=[2, -1, 6, 0])),
        ("out rows above 2^28 elements", _chunks_base(GET), dict(out_stride=1 << 27)),
        ("gather: destination above 2^28 elements", _chunks_base(GATHER), dict(strides=(12, 1 << 27, 11))),
    ],
    "convproc_mix": [
        ("odd channel count", _mix_base, dict(n_ch=3)),
        ("no channel", _mix_base, dict(n_ch=0)),
        ("negative n", _mix_base, dict(n=-1, x_len=[0, 0])),
        ("n above ch_stride", _mix_base, dict(n=10)),
        ("ring size not a power of two", _mix_base, dict(ring=np.ones((4, 12)))),
        ("ring of one element", _mix_base, dict(ring=np.ones((4, 1)), d_new=[0, 0], d_old=[0, 0], old_ring=None, ring_in=None)),
        ("negative pos0", _mix_base, dict(pos0=-1)),
        ("pos0 above 2^62", _mix_base, dict(pos0=(1 << 62) + 1)),
        ("delay == ring size", _mix_base, dict(d_new=[8, 0])),
        ("negative delay", _mix_base, dict(d_new=[3, -1])),
        ("old delay == ring size", _mix_base, dict(d_old=[7, 8])),
        ("x_len above n", _mix_base, dict(x_len=[9, 0], x_gains=np.ones((2, 9)))),
        ("x_len above x_cap", _mix_base, dict(x_gains=np.ones((2, 7)))),
        ("negative x_len", _mix_base, dict(x_len=[8, -1])),
        ("x_len without gains", _mix_base, dict(x_gains=None)),
        ("ramp_len above ramp_cap", _mix_base, dict(ramp_len=[11, 2])),
        ("negative ramp_off", _mix_base, dict(ramp_off=-1)),
        ("ramp_len without gains", _mix_base, dict(ramp_gains=None)),
        ("regrow into a smaller ring", _mix_base, dict(old_ring=np.ones((4, 16)))),
        ("old ring size not a power of two", _mix_base, dict(old_ring=np.ones((4, 6)))),
        ("negative regrow end", _mix_base, dict(regrow_end=-1)),
        ("put of 0 samples", _mix_base, dict(n_put=0)),
        ("put longer than its rows", _mix_base, dict(n_put=10)),
        ("put longer than the ring", _mix_base, dict(ring_in=np.ones((4, 16)), n_put=9)),
        ("regrow end above 2^62", _mix_base, dict(regrow_end=(1 << 62) + 1)),
        ("x_cap == 0", _mix_base, dict(x_cap=0, x_len=[0, 0])),
        ("ramp_cap == 0", _mix_base, dict(ramp_cap=0, ramp_len=[0, 0], ramp_off=0)),
        ("ring above 2^28 elements", _mix_base, dict(ring_size=1 << 27, old_ring=None, ring_in=None)),
        ("rows above 2^28 elements", _mix_base, dict(ch_stride=1 << 27)),
    ],
    "tail_reader": [
        ("no call", _tail_base, dict(n_calls=0)),
        ("a call of 0 callbacks", _tail_base, dict(T=[3, 0])),
        ("B == 0", _tail_base, dict(B=0)),
        ("partition no multiple of B", _tail_base, dict(layers=[(256, 64, 1), (544, 704, 0)])),
        ("partition below B", _tail_base, dict(layers=[(32, 64, 1), (512, 704, 0)])),
        ("three tail layers", _tail_base, dict(n_tail=3)),
        ("no tail layer", _tail_base, dict(n_tail=0)),
        ("negative output delay", _tail_base, dict(layers=[(256, -1, 1), (512, 704, 0)])),
        ("negative write lag", _tail_base, dict(layers=[(256, 64, -1), (512, 704, 0)])),
        ("negative cursor", _tail_base, dict(state=[0, -1, 0, 0])),
        ("cursor above 2^62", _tail_base, dict(state=[0, 0, (1 << 62) + 1, 0])),
        ("append ring size not a power of two", _tail_base, dict(ring=np.ones((2, 2, 48)))),
        ("append ring of one element", _tail_base, dict(ring=np.ones((2, 2, 1)))),
        ("append without a ring", _tail_base, dict(ring=None)),
        ("4097 calls", _tail_base, dict(T=[1] * 4097)),
        ("more than 2^20 callbacks in all", _tail_base, dict(T=[1 << 19, 1 << 19, 1])),
        ("a call above 2^20 callbacks", _tail_base, dict(T=[3, (1 << 20) + 1])),
        ("append without a channel", _tail_base, dict(n_ch=0)),
        ("append of no sample", _tail_base, dict(n_samples=0)),
        ("append ring above 2^28 elements", _tail_base, dict(ring_size=1 << 27)),
    ],
    "rows": [
        ("op 3", _rows_base(COPY), dict(op=3)),
        ("no channel", _rows_base(COPY), dict(n_ch=0)),
        ("n == 0", _rows_base(COPY), dict(n=0)),
        ("source window beyond its row", _rows_base(COPY), dict(src_off=4)),
        ("destination window beyond its row", _rows_base(COPY), dict(dst_off=6)),
        ("negative source offset", _rows_base(COPY), dict(src_off=-1)),
        ("negative destination offset", _rows_base(COPY), dict(dst_off=-1)),
        ("copy without a source", _rows_base(COPY), dict(src=None)),
        ("scale of an odd channel count", _rows_base(SCALE), dict(n_ch=3)),
        ("scale beyond the row", _rows_base(SCALE), dict(n=13)),
        ("scale without gains", _rows_base(SCALE), dict(gain=None)),
        ("blend beyond the dry row", _rows_base(BLEND), dict(n=10)),
        ("blend len above cap", _rows_base(BLEND), dict(length=[11, 0])),
        ("blend negative len", _rows_base(BLEND), dict(length=[10, -1])),
        ("blend with an offset", _rows_base(BLEND), dict(dst_off=1)),
        ("blend of an odd channel count", _rows_base(BLEND), dict(n_ch=3)),
        ("blend cap == 0", _rows_base(BLEND), dict(cap=0, length=[0, 0])),
        ("rows above 2^28 elements", _rows_base(COPY), dict(dst_stride=1 << 27)),
        ("source rows above 2^28 elements", _rows_base(COPY), dict(src_stride=1 << 27)),
    ],
}

CALLERS = {"direct_head": direct_head, "agc": agc, "ring_chunks": ring_chunks, "convproc_mix": convproc_mix, "tail_reader": tail_reader,
           "rows": rows}
VALID = {"direct_head": [_head_base], "agc": [_agc_base(op) for op in range(4)], "ring_chunks": [_chunks_base(op) for op in range(5)],
         "convproc_mix": [_mix_base], "tail_reader": [_tail_base], "rows": [_rows_base(op) for op in range(3)]}


def walk_refusals(lib):
    """every refusal rule once: [(entry, rule, status)]; the arrays keep the sizes of the valid base unless the override replaces them"""
    return [(kind, rule, CALLERS[kind](lib, **dict(base(), **override))[0]) for kind, rules in REFUSALS.items()
            for rule, base, override in rules]


def valid_calls(lib):
    """the base argument sets themselves: [(entry, status, arguments, outputs)]"""
    res = []
    for kind, bases in VALID.items():
        for base in bases:
            args = base()
            rc, o = CALLERS[kind](lib, **args)
            res.append((kind, rc, args, o))
    return res
