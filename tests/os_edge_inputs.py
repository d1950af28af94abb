"""Inputs of the oversampler edge tests, shared by the CPU checks (test_os_exact_cpu.py: the model against the exact
reference, and every guard / flush / silence decision determined) and the GPU tests (test_gpu_oversampling_edges.py).

A scenario is (name, factor, type, ops) with ops a list of ("up" | "down", x [2, n]) run on one stereo stream from a
fresh state.  What each scenario must construct (an output at exactly 2^53, a stage that takes the silence path, ...) is
asserted on the CPU in test_os_exact_cpu.py."""
import numpy as np

import os_model as M

D = M.DENORM
LIMIT = 2.0 ** 53
PAIRS = [(F, T) for F in (2, 4, 8) for T in (M.IIR, M.LINEAR_PHASE)]


def up_stage(F):
    """index of the stage the down path starts with (the last up stage)"""
    return {2: 0, 4: 1, 8: 2}[F]


def find_amp(c, target, avoid=None):
    """(r, a) with fl(c[r] * a) == target exactly, searching ulp neighbours of target / c[r], largest |c_r| first
    (r != avoid: at the interpolator, output r of an impulse has the impulse itself as its centre when r is cdi)"""
    for r in np.argsort(-np.abs(c), kind="stable"):
        if r == avoid:
            continue
        a = target / c[r]
        for _ in range(2):
            cand = [a]
            lo = hi = a
            for _ in range(8):
                lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
                cand += [lo, hi]
            for v in cand:
                if c[r] * v == target:
                    return int(r), float(v)
    raise AssertionError(f"no amplitude gives {target!r}")


def _z(n):
    return np.zeros((2, n))


# ---- impulses: every output a single rounded product, an exact centre, or one rounding of cen + product (E = 0)
def impulse_scenarios():
    out = []
    for T in (M.IIR, M.LINEAR_PHASE):
        st = M.design_stage(0, T)
        c, C, ct, cdi = st["conv"], st["conv_count"], st["center_tap"], st["center_delay_input"]
        n = 3 * C + 64                                    # impulses at C + 10: the halo of every output is in the call
        k = C + 10
        # interpolator centre 0.5 a at 2^53 (passes) and one ulp above (bad): both signs
        x1, x2 = _z(n), _z(n)
        x1[0, k], x1[1, k] = 2.0 ** 54, -2.0 ** 54
        x2[0, k], x2[1, k] = np.nextafter(2.0 ** 54, np.inf), -np.nextafter(2.0 ** 54, np.inf)
        out.append((f"up_centre_2p53_T{T}", 2, T, [("up", x1), ("down", _z(2 * n)), ("up", x2), ("down", _z(2 * n)),
                                                   ("up", _z(n))]))
        # interpolator convolution product fl(c_r a) at 1e-20 (kept, doubled) and one ulp below (flushed at :125);
        # centre 0.5 a at 1e-20 (a = 2e-20, kept) and one ulp below (flushed at :134)
        _, a_eq = find_amp(c, D, cdi)
        _, a_lo = find_amp(c, np.nextafter(D, 0.0), cdi)
        x = _z(n)
        x[0, k], x[1, k] = a_eq, -a_lo
        y = _z(n)
        y[0, k], y[1, k] = 2 * D, -np.nextafter(2 * D, 0.0)
        out.append((f"up_flush_1e-20_T{T}", 2, T, [("up", x), ("up", y), ("up", _z(n))]))
        # interpolator convolution sum at 2^53 (passes unflagged, doubled to 2^54) and one ulp above (zeroed, no flag);
        # the centre of the same impulse is bad (|c_r| < 0.32), which is an event at another output
        _, a_eq = find_amp(c, LIMIT, cdi)
        _, a_hi = find_amp(c, np.nextafter(LIMIT, np.inf), cdi)
        x = _z(n)
        x[0, k], x[1, k] = a_eq, -a_hi
        out.append((f"up_conv_2p53_T{T}", 2, T, [("up", x), ("down", _z(2 * n)), ("up", _z(n))]))
        # decimator (F = 2, 2n samples in): odd index = centre only, even index = single products
        m = 2 * n
        no = 2 * C + 20                                   # an output index whose window and centre are in the call
        kc = 2 * no - ct                                  # its centre sample (odd)
        assert kc % 2 == 1 and kc > 0 and 2 * no - 2 * (C - 1) > 0 and m - 2 * no > st["history_down_keep"]
        d1, d2 = _z(m), _z(m)
        d1[0, kc], d1[1, kc] = 2.0 ** 54, -2.0 ** 54
        d2[0, kc], d2[1, kc] = np.nextafter(2.0 ** 54, np.inf), -np.nextafter(2.0 ** 54, np.inf)
        out.append((f"down_centre_2p53_T{T}", 2, T, [("down", d1), ("down", d2), ("down", d1), ("down", _z(m))]))
        # cen + dot at 2^53 - 1 (passes), 2^53 (passes) and 2^53 + 2 (bad): cen = 2^53 - 2, one product of 1, 2 or 4
        ops = []
        for p in (1.0, 2.0, 4.0):
            r, a = find_amp(c, p)
            d = _z(m)
            for ch, s in ((0, 1.0), (1, -1.0)):
                d[ch, kc] = s * (2.0 ** 54 - 4.0)
                d[ch, 2 * no - 2 * r] = s * a
            ops += [("down", d), ("down", _z(m))]
        out.append((f"down_sum_2p53_T{T}", 2, T, ops))
        # a lone even-index product one ulp above 2^53 (bad) and at 2^53 (passes)
        _, a_hi = find_amp(c, np.nextafter(LIMIT, np.inf))
        _, a_eq = find_amp(c, LIMIT)
        d = _z(m)
        d[0, 2 * no], d[1, 2 * no] = a_hi, -a_eq
        out.append((f"down_product_2p53_T{T}", 2, T, [("down", d), ("down", _z(m)), ("down", _z(m))]))
        # decimator product at 1e-20 (kept) and one ulp below (flushed at :191); centre at 1e-20 and one ulp below
        _, a_eq = find_amp(c, D)
        _, a_lo = find_amp(c, np.nextafter(D, 0.0))
        d = _z(m)
        d[0, 2 * no], d[1, 2 * no] = a_eq, -a_lo
        e = _z(m)
        e[0, kc], e[1, kc] = 2 * D, -np.nextafter(2 * D, 0.0)
        out.append((f"down_flush_1e-20_T{T}", 2, T, [("down", d), ("down", e)]))
    return out


# ---- silence boundaries
def _tiny(rng, n):
    return rng.uniform(-1e-18, 1e-18, (2, n))


def silence_scenarios():
    out = []
    rng = np.random.default_rng(31)
    for F, T in PAIRS:
        nb = 700
        m = nb * F
        # a block whose largest |v| is exactly 1e-20 takes the silence path (zeros, history zeroed); one ulp above is
        # computed (channel 0 only), so the next call differs by the history it left
        for tag, top in (("eq", D), ("above", np.nextafter(D, np.inf))):
            b = rng.uniform(-D, D, (2, m))
            b[:, 17] = D
            b[:, m - 3] = -D
            b[0, m // 2] = top
            out.append((f"block_max_{tag}_F{F}_T{T}", F, T, [("down", b), ("down", _tiny(rng, m))]))
        # the history side: the previous call's tail (longer than any history) at 1e-20, then a silent block
        for tag, top in (("eq", D), ("above", np.nextafter(D, np.inf))):
            a = _tiny(rng, m)
            tail = 1100
            a[:, m - tail:] = rng.uniform(-D, D, (2, tail))
            a[:, m - tail + 5] = D
            a[0, m - 4] = top                             # inside every history (the shortest keeps 36)
            out.append((f"history_max_{tag}_F{F}_T{T}", F, T,
                        [("down", a), ("down", _z(m)), ("down", _tiny(rng, m))]))
        # a NaN-only block on a silent history: zeros, no event (fabs(NaN) > t is false)
        nan = np.full((2, m), np.nan)
        out.append((f"nan_block_F{F}_T{T}", F, T, [("down", nan), ("down", _tiny(rng, m))]))
        if F > 2:
            # an odd-index impulse of 2e-20 makes the top stage output exactly 1e-20: the stage below is silent;
            # channel 1 gets one ulp more and is computed
            st = M.design_stage(up_stage(F), T)
            k = 2 * (st["conv_count"] + 40) - st["center_tap"]
            b = _z(m)
            b[0, k] = 2 * D
            b[1, k] = np.nextafter(2 * D, np.inf)
            out.append((f"stage_below_silent_F{F}_T{T}", F, T, [("down", b), ("down", _tiny(rng, m))]))
    return out


# ---- large magnitudes through 2 and 3 stages
def _big(rng, shape):
    return rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.uniform(50.0, 53.0, shape)


def matched_run(c, amp_target=1.5 * 2.0 ** 52):
    """operands sign(c_r) A, latest first: the window's sum is A sum|c|; A = 2^52 where sum|c| > 1"""
    s = float(np.abs(c).sum())
    A = 2.0 ** 52 if s > 1.0 else amp_target / s
    assert A <= LIMIT
    return np.sign(c)[::-1] * A


def large_scenarios():
    out = []
    rng = np.random.default_rng(53)
    for F in (4, 8):
        for T in (M.IIR, M.LINEAR_PHASE):
            nb = 1500
            c0 = M.design_stage(0, T)["conv"]
            ctop = M.design_stage(up_stage(F), T)["conv"]
            x1, x2 = _big(rng, (2, nb)), _big(rng, (2, nb))
            run = matched_run(c0)
            x2[0, 200:200 + len(run)] = run
            x2[1, 300:300 + len(run)] = -run
            y1 = _big(rng, (2, nb * F))
            y2 = _big(rng, (2, nb * F))
            drun = matched_run(ctop)                       # on the even phase of the top decimator stage
            y2[0, 600:600 + 2 * len(drun):2] = drun
            y2[1, 900:900 + 2 * len(drun):2] = -drun
            out.append((f"large_F{F}_T{T}", F, T, [("up", x1), ("down", y1), ("up", x2), ("down", y2),
                                                   ("down", _big(rng, (2, nb * F))), ("up", x1)]))
    return out


# ---- tile and lane edges: kOsTile = 2048 outputs per workgroup, 8 per lane
def tile_counts(F):
    n = [2047, 2048, 2049]
    if F >= 4:
        n += [1023, 1025]
    if F >= 8:
        n += [511, 513]
    n += [8 * k + k for k in range(1, 8)]                 # 9, 18, ..., 63: n mod 8 = 1..7
    n += [1, 5, 100, 509]                                 # below C - 1 = 511 (LinearPhase stage 0): halo from history
    return n


def tile_scenarios():
    out = []
    rng = np.random.default_rng(71)
    for F, T in PAIRS:
        ops = []
        for nb in tile_counts(F):
            ops += [("up", rng.uniform(-1.0, 1.0, (2, nb))), ("down", rng.uniform(-1.0, 1.0, (2, nb * F)))]
        out.append((f"tiles_F{F}_T{T}", F, T, ops))
    return out


# ---- state: several up calls, then down calls of other lengths (the up and down histories advance independently)
def state_scenarios():
    rng = np.random.default_rng(97)
    out = []
    for F, T in ((4, M.LINEAR_PHASE), (8, M.IIR)):
        u = lambda n: ("up", rng.uniform(-1.0, 1.0, (2, n)))                 # noqa: E731
        d = lambda n: ("down", rng.uniform(-1.0, 1.0, (2, n * F)))           # noqa: E731
        out.append((f"lengths_F{F}_T{T}", F, T, [u(300), u(200), u(700), d(500), u(100), d(900), d(37), u(1200)]))
    return out


def all_scenarios():
    return impulse_scenarios() + silence_scenarios() + large_scenarios() + tile_scenarios() + state_scenarios()


def scenario(name):
    for s in all_scenarios():
        if s[0] == name:
            return s
    raise KeyError(name)
