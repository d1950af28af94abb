"""Every input of tests/out_edge_inputs.py does, on the models alone, what its GPU test (test_gpu_out_edges.py) relies on: the
restatement of k_out_pre takes the intended path span by span, the two paths give different bits where a threshold decides, the
restatement stays within half the GPU tests' bar of the long-double model wherever they apply that bar, its tables are the
host's bit for bit, and the limiter inputs stall, attack and poison the envelope where they say.  No GPU.

Where the bar applies.  Signals, sizes and rates of the parity test, the loud-then-quiet input per callback, the quiet calls
after a guarded one, and the long call.  Not the denormal input: there every error is a handful of quanta of 2^-1074 and the
ratio of two such counts says nothing (measured here: 0.3 - 17 x).  In that range sums and differences are exact and only the
products round, by half a quantum each; a section takes one product per sample and fewer than one per sample in its scan, so
the denormal input is held to (2 n + 32) quanta of the long-double run instead -- and bit for bit on the device, like the rest."""
import os
import subprocess

import numpy as np
import pytest

import out_edge_inputs as E
import out_model as M
from test_gpu_output_stage import dc_signals
from test_out_model_cpu import DC_BAR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HALF_BAR = DC_BAR / 2
QUANTUM = 2.0 ** -1074


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def wanted(case, row):
    return case["want"][row] if isinstance(case["want"], dict) else case["want"]


def check_paths(case):
    st = E.KernelStage(case["rate"], case["x"].shape[0])
    y, paths = st.run(case["x"], case["calls"], case["B"], case["flags"])
    for row in range(case["x"].shape[0]):
        got = [p[row] for p in paths]
        if row in case["rows"]:
            assert got == wanted(case, row), (row, got)
        else:
            assert all(q == E.FAST for p in got for q in p), (row, got)
    return y, st


# ----------------------------------------------------------------------------------------------------------- path lists
@pytest.mark.parametrize("rate", E.DC_RATES)
@pytest.mark.parametrize("position", E.THRESHOLD_POSITIONS)
@pytest.mark.parametrize("value", E.THRESHOLD_VALUES)
def test_threshold_inputs_take_their_paths_and_the_paths_differ(value, position, rate):
    c = E.threshold_case(value, position, rate)
    n, at, span = E.THRESHOLD_POSITIONS[position]
    assert at // E.SPAN == span and c["x"].shape == (6, n) and n % 2 == 1
    check_paths(c)
    guarded = [i for i, p in enumerate(c["want"][0]) if p == E.GUARDED]
    assert guarded == ([] if value == "just below 1e14" else [span])
    alpha = M.design(rate)[0]
    for row in c["rows"]:
        yf, sf, pf = E.kernel_dc(c["x"][row], alpha, (0.0, 0.0), c["B"], {span: E.FAST})
        yg, sg, pg = E.kernel_dc(c["x"][row], alpha, (0.0, 0.0), c["B"], {span: E.GUARDED})
        assert pf[span] == E.FAST and pg[span] == E.GUARDED
        differ = int((bits(yf) != bits(yg)).sum())
        print(f"{value} at {position}, {rate:.0f} Hz, row {row}: {differ} samples differ between the paths")
        if position in E.SAME_BITS_ON_BOTH_PATHS:
            assert n - span * E.SPAN <= 8 and differ == 0 and sf == sg       # lane 0 of wave 0 is the sequential form
        else:
            assert differ > 0


@pytest.mark.parametrize("rate", E.CARRIED_RATES)
def test_carried_state_lies_between_the_two_thresholds(rate):
    for flags in (M.DC_BLOCK, M.DC_BLOCK | M.HEADROOM):
        c = E.carried_case(rate, flags)
        check_paths(c)
        st = E.KernelStage(rate, 6)
        st.process(c["x"][:, :512], 512)
        ref = M.OutStage(rate, 3)
        ref.process(c["x"][:, :512], 512, M.DC_BLOCK)
        for row in c["rows"]:
            s0, s1 = st.state[row]
            print(f"{rate:.0f} Hz row {row}: states after the loud callback {s0:.4e}, {s1:.4e}")
            assert 1.0e14 <= abs(s0) < 1.0e15 and abs(s1) < 1.0e15 and list(st.state[row]) == ref.dc[row]    # the reference keeps it
    assert E.GUARDED in c["want"][1] and c["want"][1][0] == E.GUARDED
    # the quiet call's first span is guarded for its carried state alone, and the fast path would give other bits
    quiet = c["x"][:, 512:]
    assert np.abs(quiet).max() < 10.0
    for row in c["rows"]:
        yf, _, _ = E.kernel_dc(quiet[row], st.alpha, st.state[row], 512, {0: E.FAST})
        yg, _, pg = E.kernel_dc(quiet[row], st.alpha, st.state[row], 512)
        assert pg == c["want"][1] and (bits(yf[:E.SPAN]) != bits(yg[:E.SPAN])).any()


def test_long_callback_hands_a_state_of_1e15_or_more_to_the_next_span():
    c = E.long_callback_case()
    y, st = check_paths(c)
    assert all(n == c["B"] for n in c["calls"]) and not c["any"] and c["B"] == 2 * E.SPAN
    assert np.abs(c["x"][:, 100:]).max() < 10.0
    alpha = M.design(c["rate"])[0]
    for row in c["rows"]:
        mid = 0.0
        for v in c["x"][row, :E.SPAN].tolist():                                        # span 0 has no guard at its end
            mid = mid + alpha[0] * (v - mid)
        print(f"row {row}: state entering span 1 {mid:.4e}")
        assert abs(mid) >= 1.0e15
        _, end, _ = E.kernel_dc(c["x"][row, :4096], alpha, (0.0, 0.0), 4096)
        assert end == (0.0, 0.0)                                                        # zeroed at sample 4095
    ref = M.OutStage(c["rate"], 3)
    ref.process(c["x"][:, :4096], 4096, M.DC_BLOCK)
    assert ref.dc[0] == [0.0, 0.0] and ref.dc[3] == [0.0, 0.0]


def test_section1_carry_case_is_guarded_for_section_1_alone():
    c = E.section1_carry_case()
    check_paths(c)
    alpha = M.design(c["rate"])[0]
    assert np.abs(c["x"][:, 2048:]).max() < 10.0
    for row in c["rows"]:
        s0 = s1 = 0.0
        for v in c["x"][row, :E.SPAN].tolist():                                        # span 0 has no guard at its end
            s0 = s0 + alpha[0] * (v - s0)
            v = v - s0
            s1 = s1 + alpha[1] * (v - s1)
        print(f"row {row}: states entering span 1 {s0:.4e}, {s1:.4e}")
        assert abs(s0) < 1.0e3 and 1.0e15 <= abs(s1) < 1.0e16
        assert E.span_is_fast(c["x"][row, E.SPAN:4096], s0, 0.0) and not E.span_is_fast(c["x"][row, E.SPAN:4096], s0, s1)
        yf, _, _ = E.kernel_dc(c["x"][row, :4096], alpha, (0.0, 0.0), 4096, {1: E.FAST})
        yg, _, pg = E.kernel_dc(c["x"][row, :4096], alpha, (0.0, 0.0), 4096)
        assert pg == c["want"][0] and (bits(yf[E.SPAN:]) != bits(yg[E.SPAN:])).any()


def test_part_callback_guard_is_the_one_at_the_call_end():
    c = E.part_callback_case()
    y, st = check_paths(c)
    n = c["calls"][0]
    assert n == 441 + 441 + 100 and n % c["B"] == 100 and c["any"]
    for row in c["rows"]:
        at = int(np.flatnonzero(np.isnan(c["x"][row]))[0])
        assert 2 * 441 <= at < n                                    # in the part callback
        assert np.isnan(y[row, at:n]).all() and np.isfinite(y[row, n:]).all() and np.isfinite(y[row, :at]).all()
    ref = M.OutStage(c["rate"], 3)
    ref.process(c["x"][:, :n], c["B"], M.DC_BLOCK)
    assert ref.dc[0] == [0.0, 0.0] and ref.dc[3] == [0.0, 0.0]


def test_nonfinite_headroom_case_is_scrubbed_clean():
    c = E.nonfinite_headroom_case()
    y, st = check_paths(c)
    assert np.isfinite(y).all()
    ref = M.OutStage(c["rate"], 3).process(c["x"], c["B"], c["flags"])
    at = 2048 + 5
    end = (at // 512 + 1) * 512
    assert not y[0, at:end].any() and y[0, end:].all() and not ref[0, at:end].any()       # NaN to the callback's end, then a zeroed state
    assert y[3, 7] == ref[3, 7] and abs(y[3, 7]) > 1.0e299 and y[4, -1] == 0.0
    # rows whose guarded span is the call's first are the model's bit for bit
    assert np.array_equal(bits(y[3, :512]), bits(ref[3, :512]))


# ------------------------------------------------------------------------------------------------------------------ bar
def held_to_half_bar(label, y, ld, f64, segments=None):
    worst = 0.0
    for a, b in (segments or [(0, y.shape[1])]):
        for ch in range(y.shape[0]):
            err, dist = E.bar_figures(y[ch, a:b], ld[ch, a:b], f64[ch, a:b])
            ratio = err / dist if dist else (0.0 if err == 0.0 else float("inf"))
            print(f"{label} [{a}, {b}) channel {ch}: fp64 model {dist:.3e} from long double, restatement {err:.3e}: {ratio:.2f} x")
            assert err <= HALF_BAR * dist, (label, ch, a, b, err, dist)
            worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("rate", E.DC_RATES)
def test_restatement_within_half_the_bar_sizes(rate):
    worst = 0.0
    for n in E.DC_SIZES:
        x = dc_signals(n)
        ld, f64 = E.model_runs(x, rate, [n], 512)
        y, paths = E.KernelStage(rate, 6).process(x, 512)
        assert all(q == E.FAST for p in paths for q in p)
        worst = max(worst, held_to_half_bar(f"{rate:.0f} Hz n {n}", y, ld, f64))
    print(f"{rate:.0f} Hz: worst ratio {worst:.2f}")


@pytest.mark.parametrize("rate", E.DC_RATES)
def test_restatement_within_half_the_bar_loud_then_quiet(rate):
    x = E.loud_then_quiet_rows()
    assert np.abs(x).max() == 9.9e13 and np.abs(x[:, 512:]).max() < 0.1
    for calls in ([1536], [512, 1024]):
        ld, f64 = E.model_runs(x, rate, calls, 512)
        y, paths = E.KernelStage(rate, 6).run(x, calls, 512)
        assert all(q == E.FAST for call in paths for p in call for q in p)
        held_to_half_bar(f"{rate:.0f} Hz calls {calls}", y, ld, f64, [(0, 512), (512, 1024), (1024, 1536)])


def test_restatement_within_half_the_bar_after_guarded_calls():
    for c in (E.part_callback_case(), E.long_callback_case(), E.section1_carry_case()):
        n0 = c["calls"][0]
        y, _ = E.KernelStage(c["rate"], 6).run(c["x"], c["calls"], c["B"])
        ld, f64 = E.model_runs(c["x"], c["rate"], c["calls"], c["B"])
        held_to_half_bar(f"B {c['B']}, the call after the guarded one", y[:, n0:], ld[:, n0:], f64[:, n0:])


def test_restatement_within_half_the_bar_long_call():
    x = E.long_dc_rows(E.LONG_N)
    assert E.LONG_N == 258 * E.SPAN and E.LONG_N > 2 * E.HEADROOM_GRID and E.LONG_N > E.CLAMP_GRID + E.BATCH
    ld, f64 = E.model_runs(x[:1].repeat(2, axis=0), 48000.0, [E.LONG_N], E.LONG_B)
    y, _, p = E.kernel_dc(x[0], M.design(48000.0)[0], (0.0, 0.0), E.LONG_B)
    assert p == [E.FAST] * 258
    held_to_half_bar("long call", y[None], ld[:1], f64[:1])


@pytest.mark.parametrize("rate", E.DC_RATES)
def test_denormal_input_stays_denormal_and_close(rate):
    for n in (9, 2049, E.N3):
        x = E.denormal_rows(n)
        assert 0.0 < np.abs(x).max() < 2.0 ** -1022 and np.count_nonzero(x) == x.size
        ld, f64 = E.model_runs(x, rate, [n], 512)
        y, paths = E.KernelStage(rate, 6).process(x, 512)
        assert all(q == E.FAST for p in paths for q in p) and np.count_nonzero(y) > 0.9 * y.size
        for ch in range(6):
            err, dist = E.bar_figures(y[ch], ld[ch], f64[ch])
            print(f"{rate:.0f} Hz n {n} channel {ch}: fp64 model {dist / QUANTUM:.0f} quanta from long double, restatement {err / QUANTUM:.0f}")
            assert err <= (2 * n + 32) * QUANTUM


# --------------------------------------------------------------------------------------------------------------- tables
TABLE_RATES = (8000.0, 44100.0, 48000.0, 96000.0, 192000.0, 384000.0)


def test_scan_tables_are_the_hosts_bit_for_bit(tmp_path):
    exe = tmp_path / "out_tables_print"
    csrc = os.path.join(ROOT, "convopeq_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "sanitize", "out_tables_print.cpp"), os.path.join(csrc, "out_design.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)] + [repr(v) for v in TABLE_RATES], capture_output=True, text=True, timeout=60, check=True)
    lines = r.stdout.splitlines()
    print(r.stdout[:600])
    assert len(lines) == 2 * len(TABLE_RATES)
    for i, line in enumerate(lines):
        f = line.split()
        rate, sec = TABLE_RATES[i // 2], i % 2
        assert float(f[0]) == rate and int(f[1]) == sec and len(f) == 2 + 1 + 7 + 64
        host = [float.fromhex(v) for v in f[2:]]
        alpha = M.design(rate)[0][sec]
        pow2, lane = E.scan_tables(alpha)
        assert [v.hex() for v in host] == [v.hex() for v in [alpha] + pow2 + lane.tolist()], (rate, sec)


# -------------------------------------------------------------------------------------------------------------- limiter
def is_fixed_point(env, release):
    return 1.0 + (env - 1.0) * release == env


def test_attack_positions_cover_seams_last_slice_and_short_groups():
    assert E.ATTACK_N == 2 * E.BATCH + 130 and E.ATTACK_N % E.GROUP == 2
    k = [(at % E.BATCH) // E.SLICE for at in E.ATTACK_POSITIONS]
    assert k.count(7) >= 3 and {1791 // E.SLICE, 1792 // E.SLICE} == {6, 7}
    assert {at // E.BATCH for at in E.ATTACK_POSITIONS} == {0, 1, 2}
    for n in E.ATTACK_LAST_N:
        assert (n % E.BATCH) % E.GROUP == 1                        # the attacked sample is alone in the call's last group
    for n, at in [(E.ATTACK_N, at) for at in E.ATTACK_POSITIONS] + [(n, n - 1) for n in E.ATTACK_LAST_N]:
        x = E.attack_rows(n, at)
        d = M.desired_gain(x[0], x[1])
        assert d[at] == M.THRESHOLD / 3.0 and np.count_nonzero(d < 1.0) == 1 and abs(x[at % 2, at]) == 3.0


@pytest.mark.parametrize("rate", E.STALL_CALLS)
def test_stall_rows_rest_on_the_fixed_point_before_the_second_attack(rate):
    x, calls = E.stall_rows(rate)
    _, rel = M.design(rate)
    d = M.desired_gain(x[0], x[1])
    g, _ = M.envelope_run(d, 1.0, rel)
    o = sum(calls[:-1])
    stall = int(np.argmax(g == g[o - 1]))
    fixed = float(g[o - 1])
    print(f"{rate:.0f} Hz: the release stalls after {stall} samples at {fixed!r}; {o} run before the last call")
    assert stall < o - 8192 and fixed < 1.0 and is_fixed_point(fixed, rel) and not is_fixed_point(float(g[stall - 2]), rel)
    assert np.count_nonzero(d[1:o] < 1.0) == 0
    miss, hit = o + E.STALL_NEAR_MISS_AT, o + E.STALL_ATTACK_AT
    assert miss // E.BATCH == hit // E.BATCH and miss // E.GROUP < hit // E.GROUP and (hit % E.BATCH) // E.GROUP == 5
    assert fixed < d[miss] < 1.0 and d[hit] < fixed and fixed - d[hit] < 1.0e-12        # a near miss and a mild attack
    assert np.all(g[o:hit] == fixed) and g[hit] == d[hit] and np.all(g[hit + 1:] > d[hit])
    assert np.all(np.diff(g[hit:]) >= 0.0) and g[-1] == fixed                              # and back onto the fixed point


@pytest.mark.parametrize("at", E.NONFINITE_AT)
@pytest.mark.parametrize("kind", E.NONFINITE_KINDS)
def test_nonfinite_limiter_rows_do_what_the_reference_does(kind, at):
    x, calls = E.nonfinite_limiter_rows(kind, at)
    assert calls[0] == at + 301 and (at // E.BATCH, at % E.BATCH) in ((0, 5), (1, 0))
    for flags in (M.LIMITER, M.LIMITER | M.CLAMP):
        st = M.OutStage(48000.0, 1)
        with np.errstate(invalid="ignore"):                         # inf * 0
            y0 = st.process(x[:, :calls[0]], 512, flags)
            env0 = st.env[0]
            y1 = st.process(x[:, calls[0]:], 512, flags)
        y = np.concatenate([y0, y1], axis=1)
        nan_in = np.isnan(x)
        if kind.startswith("NaN"):
            # a NaN on the left makes the peak NaN and the desired gain 1.0; one on the right alone is dropped by jmax
            assert env0 == 1.0 and st.env[0] == 1.0
            if flags & M.CLAMP:
                assert np.isfinite(y).all() and np.all(y[nan_in] == -M.H)
            else:
                assert np.array_equal(np.isnan(y), nan_in)
            clean = ~nan_in
            assert np.array_equal(bits(y[clean]), bits(M.clamp(x[clean]) if flags & M.CLAMP else x[clean]))
        else:
            # Inf: desired gain 0, envelope 0, and the release climbs from 0: 1 - release after the next sample
            g, _ = M.envelope_run(M.desired_gain(x[0], x[1]), 1.0, st.release)
            assert g[at] == 0.0 and g[at + 1] == 1.0 + (0.0 - 1.0) * st.release and 0.0 < env0 < 0.07 and env0 < st.env[0] < 0.2
            ch = 0 if "left" in kind else 1
            assert (y[ch, at] == -M.H) if flags & M.CLAMP else np.isnan(y[ch, at])            # inf * 0
            assert y[1 - ch, at] == 0.0 and np.isnan(y).sum() == (0 if flags & M.CLAMP else 1)


def test_long_rows_reach_the_second_trip_of_both_grids():
    x = E.long_scrub_rows()
    bad = ~(np.abs(x * M.H) < 1.0e300)
    assert bad[:, :E.HEADROOM_GRID].any() and bad[:, E.HEADROOM_GRID:2 * E.HEADROOM_GRID].any() and bad[:, 2 * E.HEADROOM_GRID:].any()
    y = M.scrub(x * M.H)
    assert np.isfinite(y).all() and (np.abs(y) > 9.9e299).sum() >= 4 and bad.sum() >= 8
    x = E.long_clamp_rows()
    for lo in (E.CLAMP_GRID, E.CLAMP_GRID + E.BATCH):
        seg = x[:, lo:lo + E.BATCH]
        assert (seg > M.H).any() and (seg < -M.H).any()
        assert (seg * M.H > M.H).any() and (seg * M.H < -M.H).any()
    x = E.long_attack_rows()
    d = M.desired_gain(x[0], x[1])
    assert np.flatnonzero(d < 1.0).tolist() == [E.CLAMP_GRID + 1] and (E.CLAMP_GRID + 1) // E.BATCH == 256
