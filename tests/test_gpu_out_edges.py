"""GPU tests of the output stage kernels (convopeq_amd/csrc/out_kernels.hip) at span and batch seams, at the thresholds of
k_out_pre's path choice, with NaN and Inf, and in calls long enough for every loop to loop -- through cpq_out_process, on the
inputs of tests/out_edge_inputs.py, which tests/test_out_edges_cpu.py proves on the models alone.

DC blocker.  The device is held bit for bit to kernel_dc, the restatement of one k_out_pre call: the fast path lane by lane
where the kernel's own test passes, the reference's loop with its guards where it fails.  Which path a span took therefore shows
in the bits (the CPU file shows that the two paths differ on every threshold input but the one whose event lies in a span's
first 8 samples).  Where the CPU file holds the restatement to half the bar, the device is also held to the bar itself (8 x the
fp64 model's distance from the long-double model, tests/test_gpu_output_stage.py); a call whose spans were all guarded since
the reset is the fp64 model's bit for bit.

Limiter and clamp.  Bit for bit against tests/out_model.py, the envelope included.

Measured on an MI355X: see RESULTS.md (worst ratio against the bar, bit equality, wall time per test)."""
import time

import numpy as np
import pytest

import out_edge_inputs as E
import out_model as M
from test_gpu_output_stage import DC_BAR, dc_signals, run_calls, same_bits, same_bits_or_nan, stage_engine

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def first_difference(y, ref):
    """where the device leaves the restatement: (row, sample, span, lane, wave) of the first differing sample of the first
    differing row, for the report the bit equality asks for"""
    na, nb = np.isnan(y), np.isnan(ref)
    diff = (na != nb) | (np.where(na, 0.0, y).view(np.uint64) != np.where(nb, 0.0, ref).view(np.uint64))
    if not diff.any():
        return None
    row = int(np.flatnonzero(diff.any(axis=1))[0])
    at = int(np.flatnonzero(diff[row])[0])
    lane = (at % E.SPAN) // 8
    return dict(row=row, sample=at, span=at // E.SPAN, lane=lane % 64, wave=lane // 64, device=float(y[row, at]),
                restatement=float(ref[row, at]), samples=int(diff.sum()))


def held_to_bar(label, y, ld, f64, segments=None):
    worst = 0.0
    for a, b in (segments or [(0, y.shape[1])]):
        for ch in range(y.shape[0]):
            err, dist = E.bar_figures(y[ch, a:b], ld[ch, a:b], f64[ch, a:b])
            ratio = err / dist if dist else (0.0 if err == 0.0 else float("inf"))
            print(f"{label} [{a}, {b}) channel {ch}: fp64 model {dist:.3e} from long double, kernel {err:.3e}: {ratio:.2f} x (bar {DC_BAR:.0f} x)")
            assert err <= DC_BAR * dist, (label, ch, a, b, err, dist)
            worst = max(worst, ratio)
    return worst


def run_case(amd, c):
    """(device rows, restatement rows, paths) of a DC input"""
    eng = stage_engine(amd, c["x"].shape[0] // 2, c["flags"], B=c["B"], T=c["T"], rate=c["rate"], any_calls=c["any"])
    y = run_calls(eng, c["x"], c["calls"])
    eng.close()
    ref, paths = E.KernelStage(c["rate"], c["x"].shape[0]).run(c["x"], c["calls"], c["B"], c["flags"])
    return y, ref, paths


def assert_restatement_bits(y, ref, label=""):
    d = first_difference(y, ref)
    assert d is None, (label, d)


# -------------------------------------------------------------------------------------------------------- the DC blocker
@pytest.mark.parametrize("rate", E.DC_RATES)
@pytest.mark.parametrize("n", E.DC_SIZES)
def test_dc_sizes_and_rates_bit_for_bit(amd, n, rate):
    x = np.concatenate([dc_signals(n), E.denormal_rows(n)])            # three streams of signals, three of denormals
    eng = stage_engine(amd, 6, M.DC_BLOCK, rate=rate)
    y = eng.out_process(x)
    eng.close()
    ref, paths = E.KernelStage(rate, 12).process(x, 512)
    assert all(q == E.FAST for p in paths for q in p)
    assert_restatement_bits(y, ref, f"n {n} at {rate:.0f} Hz")
    ld, f64 = E.model_runs(x, rate, [n], 512)
    held_to_bar(f"n {n} at {rate:.0f} Hz", y[:6], ld[:6], f64[:6])
    err = float(np.max(np.abs(y[6:].astype(LD) - ld[6:])))
    print(f"denormal rows: {err / 2.0 ** -1074:.0f} quanta from long double")
    assert err <= (2 * n + 32) * 2.0 ** -1074 and (n < 9 or np.count_nonzero(y[6:]) > 0.9 * 6 * n)


@pytest.mark.parametrize("rate", E.DC_RATES)
def test_dc_loud_callback_then_quiet_ones(amd, rate):
    x = E.loud_then_quiet_rows()
    for calls in ([1536], [512, 1024]):
        eng = stage_engine(amd, 3, M.DC_BLOCK, rate=rate)
        y = run_calls(eng, x, calls)
        eng.close()
        ref, _ = E.KernelStage(rate, 6).run(x, calls, 512)
        assert_restatement_bits(y, ref, f"calls {calls}")
        ld, f64 = E.model_runs(x, rate, calls, 512)
        held_to_bar(f"{rate:.0f} Hz calls {calls}", y, ld, f64, [(0, 512), (512, 1024), (1024, 1536)])


@pytest.mark.parametrize("rate", E.DC_RATES)
@pytest.mark.parametrize("position", E.THRESHOLD_POSITIONS)
@pytest.mark.parametrize("value", E.THRESHOLD_VALUES)
def test_dc_sample_threshold(amd, value, position, rate):
    c = E.threshold_case(value, position, rate)
    y, ref, paths = run_case(amd, c)
    assert [paths[0][r] for r in c["rows"]] == [c["want"][0]] * 2
    assert_restatement_bits(y, ref, f"{value} at {position}, {rate:.0f} Hz")
    if c["want"][0][0] == E.GUARDED:                                   # guarded from the reset on: the model's own bits
        model = M.OutStage(rate, 3).process(c["x"], c["B"], c["flags"])
        assert same_bits_or_nan(y[list(c["rows"]), :E.SPAN], model[list(c["rows"]), :E.SPAN])


@pytest.mark.parametrize("flags", (M.DC_BLOCK, M.DC_BLOCK | M.HEADROOM))
@pytest.mark.parametrize("rate", E.CARRIED_RATES)
def test_dc_carried_state_between_the_thresholds(amd, rate, flags):
    c = E.carried_case(rate, flags)
    y, ref, paths = run_case(amd, c)
    assert [p[0] for p in paths] == c["want"] == [p[3] for p in paths]
    assert_restatement_bits(y, ref, f"{rate:.0f} Hz flags {flags}")
    rows, guarded = list(c["rows"]), 512 + E.SPAN * c["want"][1].count(E.GUARDED)
    model = M.OutStage(rate, 3)
    ym = np.concatenate([model.process(c["x"][:, :512], 512, flags), model.process(c["x"][:, 512:], 512, flags)], axis=1)
    assert same_bits_or_nan(y[rows, :guarded], ym[rows, :guarded])
    assert np.abs(y[rows, 512:]).max() > 1.0e12                        # the kept state is what the quiet call puts out


@pytest.mark.parametrize("case", (E.long_callback_case, E.section1_carry_case))
def test_dc_callback_longer_than_a_span(amd, case):
    c = case()
    y, ref, paths = run_case(amd, c)
    assert [p[0] for p in paths] == c["want"]
    assert_restatement_bits(y, ref)
    model = M.OutStage(c["rate"], 3).process(c["x"][:, :4096], 4096, c["flags"])
    assert same_bits_or_nan(y[list(c["rows"]), :4096], model[list(c["rows"])])
    ld, f64 = E.model_runs(c["x"], c["rate"], c["calls"], c["B"])
    held_to_bar("the call after the guarded one", y[:, 4096:], ld[:, 4096:], f64[:, 4096:])


def test_dc_nan_in_a_part_callback(amd):
    c = E.part_callback_case()
    y, ref, paths = run_case(amd, c)
    assert [p[0] for p in paths] == c["want"]
    assert_restatement_bits(y, ref)
    n0 = c["calls"][0]
    model = M.OutStage(c["rate"], 3).process(c["x"][:, :n0], c["B"], c["flags"])
    assert same_bits_or_nan(y[list(c["rows"]), :n0], model[list(c["rows"])])
    assert np.isnan(y[0, 882 + 50:n0]).all() and np.isfinite(y[:, n0:]).all()
    ld, f64 = E.model_runs(c["x"], c["rate"], c["calls"], c["B"])
    held_to_bar("the call after the NaN", y[:, n0:], ld[:, n0:], f64[:, n0:])


def test_dc_inf_and_1e300_through_the_headroom_instance(amd):
    c = E.nonfinite_headroom_case()
    y, ref, paths = run_case(amd, c)
    assert {r: [p[r] for p in paths] for r in c["rows"]} == c["want"]
    assert_restatement_bits(y, ref)
    assert np.isfinite(y).all() and not y[0, 2048 + 5:2560].any() and abs(y[3, 7]) > 1.0e299
    model = M.OutStage(c["rate"], 3).process(c["x"], c["B"], c["flags"])
    assert same_bits(y[3, :E.SPAN], model[3, :E.SPAN])                 # guarded from the reset on


# ---------------------------------------------------------------------------------------------------- limiter and clamp
def limiter_run(amd, x, calls, flags, rate=48000.0):
    """device and model side by side, the envelope compared after every call"""
    eng = stage_engine(amd, 1, flags, rate=rate)
    st = M.OutStage(rate, 1)
    out, ref, envs, o = [], [], [], 0
    with np.errstate(invalid="ignore"):
        for n in calls:
            out.append(eng.out_process(np.ascontiguousarray(x[:, o:o + n])))
            ref.append(st.process(x[:, o:o + n], 512, flags))
            env = eng.out_read_envelope(0)
            assert env == st.env[0], (o, env, st.env[0])
            envs.append(env)
            o += n
    eng.close()
    return np.concatenate(out, axis=1), np.concatenate(ref, axis=1), envs


@pytest.mark.parametrize("n,at", [(E.ATTACK_N, at) for at in E.ATTACK_POSITIONS] + [(n, n - 1) for n in E.ATTACK_LAST_N])
def test_attack_at_batch_seams_last_slice_and_short_groups(amd, n, at):
    x = E.attack_rows(n, at)
    for flags in (M.LIMITER | M.CLAMP, M.HEADROOM | M.LIMITER | M.CLAMP):
        y, ref, envs = limiter_run(amd, x, [n], flags)
        assert same_bits(y, ref) and envs[0] < 1.0
        scale = M.H if flags & M.HEADROOM else 1.0
        assert same_bits(y[:, :at], x[:, :at] * scale) and abs(y[at % 2, at]) < 0.9      # nothing before the attack is touched


def test_attack_on_the_last_sample_releases_in_the_next_calls(amd):
    calls = [2048 + 65, 1, 3000]
    x = E.attack_rows(sum(calls), calls[0] - 1)
    y, ref, envs = limiter_run(amd, x, calls, M.LIMITER | M.CLAMP)
    assert same_bits(y, ref)
    assert envs[0] == M.THRESHOLD / 3.0 and envs[0] < envs[1] < envs[2] < 1.0
    assert envs[1] == 1.0 + (envs[0] - 1.0) * M.design(48000.0)[1]


@pytest.mark.parametrize("rate", E.STALL_CALLS)
def test_stall_then_a_near_miss_and_a_mild_attack(amd, rate):
    x, calls = E.stall_rows(rate)
    y, ref, envs = limiter_run(amd, x, calls, M.LIMITER, rate)
    rel = M.design(rate)[1]
    fixed = envs[-2]
    print(f"{rate:.0f} Hz: fixed point {fixed!r}, envelope after the last call {envs[-1]!r}")
    assert same_bits(y, ref)
    assert fixed < 1.0 and 1.0 + (fixed - 1.0) * rel == fixed and envs[-3] == fixed
    o = sum(calls[:-1])
    hit = o + E.STALL_ATTACK_AT
    assert same_bits(y[:, o:hit], x[:, o:hit] * fixed)                 # up to the attack the call streams at the stalled gain
    assert y[0, hit] == x[0, hit] * (M.THRESHOLD / x[0, hit]) and y[0, hit] != x[0, hit] * fixed


@pytest.mark.parametrize("flags", (M.LIMITER, M.LIMITER | M.CLAMP))
@pytest.mark.parametrize("at", E.NONFINITE_AT)
@pytest.mark.parametrize("kind", E.NONFINITE_KINDS)
def test_nan_and_inf_into_the_limiter(amd, kind, at, flags):
    x, calls = E.nonfinite_limiter_rows(kind, at)
    y, ref, envs = limiter_run(amd, x, calls, flags)
    assert same_bits_or_nan(y, ref)
    if kind.startswith("NaN"):
        assert envs == [1.0, 1.0]
    else:
        assert 0.0 < envs[0] < envs[1] < 0.2
    if flags & M.CLAMP:
        assert np.isfinite(y).all() and np.abs(y).max() <= M.H


# ------------------------------------------------------------------------------------------------------------ long calls
def long_engine(amd, flags):
    return stage_engine(amd, 1, flags, B=E.LONG_B, T=E.LONG_T, any_calls=False)


def test_long_call_headroom_second_trip_of_the_grid(amd):
    x = E.long_scrub_rows()
    eng = long_engine(amd, M.HEADROOM)
    y = eng.out_process(x)
    eng.close()
    assert same_bits(y, M.scrub(x * M.H)) and np.isfinite(y).all() and y[:, E.HEADROOM_GRID:].any()


@pytest.mark.parametrize("flags", (M.CLAMP, M.HEADROOM | M.CLAMP))
def test_long_call_clamp_batch_257(amd, flags):
    x = E.long_clamp_rows()
    eng = long_engine(amd, flags)
    y = eng.out_process(x)
    eng.close()
    ref = M.OutStage(48000.0, 1).process(x, E.LONG_B, flags)
    assert same_bits(y, ref) and np.abs(y).max() == M.H and (np.abs(y[:, E.CLAMP_GRID:]) == M.H).sum() >= 8


def test_long_call_limiter_attack_in_batch_257(amd):
    x = E.long_attack_rows()
    eng = long_engine(amd, M.LIMITER | M.CLAMP)
    y = eng.out_process(x)
    env = eng.out_read_envelope(0)
    eng.close()
    st = M.OutStage(48000.0, 1)
    ref = st.process(x, E.LONG_B, M.LIMITER | M.CLAMP)
    at = E.CLAMP_GRID + 1
    assert same_bits(y, ref) and env == st.env[0] < 1.0
    assert same_bits(y[:, :at], x[:, :at]) and abs(y[1, at]) == 3.0 * (M.THRESHOLD / 3.0)


def test_long_call_dc_blocker_258_spans(amd):
    """The long-double yardstick is a Python loop: it runs on one channel (0.6 s here); the restatement is vectorised per span
    and covers both."""
    x = E.long_dc_rows(E.LONG_N)
    eng = long_engine(amd, M.DC_BLOCK)
    y = eng.out_process(x)
    eng.close()
    t0 = time.perf_counter()
    ref, paths = E.KernelStage(48000.0, 2).process(x, E.LONG_B)
    assert paths == [[E.FAST] * 258] * 2
    assert_restatement_bits(y, ref)
    ld, f64 = E.model_runs(x[:1].repeat(2, axis=0), 48000.0, [E.LONG_N], E.LONG_B)
    print(f"model side: {time.perf_counter() - t0:.2f} s")
    held_to_bar("long call", y[:1], ld[:1], f64[:1])
