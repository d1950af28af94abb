"""CPU tests of the meters' host side (no GPU): the K-weighting design and the true-peak stage design behind the C ABI
against tests/meter_model.py, the model against BS.1770-4 Table 1 and scipy, and the reference's zero future at callback
ends, which the model states and the kernels reproduce."""
import ctypes as C

import numpy as np
import pytest

import meter_model as M

RATES = (44100.0, 48000.0, 88200.0, 96000.0, 192000.0, 384000.0)


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("rate", RATES)
def test_kweighting_equals_model(amd, rate):
    """Same operation order on both sides: bit for bit.  Measured: 0 ulp at all six rates (Python's math and the library
    call the same libm here).  Only where they are not equal -- another libm, whose cos / sin / pow may differ in the last
    ulp -- the slack applies: an ulp of cos(w0) or sin(w0) moves each a0-normalised coefficient, all ratios of O(1) sums, by a
    few ulp at most: 4."""
    pre, rlb = amd.meter_kweighting(rate)
    mp, mr = M.kweighting(rate)
    if np.array_equal(pre, mp) and np.array_equal(rlb, mr):
        return
    worst = float(max(ulps(pre, mp).max(), ulps(rlb, mr).max()))
    print(f"rate {rate}: worst difference {worst} ulp")
    assert worst <= 4.0


def test_kweighting_against_bs1770_table_1(amd):
    """ITU-R BS.1770-4 Table 1 (48 kHz).  The table's filters were not designed with the cookbook formulas the reference uses
    (1500 Hz / +4 dB / Q 0.7071 and 38 Hz / Q 0.5 are the commonly quoted approximations of it), so the two agree only roughly.
    Measured worst relative difference per coefficient: pre-filter 4.0e-5, RLB denominator 2.9e-5.  The RLB numerator of the
    table is exactly 1, -2, 1; the cookbook high-pass has the same shape scaled by (1 + cos w0) / (2 a0) = 0.99504.
    Bar: 1e-4 relative.  A design with every corner frequency 1 % off moves the pre-filter by 3.1e-3 and the RLB denominator
    by 9.9e-5 on top of the 2.9e-5 (it sits at 0.99 of its limit 2, 1: insensitive), so the pre-filter bar tells a right
    design from a wrong one and the RLB bar is at the size of a 1 % error."""
    pre_t = np.array([1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585])
    rlb_t = np.array([1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621])
    for who, (pre, rlb) in (("library", amd.meter_kweighting(48000.0)), ("model", M.kweighting(48000.0))):
        d_pre = float(np.max(np.abs(pre - pre_t) / np.abs(pre_t)))
        d_den = float(np.max(np.abs(rlb[3:] - rlb_t[3:]) / np.abs(rlb_t[3:])))
        d_shape = float(np.max(np.abs(rlb[:3] / rlb[0] - rlb_t[:3])))
        print(f"{who}: pre {d_pre:.3e}  rlb denominator {d_den:.3e}  rlb numerator shape {d_shape:.3e}  rlb b0 {rlb[0]!r}")
        assert d_pre <= 1e-4, who
        assert d_den <= 1e-4, who
        assert d_shape <= 1e-15, who
        assert abs(rlb[0] - 1.0) <= 1e-2, who   # the cookbook high-pass carries its pass-band gain in b0: 1 / a0 (1 + cos) / 2


@pytest.mark.parametrize("stage", (0, 1))
def test_tp_design_stage_equals_model(amd, stage):
    info, taps = amd.meter_tp_design_stage(stage)
    m = M.tp_stages()[stage]
    want = {0: dict(taps=63, center_tap=31, center_parity=1, conv_parity=0, conv_count=32, center_delay_input=15, history_up_keep=31),
            1: dict(taps=31, center_tap=15, center_parity=1, conv_parity=0, conv_count=16, center_delay_input=7, history_up_keep=15)}[stage]
    for k, v in want.items():
        assert info[k] == v == m[k], k
    assert info["attenuation_db"] == 100.0 and info["center_coeff"] == 0.5
    assert len(taps) == m["taps"]
    assert float(ulps(taps, m["raw"]).max()) <= 1.0
    assert taps[m["center_tap"]] == 0.5
    assert abs(taps.sum() - 1.0) < 1e-15


def test_invalid_arguments_without_a_gpu(amd):
    from convopeq_amd import _capi as K
    lib = K.load()
    a, b = np.zeros(5), np.zeros(5)
    pa, pb = a.ctypes.data_as(K.c_double_p), b.ctypes.data_as(K.c_double_p)
    for rate in (0.0, -48000.0, float("nan"), float("inf")):
        assert lib.cpq_meter_kweighting(rate, pa, pb) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_meter_kweighting(48000.0, None, pb) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_meter_kweighting(48000.0, pa, None) == K.CPQ_ERR_INVALID_ARG
    for stage in (-1, 2):
        assert lib.cpq_meter_tp_design_stage(stage, None, None, 0) == K.CPQ_ERR_INVALID_ARG
    t = np.zeros(63)
    assert lib.cpq_meter_tp_design_stage(0, None, t.ctypes.data_as(K.c_double_p), 62) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_meter_tp_design_stage(0, None, t.ctypes.data_as(K.c_double_p), 63) == 63
    # entry points that need an engine refuse a null handle before touching a device
    assert lib.cpq_engine_set_metering(None, 3) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_meter_reset(None) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_meter_process(None, pa, 5) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_meter_process_device(None, None, 5) == K.CPQ_ERR_INVALID_ARG
    n = C.c_int32()
    assert lib.cpq_meter_read_blocks(None, None, 0, C.byref(n), None) == K.CPQ_ERR_INVALID_ARG
    assert lib.cpq_kernel_name(9) == b"k_meter"
    assert K.KERNEL_IDS["k_meter"] == 9 and C.sizeof(K.MeterBlock) == 40


def test_model_kweighting_equals_lfilter():
    """The sequential Direct Form I of the model against scipy's (transposed Direct Form II) with the same coefficients:
    the same filter, different rounding.  Noise at 0.25 rms over 3 callbacks of 4800; the RLB section's poles (radius 0.995)
    amplify rounding by about 1 / (1 - r)^2 = 4e4, so 1e-10 of the peak is ample and still 1e6 below any design error."""
    from scipy.signal import lfilter
    rng = np.random.default_rng(3)
    x = 0.25 * rng.standard_normal((2, 3 * 4800))
    pre, rlb = M.kweighting(48000.0)
    m = M.LoudnessMeter(48000.0)
    y = np.concatenate([m.weighted(x[:, o:o + 4800]) for o in range(0, x.shape[1], 4800)], axis=1)
    ref = x
    for c in (pre, rlb):
        ref = lfilter(c[:3], np.concatenate([[1.0], c[3:]]), ref, axis=1)
    err = float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))
    print(f"model vs lfilter: {err:.3e} of the peak")
    assert err <= 1e-10
    # the records: mean square of both channels with weights 1.0, peak over both, the counter
    m.reset()
    recs = m.process(x, 4800)
    assert [r[2] for r in recs] == [0, 1, 2]
    k = 1
    seg = ref[:, k * 4800:(k + 1) * 4800]
    assert abs(recs[k][0][0] - (seg ** 2).sum() / 4800) <= 1e-9 * recs[k][0][0]
    assert abs(recs[k][1][0] - np.abs(seg).max()) <= 1e-9


def test_zero_future_at_callback_ends():
    """interpolateStage sees zeros where the next callback's samples will be: against a continuous evaluation (the next 16
    samples in place of the pad) stage 0 is bit-equal up to input sample N - 17 and differs within the last 16."""
    rng = np.random.default_rng(9)
    N = 256
    x = rng.standard_normal(2 * N)
    st = M.tp_stages()[0]
    hist = rng.standard_normal(st["history_up_keep"])
    cut, _, _, _ = M.interpolate(st, hist, x[:N], dtype=np.float64)
    cont, _, _, _ = M.interpolate(st, hist, x[:N], future=x[N:N + 16], dtype=np.float64)
    assert np.array_equal(cut[:2 * (N - 16)], cont[:2 * (N - 16)])
    assert np.all(cut[2 * (N - 15):] != cont[2 * (N - 15):])         # every later window holds at least one future sample
    assert cut[2 * (N - 16)] != cont[2 * (N - 16)]                    # the even branch reaches one sample further
    # and the history the next callback starts from is the input, not a function of the pad
    _, keep, _, _ = M.interpolate(st, hist, x[:N], dtype=np.float64)
    assert np.array_equal(keep, x[N - st["history_up_keep"]:N])
    # a step in the last 16 samples reads as a 4-sample pulse: another peak than the continuing step's
    s = np.zeros(N)
    s[N - 4:] = 1.0
    a, _, _, _ = M.interpolate(st, np.zeros(31), s, dtype=np.float64)
    b, _, _, _ = M.interpolate(st, np.zeros(31), s, future=np.ones(16), dtype=np.float64)
    assert np.abs(a).max() != np.abs(b).max()


def test_ring_drops_the_newest():
    r = M.Ring()
    pushed = [r.push(i) for i in range(M.RING + 5)]
    assert pushed == [True] * M.RING + [False] * 5
    assert [r.pop() for _ in range(3)] == [0, 1, 2]
    assert r.push(-1) and r.w - r.r == M.RING - 2
