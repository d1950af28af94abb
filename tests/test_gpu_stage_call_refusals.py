"""Every refusal of the base-rate stage entry points, pinned by status code and by the text cpq_last_error keeps:
cpq_os_up / cpq_os_down, cpq_out_process, cpq_dither_process, cpq_meter_process and their _device variants.

The expected codes are the table EXPECTED below, written down from the order of the checks in convopeq_amd/csrc (null handle,
stage off, null buffer, 1..maxCall / factor, whole callbacks outside CPQ_CALLS_ANY, 16-byte alignment, then the meters' own
true-peak rules); nothing here asks the library what it would answer.  Every refusal happens on the host before anything is
enqueued, so the smallest engines show all of them: 2 streams, block_size 64, 4 blocks per call, whole-block and CPQ_CALLS_ANY,
at oversampling factors 1 and 2.  No bad pointer reaches a launch: a null or misaligned buffer is refused whatever else the
call holds.  The calls the table marks OK (a callback less one sample where ragged calls are allowed, and at any engine for
the oversampler, whose entry points have no whole-callback rule) run on valid buffers.

That the refusals move no state: after every case the stage is reset and a good call of 64 samples runs.  A twin engine makes
the same resets and good calls and, of the cases, only the accepted ones; the two engines' good calls must agree bit for bit,
one by one (the meters: their records).  Where the stage's reset restores everything the stage carries -- oversampler, output
stage, meters -- every good call must also equal the first one.  cpq_dither_reset clears the error taps and, like the
reference's reset(), leaves the generator words where they are, so the dither stage's good calls differ from one another and
are held to the twin alone."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, NOT_READY = 0, -1, -5, -6
S, B, T, GOOD = 2, 64, 4, 64
NCH, MAX_CALL = 2 * S, B * T
ROW_CAP = MAX_CALL + 8                      # doubles per channel in every buffer: the longest accepted call and to spare

# stage -> column of EXPECTED
STAGES = ("os_up", "os_down", "out", "dither", "meter", "meter_tp")
ENTRY = {"os_up": "cpq_os_up", "os_down": "cpq_os_down", "out": "cpq_out_process", "dither": "cpq_dither_process",
         "meter": "cpq_meter_process", "meter_tp": "cpq_meter_process"}
COLUMN = {"os_up": 0, "os_down": 0, "out": 1, "dither": 1, "meter": 2, "meter_tp": 3}
RESETS_ALL = ("os_up", "os_down", "out", "meter", "meter_tp")       # the stage's reset restores everything it carries
OFF_TEXT = {"os_up": "oversampling is not set", "os_down": "oversampling is not set", "out": "the output stage is off",
            "dither": "dither is off", "meter": "metering is off", "meter_tp": "metering is off"}

# case -> (status of the oversampler's calls, output stage / dither, meters with loudness alone, meters with true peak),
# the stage on; None: the entry point has no such argument.  "short" is one sample less than a callback (block_size / factor).
#                           os          out/dither  loudness    true peak
EXPECTED = {
    "null_handle":         (INVALID,    INVALID,    INVALID,    INVALID),
    "null_in":             (INVALID,    INVALID,    INVALID,    INVALID),
    "null_out":            (INVALID,    INVALID,    None,       None),
    "n_zero":              (INVALID,    INVALID,    INVALID,    INVALID),
    "n_over":              (INVALID,    INVALID,    INVALID,    INVALID),
    "short_whole_blocks":  (OK,         INVALID,    INVALID,    INVALID),        # on the whole-block engine
    "short_any":           (OK,         OK,         OK,         UNSUPPORTED),    # on the CPQ_CALLS_ANY engine
    "in_plus_8":           (INVALID,    INVALID,    INVALID,    INVALID),
    "out_plus_8":          (INVALID,    INVALID,    None,       None),
    "short_in_plus_8":     (INVALID,    INVALID,    INVALID,    INVALID),        # alignment is looked at before true peak's rules
}
# what cpq_last_error holds after the refusal ({limit}: maxCall / factor, {cb}: the callback length)
TEXT = {
    "null_in": "null buffer", "null_out": "null buffer", "n_zero": "outside 1..{limit}", "n_over": "outside 1..{limit}",
    "short_whole_blocks": "not a multiple of the callback length {cb}", "short_any": "true-peak metering needs whole callbacks",
    "in_plus_8": "16-byte aligned", "out_plus_8": "16-byte aligned",
}


@pytest.fixture(scope="module")
def amd():
    import convopeq_amd
    return convopeq_amd


def aligned_rows(count):
    raw = np.zeros(count + 2)
    return raw[(-(raw.ctypes.data // 8)) % 2:][:count]


class Rig:
    """one engine with its host and device buffers; call() hands raw addresses to an entry point and returns the status"""

    def __init__(self, amd, any_calls, factor):
        import torch
        self.torch, self.amd, self.any_calls, self.F = torch, amd, any_calls, factor
        self.eng = amd.BatchedEngine(S, block_size=B, max_ir_len=B, max_blocks_per_call=T,
                                     call_mode=amd.CPQ_CALLS_ANY if any_calls else amd.CPQ_CALLS_WHOLE_BLOCKS)
        if factor > 1:
            self.eng.set_oversampling(factor)
        self.lib, self.h = self.eng._lib, self.eng._h
        self.cb, self.limit = B // factor, MAX_CALL // factor
        self.h_in, self.h_out = aligned_rows(NCH * ROW_CAP), aligned_rows(NCH * ROW_CAP)
        self.d_in = torch.zeros(NCH * ROW_CAP + 2, dtype=torch.float64, device="cuda")
        self.d_out = torch.zeros(NCH * ROW_CAP + 2, dtype=torch.float64, device="cuda")
        assert self.d_in.data_ptr() % 16 == 0 and self.d_out.data_ptr() % 16 == 0
        rng = np.random.default_rng(11)
        self.x = {n: rng.uniform(-0.9, 0.9, NCH * n) for n in (GOOD, GOOD * factor)}

    def stages_on(self):
        K = self.amd
        self.eng.set_output_stage(K.CPQ_OUT_ALL)
        self.eng.set_dither(K.CPQ_DITHER_FIXED4, 16)

    def select(self, stage):
        K = self.amd
        if stage.startswith("meter"):
            self.eng.set_metering(K.CPQ_METER_LOUDNESS | (K.CPQ_METER_TRUE_PEAK if stage == "meter_tp" else 0))

    def lens(self, stage, n):
        """doubles per channel the call reads and writes"""
        return (n * self.F if stage == "os_down" else n), (n * self.F if stage == "os_up" else 0 if stage.startswith("meter") else n)

    def call(self, stage, device, handle, p_in, p_out, n):
        fn = getattr(self.lib, ENTRY[stage] + ("_device" if device else ""))
        ptr = (lambda a: None if a is None else C.c_void_p(a)) if device else \
              (lambda a: None if a is None else C.cast(C.c_void_p(a), C.POINTER(C.c_double)))
        args = [handle, ptr(p_in)] + ([] if stage.startswith("meter") else [ptr(p_out)]) + [n]
        if device:
            self.torch.cuda.synchronize()
        return fn(*args)

    def bufs(self, device):
        return (self.d_in.data_ptr(), self.d_out.data_ptr()) if device else (self.h_in.ctypes.data, self.h_out.ctypes.data)

    def case(self, stage, device, case):
        """the arguments of one case: (handle, in, out, n)"""
        p_in, p_out = self.bufs(device)
        short = self.cb - 1
        return {
            "null_handle": (None, p_in, p_out, GOOD), "null_in": (self.h, None, p_out, GOOD), "null_out": (self.h, p_in, None, GOOD),
            "n_zero": (self.h, p_in, p_out, 0), "n_over": (self.h, p_in, p_out, self.limit + 1),
            "short_whole_blocks": (self.h, p_in, p_out, short), "short_any": (self.h, p_in, p_out, short),
            "in_plus_8": (self.h, p_in + 8, p_out, GOOD), "out_plus_8": (self.h, p_in, p_out + 8, GOOD),
            "short_in_plus_8": (self.h, p_in + 8, p_out, short),
        }[case]

    def reset(self, stage):
        {"os_up": self.eng.os_reset, "os_down": self.eng.os_reset, "out": self.eng.out_reset, "dither": self.eng.dither_reset,
         "meter": self.eng.meter_reset, "meter_tp": self.eng.meter_reset}[stage]()

    def good(self, stage, device):
        """64 samples through the stage: status and what the call delivered, as bytes"""
        n_in, n_out = self.lens(stage, GOOD)
        x = self.x[n_in]
        if device:
            self.d_in[:x.size].copy_(self.torch.from_numpy(x))
            self.d_out.zero_()
        else:
            self.h_in[:x.size] = x
            self.h_out[:] = 0.0
        rc = self.call(stage, device, self.h, *self.bufs(device), GOOD)
        self.eng.synchronize()
        if stage.startswith("meter"):
            rec, dropped = self.eng.meter_read_blocks()
            assert rec.shape == (S, GOOD // self.cb) and dropped == 0
            return rc, rec.tobytes()
        got = self.d_out[:NCH * n_out].cpu().numpy() if device else self.h_out[:NCH * n_out]
        return rc, got.tobytes()

    def close(self):
        self.eng.close()


def cases_of(rig):
    return [c for c in EXPECTED if c != ("short_any" if not rig.any_calls else "short_whole_blocks")]


def expected(rig, stage, case, on):
    want = EXPECTED[case][COLUMN[stage]]
    if want is None or case == "null_handle":
        return want, None
    if not on or (stage.startswith("os") and rig.F == 1):        # the stage-off refusal comes before every other but the null handle
        return NOT_READY, OFF_TEXT[stage]
    return want, TEXT.get(case, "").format(limit=rig.limit, cb=rig.cb)


def refuse_all_off(rig):
    """a fresh engine, every stage off: each case of each entry point is NOT_READY (the null handle INVALID_ARG)"""
    for stage in STAGES:
        if stage.startswith("os") and rig.F > 1:
            continue                                            # set_oversampling has turned it on
        for device in (False, True):
            for case in cases_of(rig):
                want, text = expected(rig, stage, case, on=False)
                if want is None:
                    continue
                rc = rig.call(stage, device, *rig.case(stage, device, case))
                assert rc == want, (stage, device, case, rc)
                if text:
                    assert text in rig.lib.cpq_last_error(rig.h).decode(), (stage, device, case)


def good_calls(rig, refusals):
    """{(stage, device): [the good calls' bytes]}: one before the cases, one after each case and the stage's reset.  refusals =
    False leaves out every case the table refuses."""
    out = {}
    for stage in STAGES:
        if stage.startswith("os") and rig.F == 1:
            continue
        rig.select(stage)
        for device in (False, True):
            rc, first = rig.good(stage, device)
            assert rc == OK, (stage, device, rc)
            seq = [first]
            for case in cases_of(rig):
                want, text = expected(rig, stage, case, on=True)
                if want is None:
                    continue
                if refusals or want == OK:
                    rc = rig.call(stage, device, *rig.case(stage, device, case))
                    assert rc == want, (stage, device, case, rc, rig.lib.cpq_last_error(rig.h).decode())
                    if rc != OK and text:
                        assert text in rig.lib.cpq_last_error(rig.h).decode(), (stage, device, case)
                rig.eng.synchronize()
                rig.reset(stage)
                rc, got = rig.good(stage, device)
                assert rc == OK, (stage, device, case, rc)
                seq.append(got)
            rig.reset(stage)
            out[stage, device] = seq
    return out


@pytest.mark.parametrize("factor", (1, 2))
@pytest.mark.parametrize("any_calls", (False, True), ids=("whole_blocks", "any"))
def test_every_refusal_and_the_good_calls_around_it(amd, any_calls, factor):
    rig, twin = Rig(amd, any_calls, factor), Rig(amd, any_calls, factor)
    refuse_all_off(rig)
    rig.stages_on()
    twin.stages_on()
    got, want = good_calls(rig, refusals=True), good_calls(twin, refusals=False)
    rig.close()
    twin.close()
    assert got.keys() == want.keys() and len(got) == (12 if factor > 1 else 8)
    for key, seq in got.items():
        assert len(seq) == len(want[key]) >= 8
        for k, (a, b) in enumerate(zip(seq, want[key])):
            assert a == b, (key, k)                             # a refusal moved nothing
        if key[0] in RESETS_ALL:
            assert all(a == seq[0] for a in seq), key
        else:
            assert len(set(seq)) == len(seq), key               # the generator ran on: no two of the dither calls agree
        assert any(np.frombuffer(seq[0], dtype=np.uint8))


@pytest.mark.parametrize("factor", (1, 2))
def test_host_calls_equal_device_calls(amd, factor):
    """fresh engines, output stage and dither on: 64 samples through each host entry point are the rows its _device variant
    writes (the host round trip: one buffer in place for the output stage and dither, two for the oversampler)"""
    host, dev = Rig(amd, True, factor), Rig(amd, True, factor)
    host.stages_on()
    dev.stages_on()
    for stage in ("out", "dither") + (("os_up", "os_down") if factor > 1 else ()):
        (rh, a), (rd, b) = host.good(stage, False), dev.good(stage, True)
        assert rh == OK and rd == OK, (stage, rh, rd)
        assert a == b and any(np.frombuffer(a, dtype=np.uint8)), stage
    host.close()
    dev.close()
