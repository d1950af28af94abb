"""Named inputs that reach the value edges of the minimum-phase conversion (convertToMinimumPhase: zero-pad to N -> FFT ->
ln max(|X|, 1e-300) -> IFFT -> fold -> FFT -> clamp +-50 on both parts, exp -> IFFT -> |v| < 1e-18 -> 0), the numpy restatement
that counts how often each edge is hit, and the pointwise rule of tests/test_gpu_ir_minphase_edges.py.  numpy only: no GPU, no
library.  Every input is a function of n returning a (1, n) or (2, n) float64 array; the seeds are fixed here.

    huge           uniform +-0.5 noise * 1e30         ln |X| is 60 and more: the real part is clamped at +50 in every bin
    tiny           the same noise * 1e-30             the real part is clamped at -50 in every bin; all outputs are flushed to 0
    silence        zeros                              |X| = 0: the 1e-300 floor in every bin, then the -50 clamp; output all zeros
    half_silent    stereo: the noise, zeros           the IR is not refused, channel 1 comes back as zeros
    flush          the noise * 1e-16                  dozens of outputs on either side of the 1e-18 flush
    comb           x[0] = 1, x[n - 1] = -1            bin 0 is 1 - 1 plus zeros, exactly 0 in any FFT: the floor in that bin, the -50
                                                      real clamp there, and the +-50 imaginary clamp in the bins around it
    late_impulse   a unit impulse at n // 2           a flat spectrum, ln (1 +- ulp): an impulse at 0, the rest flushed

No boxcar, nor any other input whose spectral zeros fall on bins with irrational twiddles: whether such a bin is exactly 0
depends on the FFT, and the floor makes the result discontinuous there.  (comb at n = 1025, N = 8192, has x[1024] = -1 and so a
zero in every eighth bin; those twiddles are w_8^(8 j) = 1, exact in any table, so the rule above is kept.)"""
import numpy as np

NOISE_SEED = 20240611
FLOOR = 1.0e-300
CLAMP = 50.0
FLUSH = 1.0e-18
EPS = 2.0 ** -52


def noise(n):
    return np.random.default_rng(NOISE_SEED + n).uniform(-0.5, 0.5, (1, n))


def huge(n):
    return noise(n) * 1.0e30


def tiny(n):
    return noise(n) * 1.0e-30


def silence(n):
    return np.zeros((1, n))


def half_silent(n):
    return np.concatenate([noise(n), np.zeros((1, n))])


def flush(n):
    return noise(n) * 1.0e-16


def comb(n):
    x = np.zeros((1, n))
    x[0, 0] = 1.0
    x[0, n - 1] = -1.0
    return x


def late_impulse(n):
    x = np.zeros((1, n))
    x[0, n // 2] = 1.0
    return x


INPUTS = {f.__name__: f for f in (huge, tiny, silence, half_silent, flush, comb, late_impulse)}

EDGE_SIZES = (700, 2000)                        # N = 4096: the row stays in LDS; N = 8192: column and row passes
BOUNDARY_SIZES = (1024, 1025)                   # the last row of the first path, the first of the second
BOUNDARY_INPUTS = ("comb", "silence", "flush")
# one row each: N = 2^19 (N2 = 1024), 2^20 (N1 = 1024), 2^21 (N2 = 2048), 2^22 (N1 = 2048: the 4-column tile), 2^23 (the largest
# row that is converted)
LARGE_SIZES = (65537, 131073, 262145, 524289, 2097152)


def large_row(n):
    """kind "b" of tests/test_gpu_ir_minphase.py's rows_of, seed 1000 + n: noise under exp(-6 t / n) with x[0] += 1"""
    x = np.random.default_rng(1000 + n).uniform(-0.5, 0.5, n) * np.exp(-6.0 * np.arange(n, dtype=np.float64) / n)
    x[0] += 1.0
    return x[None, :]


def edge_cases():
    """(name, n) of every value-edge case that runs on the device"""
    return [(name, n) for n in EDGE_SIZES for name in INPUTS] + [(name, n) for n in BOUNDARY_SIZES for name in BOUNDARY_INPUTS]


_REFERENCES = {}


def reference(key, x, host_fn, oracle_fn):
    """(x, host path, oracle, d_ref per row) of the input named by key, computed once in a session and shared by the CPU and the
    GPU file; the arrays are read-only"""
    if key not in _REFERENCES:
        host, orc = host_fn(x), oracle_fn(x)
        d_ref = np.array([yardstick(host[r], orc[r]) for r in range(x.shape[0])])
        for a in (x, host, orc, d_ref):
            a.setflags(write=False)
        _REFERENCES[key] = (x, host, orc, d_ref)
    return _REFERENCES[key]


def fft_size(n):
    size = 1
    while size < 4 * n:
        size <<= 1
    return size


def edge_counts(row):
    """The oracle's steps (oracle/ir_ingest_oracle.py: convert_to_minimum_phase) on one row, counting the bins and outputs at each
    edge: dict(N, floored, re_hi, re_lo, im_hi, im_lo, flushed, kept, near) -- near: outputs with 0 < |v| < 4e-18 before the flush
    decides, i.e. kept ones just above it and flushed ones just below."""
    n = len(row)
    size = fft_size(n)
    half = size // 2
    mag = np.abs(np.fft.fft(row, size))
    c = np.fft.ifft(np.log(np.maximum(mag, FLOOR)).astype(np.complex128))
    c[0] = c[0].real
    c[1:half] = c[1:half].real * 2.0
    c[half] = c[half].real
    c[half + 1:] = 0.0
    z = np.fft.fft(c)
    m = np.exp(np.clip(z.real, -CLAMP, CLAMP))
    im = np.clip(z.imag, -CLAMP, CLAMP)
    y = np.fft.ifft(m * np.cos(im) + 1j * (m * np.sin(im))).real[:n]
    return {"N": size, "floored": int((mag < FLOOR).sum()), "re_hi": int((z.real > CLAMP).sum()), "re_lo": int((z.real < -CLAMP).sum()),
            "im_hi": int((z.imag > CLAMP).sum()), "im_lo": int((z.imag < -CLAMP).sum()), "flushed": int((np.abs(y) < FLUSH).sum()),
            "kept": int((np.abs(y) >= FLUSH).sum()), "near": int(((np.abs(y) > 0.0) & (np.abs(y) < 4.0 * FLUSH)).sum())}


def excused(a, b, limit):
    """the flush clause: one of the two is exactly 0 and the other is below 1e-18 + limit (a value near 1e-18 may be kept by one
    implementation and zeroed by the other)"""
    return ((a == 0.0) & (np.abs(b) < FLUSH + limit)) | ((b == 0.0) & (np.abs(a) < FLUSH + limit))


def floor_of(host_row):
    return 8.0 * EPS * float(np.abs(host_row).max())


def yardstick(host_row, oracle_row):
    """d_ref of one row: the largest |host - oracle| over the elements the flush clause does not excuse.  The clause needs a limit
    and the limit needs d_ref, so d_ref is taken in two steps: first over the elements where both values are zero or both are not
    (no flush decision differs there), then, with the limit that follows from it, over everything the clause leaves."""
    diff = np.abs(host_row - oracle_row)
    same_side = (host_row == 0.0) == (oracle_row == 0.0)
    d0 = float(diff[same_side].max()) if same_side.any() else 0.0
    left = ~excused(host_row, oracle_row, max(8.0 * d0, floor_of(host_row)))
    return float(diff[left].max()) if left.any() else 0.0


def limit_of(host_row, d_ref):
    return max(8.0 * d_ref, floor_of(host_row))


def worst_ratio(got_row, host_row, d_ref):
    """(the largest |got - host| over the elements the flush clause does not excuse, the limit, their ratio): every element passes
    the rule exactly when the ratio is <= 1.  Against a limit of 0 (an all-zero host row) the ratio is 0 for no difference and inf
    for any."""
    limit = limit_of(host_row, d_ref)
    diff = np.abs(got_row - host_row)
    worst = float(diff[~excused(got_row, host_row, limit)].max(initial=0.0))
    if limit > 0.0:
        return worst, limit, worst / limit
    return worst, limit, (0.0 if worst == 0.0 else float("inf"))
