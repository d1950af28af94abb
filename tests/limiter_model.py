"""numpy and Python restatement of the look-ahead true-peak limiter of convopeq_amd/csrc/lim_plan.hpp over one whole programme,
independent of the C++.  The interpolator's integers and its term order are tests/prog_peak_model.py's.

  limit(x, rate, c, W, g)   x [2, N], one stereo programme from its start -> Result: y [2, N + D] (what every call and the
                            flush emit, back to back), a [N + D], min_gain, limited_samples
  named_inputs(n, seed)     the inputs the bound and the overshoot are taken on
  bound(c, W)               the largest |y| the definition allows: c + (W + 3) ulp(c)

The six steps.  u = scrub(x g); p = the largest of |u| and the interpolated phases over both channels; r = c / p where p > c,
else 1; m = the minimum of r over the last M = W + 12; a = (m[i] + m[i - 1] + ... + m[i - W + 1]) / W, added in that order from
0.0; y[i] = u[i - D] a[i] with D = W + 11.  Before the programme u = 0 and r = m = 1; behind its end x = 0."""
from collections import namedtuple

import numpy as np

import prog_peak_model as PM

Result = namedtuple("Result", "y a min_gain limited_samples")


def default_window(rate):
    return int(min(max(np.floor(0.0015 * rate + 0.5), 8), 1024))


def bound(c, W):
    return c + (W + 3) * np.spacing(c)


def limit(x, rate, c, W, g=1.0):
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 2 and x.shape[0] == 2
    M, D, N = W + 12, W + 11, x.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        u = PM.scrub(x * g)
    u = np.concatenate([u, np.zeros((2, D))], axis=1)          # the flush: x is 0.0 from its end on
    p = np.abs(u).max(axis=0)
    for ph in PM.phases(rate):
        p = np.maximum(p, PM.interpolated(u, ph).max(axis=0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = np.where(p > c, c / p, 1.0)
    rp = np.concatenate([np.ones(M - 1), r])
    m = np.lib.stride_tricks.sliding_window_view(rp, M).min(axis=1)     # m[i], i = 0 ... N + D - 1
    mp = np.concatenate([np.ones(W - 1), m])
    s = np.zeros(N + D)
    for j in range(W):                                          # newest first
        s = s + mp[W - 1 - j:W - 1 - j + N + D]
    a = s / float(W)
    delayed = np.concatenate([np.zeros((2, D)), u[:, :N]], axis=1)
    y = delayed * a
    return Result(y, a, float(a.min()), int((a < 1.0).sum()))


def named_inputs(n=6000, seed=7):
    """name -> [2, n]: noise with planted spikes, a full-scale fs/4 tone at the phase whose samples lie 3 dB under its crest, a step"""
    rng = np.random.default_rng(seed)
    noise = 0.2 * rng.standard_normal((2, n))
    for k, i in enumerate(range(97, n - 50, 411)):
        noise[k % 2, i] += (1.5 + 0.25 * (k % 5)) * (-1.0) ** k
        if k % 3 == 0:
            noise[:, i + 1] -= 1.1
    t = np.arange(n)
    tone = np.stack([np.sin(0.5 * np.pi * t + 0.25 * np.pi), np.cos(0.5 * np.pi * t + 0.25 * np.pi)]) / np.sin(0.25 * np.pi)
    step = np.zeros((2, n))
    step[0, n // 3:] = 1.7
    step[1, n // 2:] = -2.4
    return {"spikes": noise, "tone": tone, "step": step}
