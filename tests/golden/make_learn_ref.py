"""Records tests/golden/learn_ref.npz from the reference's own CmaEsOptimizer.h through learn_probe.cpp.
    python tests/golden/make_learn_ref.py <reference source tree>
The probe binary is built into a temporary directory and is not kept.  Every case is a list of probe commands (learn_probe.cpp);
per generation the file holds the state before (mean 9, covariance 45, sigma), the z sample() drew, its candidates, the fitness
vector given, and the state after.  covRetentionCurrent is private to the optimiser and not serialised: it follows
min(target, current + step) from the target in force at initFromParcor, one comparison and one addition, restated in retention()
below.  Fitness vectors are made here and hold no two equal finite values: std::sort's order of ties is not pinned.  Where a
vector holds DBL_MAX at least six values are finite, so that the elite does not depend on the order of the tied tail."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT = [-0.003796, -0.006752, 0.008418, -0.010546, 0.004716, -0.007624, -0.020750, -0.002049, -0.003632]
STRONG = [0.82, -0.68, 0.55, -0.43, 0.33, -0.25, 0.18, -0.12, 0.07]
WIDE = [1.5, -3.0, 0.999, -0.995, 0.9949, 0.0, -0.0, 1.0e-20, -0.5]         # parcorToUnconstrained's clamp at +-0.995
DBL_MAX = float(np.finfo(np.float64).max)
STD = (0.03, 0.30, 0.92, 0.0)
N_STATE = 55
N_GEN = N_STATE + 162 + 162 + 18 + N_STATE


def fitness(g, salt=0, n_max=0):
    """18 distinct values, a different permutation per generation; the n_max largest become DBL_MAX"""
    f = [1.0 + 0.37 * ((7 * i + 5 * g + salt) % 18) + 0.01 * i for i in range(18)]
    for i in sorted(range(18), key=lambda i: -f[i])[:n_max]:
        f[i] = DBL_MAX
    return f


def upper(m):
    return [float(m[r][c]) for r in range(9) for c in range(r, 9)]


def spd():
    """a dense symmetric positive definite 9 x 9, from integers"""
    a = np.array([[((3 * r + 5 * c + r * c) % 7 - 3) / 8.0 for c in range(9)] for r in range(9)])
    return a @ a.T / 4.0 + 0.5 * np.eye(9)


def tiny():
    m = np.full((9, 9), 1.0e-16)
    m[np.arange(9), np.arange(9)] = 1.0
    m[0, 1] = m[1, 0] = -3.0e-16
    return m


def floors():
    """diagonal entries at 0 and below it, and one tiny: computeCholesky's two 1e-9 floors"""
    m = spd()
    m[2, 2] = 0.0
    m[5, 5] = -1.0
    m[7, 7] = 1.0e-20
    return m


def case(params0, parcor, seed, gens, params1=None, load=None, salt=0, n_max=0):
    """-> (commands, params in force per generation, retention before each generation's update)"""
    cmds = [("params",) + tuple(params0), ("init",) + tuple(parcor)]
    current = params0[2]
    p = params0
    if params1 is not None:
        cmds.append(("params",) + tuple(params1))
        p = params1
    if load is not None:
        mean, cov, sigma = load
        cmds.append(("load",) + tuple(mean) + tuple(upper(cov)) + (sigma,))
    cmds.append(("seed", seed))
    fits, rets = [], []
    for g in range(gens):
        f = fitness(g, salt, n_max)
        cmds.append(("gen",) + tuple(f))
        fits.append(f)
        rets.append(current)
        current = min(p[2], current + p[3])
    return cmds, [p] * gens, rets


MEAN = [0.3, -0.2, 0.1, 0.05, -0.4, 0.25, -0.15, 0.02, -0.01]
CASES = {
    "default": case(STD, DEFAULT, 7, 6),
    "strong": case((0.03, 0.30, 0.80, 0.02), STRONG, 11, 6, params1=(0.03, 0.30, 0.90, 0.02), salt=3),
    "loaded": case(STD, DEFAULT, 5, 5, load=(MEAN, spd(), 0.2), salt=1),
    "dblmax": case(STD, DEFAULT, 13, 5, salt=2, n_max=12),
    "clamp_lo": case((0.25, 0.3, 0.92, 0.0), DEFAULT, 17, 3, salt=4),
    "clamp_hi": case((0.01, 0.05, 0.92, 0.0), STRONG, 19, 3, salt=5),
    "tiny": case((0.03, 0.30, 1.0, 0.0), DEFAULT, 23, 3, load=(MEAN, tiny(), 0.1), salt=6),
    "floors": case(STD, DEFAULT, 29, 3, load=(MEAN, floors(), 0.15), salt=7),
}
INITS = {"default": DEFAULT, "strong": STRONG, "wide": WIDE}


def text(cmds):
    return "\n".join(" ".join(t if isinstance(t, str) else str(t) if isinstance(t, int) else float(t).hex() for t in c) for c in cmds) + "\n"


def main(ref):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "learn_probe")
        subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-I" + os.path.join(HERE, "juce_shim"), "-I" + os.path.join(ref, "src"),
                        os.path.join(HERE, "learn_probe.cpp"), "-o", exe], check=True)
        script, res = os.path.join(tmp, "script.txt"), os.path.join(tmp, "out.bin")

        def run(cmds):
            with open(script, "w") as f:
                f.write(text(cmds))
            subprocess.run([exe, script, res], check=True)
            return np.fromfile(res)

        for name, parcor in INITS.items():
            out["init_parcor_" + name] = np.array(parcor)
            out["init_state_" + name] = run([("params",) + STD, ("init",) + tuple(parcor), ("dump",)])
            assert out["init_state_" + name].shape == (N_STATE,)
        for name, (cmds, params, rets) in CASES.items():
            y = run(cmds).reshape(len(params), N_GEN)
            at = 0
            for key, n, shape in (("before", N_STATE, (N_STATE,)), ("z", 162, (18, 9)), ("cand", 162, (18, 9)), ("fit", 18, (18,)),
                                  ("after", N_STATE, (N_STATE,))):
                out[f"{name}_{key}"] = y[:, at:at + n].reshape((len(params),) + shape)
                at += n
            out[name + "_params"] = np.array(params)
            out[name + "_ret"] = np.array(rets)
            assert np.array_equal(out[name + "_before"][1:], out[name + "_after"][:-1]), name
            assert np.isfinite(out[name + "_z"]).all() and np.isfinite(out[name + "_cand"]).all(), name
    # what the cases are there for
    assert out["clamp_lo_after"][0, 54] == 0.25 and out["clamp_hi_after"][0, 54] == 0.05      # 0.12 is outside both ranges
    assert np.any((out["tiny_before"][0, 9:54] != 0.0) & (out["tiny_after"][0, 9:54] == 0.0))
    assert len(set(out["strong_ret"])) > 2
    np.savez_compressed(os.path.join(HERE, "learn_ref.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
