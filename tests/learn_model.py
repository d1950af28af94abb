"""The optimiser of cpq_learner (csrc/learn_plan.hpp) restated in plain Python floats: every +, -, *, / and math.sqrt is one
correctly rounded double operation, in the order the reference's CmaEsOptimizer.h writes them, so the model agrees with the
reference and with the library bit for bit wherever no log or tanh is involved.  States are dicts as
convopeq_amd.learner.state_to_dict makes them (lists or arrays of floats; rng: four Python ints)."""
import math

DIM, POP, ELITE = 9, 18, 6
DBL_MAX = 1.7976931348623157e308
MASK = (1 << 64) - 1
MAX_TRIES = 32


def sanitize(x):
    return 0.0 if (not math.isfinite(x) or abs(x) < 1e-15) else x


def clamp(v, lo, hi):
    return lo if v < lo else (hi if hi < v else v)


def cov_index(r, c):
    if c < r:
        r, c = c, r
    return r * DIM - (r * (r - 1)) // 2 + (c - r)


def rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & MASK


def word(s):
    """xoshiro256++: s is a list of four ints, advanced in place"""
    result = (rotl((s[0] + s[3]) & MASK, 23) + s[0]) & MASK
    t = (s[1] << 17) & MASK
    s[2] ^= s[0]
    s[3] ^= s[1]
    s[1] ^= s[2]
    s[0] ^= s[3]
    s[2] ^= t
    s[3] = rotl(s[3], 45)
    return result


def seed(v):
    """four successive splitmix64 outputs"""
    out = []
    for _ in range(4):
        v = (v + 0x9E3779B97F4A7C15) & MASK
        z = v
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        out.append(z ^ (z >> 31))
    return out


def normals(rng):
    """-> (z [162], words drawn, pairs given up, per pair the s whose logarithm was taken or None); rng advances in place"""
    z, words, rejected, ss = [], 0, 0, []
    for _ in range(POP * DIM // 2):
        for _t in range(MAX_TRIES):
            v1 = 2.0 * ((word(rng) >> 11) * 2.0 ** -53) - 1.0
            v2 = 2.0 * ((word(rng) >> 11) * 2.0 ** -53) - 1.0
            words += 2
            s = v1 * v1 + v2 * v2
            if 0.0 < s < 1.0:
                m = math.sqrt((-2.0 * math.log(s)) / s)
                z += [v1 * m, v2 * m]
                ss.append(s)
                break
        else:
            z += [0.0, 0.0]
            ss.append(None)
            rejected += 1
    return z, words, rejected, ss


def cholesky(cov):
    low = [[0.0] * DIM for _ in range(DIM)]
    for row in range(DIM):
        for column in range(row + 1):
            s = cov[cov_index(row, column)]
            for k in range(column):
                s -= low[row][k] * low[column][k]
            if row == column:
                low[row][column] = math.sqrt(max(s, 1.0e-9))
            else:
                low[row][column] = s / max(low[column][column], 1.0e-9)
    return low


def ask(state, z):
    """z [18][9] -> candidates [18][9]"""
    low = cholesky([float(v) for v in state["cov_upper"]])
    out = []
    for p in range(POP):
        row = []
        for dim in range(DIM):
            correlated = 0.0
            for column in range(dim + 1):
                correlated += low[dim][column] * float(z[p][column])
            row.append(sanitize(float(state["mean"][dim]) + float(state["sigma"]) * correlated))
        out.append(row)
    return out


def before(f, a, b):
    fa, fb = f[a], f[b]
    na, nb = fa != fa, fb != fb
    if na or nb:
        return a < b if na == nb else nb
    if fa < fb:
        return True
    if fb < fa:
        return False
    return a < b


def order(f):
    """ascending fitness, ties by the lower index, NaN last: stated as a key, so not the library's insertion sort restated"""
    return sorted(range(POP), key=lambda i: (f[i] != f[i], 0.0 if f[i] != f[i] else f[i], i))


def tell(state, params, cand, fit, mapped=None):
    """params: (sigma_min, sigma_max, target, step) -> (new state, the sort)"""
    smin, smax, target, step = params
    st = dict(state)
    cur = float(state["cov_retention"]) + step
    ret = cur if cur < target else target                    # std::min(target, current + step)
    idx = order(fit)
    old_mean, sigma = [float(v) for v in state["mean"]], float(state["sigma"])
    new_mean = []
    for dim in range(DIM):
        m = 0.0
        for e in range(ELITE):
            m += cand[idx[e]][dim]
        new_mean.append(m / 6.0)
    cov = [0.0] * 45
    for row in range(DIM):
        for column in range(row, DIM):
            elite = 0.0
            for e in range(ELITE):
                c = cand[idx[e]]
                elite += ((c[row] - old_mean[row]) / sigma) * ((c[column] - old_mean[column]) / sigma)
            i = cov_index(row, column)
            cov[i] = sanitize((ret * float(state["cov_upper"][i])) + (((1.0 - ret) / 6.0) * elite))
    var = 0.0
    for e in range(ELITE):
        for row in range(DIM):
            d = cand[idx[e]][row] - new_mean[row]
            var += d * d
    st["mean"] = [sanitize(m) for m in new_mean]
    st["cov_upper"] = cov
    st["sigma"] = clamp(math.sqrt(var / 54.0), smin, smax)
    st["cov_retention"] = ret
    best, best_score = 0, DBL_MAX
    for p in range(POP):
        if fit[p] < best_score:
            best_score, best = fit[p], p
    if best_score < float(state["best_score"]) and best_score < DBL_MAX:
        st["best_score"] = best_score
        st["best_raw"] = list(cand[best])
        if mapped is not None:
            st["best_scored"] = list(mapped[best])
    st["generations"] = int(state["generations"]) + 1
    return st, idx


def init(parcor, seed_value, target=0.92):
    mean = []
    for v in parcor:
        c = clamp(v, -0.995, 0.995)
        mean.append(0.5 * math.log((1.0 + c) / (1.0 - c)))
    cov = [0.0] * 45
    for r in range(DIM):
        cov[cov_index(r, r)] = 1.0
    return {"mean": mean, "cov_upper": cov, "sigma": 0.12, "cov_retention": target, "rng": seed(seed_value), "best_score": DBL_MAX,
            "best_raw": [0.0] * 9, "best_scored": [0.0] * 9, "generations": 0, "rejected_pairs": 0}


def map_candidates(cand, margin=0.85):
    """clampCoeff(std::tanh(candidate), margin)"""
    out = []
    for row in cand:
        r = []
        for c in row:
            k = math.tanh(c)
            r.append(0.0 if not math.isfinite(k) else (margin if k > margin else (-margin if k < -margin else k)))
        out.append(r)
    return out


# typed from src/NoiseShaperLearner.cpp:227-317: per mode, the two phase boundaries in seconds, the generation interval and the
# retention target per phase, and the retention step
PHASE_TABLE = {
    0: ((5.0, 10.0), (0.25, 0.5, 1.0), (0.80, 0.85, 0.90), 0.02),        # Shortest
    1: ((10.0, 20.0), (0.5, 1.0, 2.0), (0.85, 0.90, 0.95), 0.01),        # Short
    2: ((30.0, 60.0), (1.0, 2.0, 4.0), (0.90, 0.95, 0.98), 0.005),       # Middle
    3: ((60.0, 120.0), (2.0, 4.0, 8.0), (0.95, 0.98, 0.99), 0.002),      # Long
    4: ((120.0, 240.0), (4.0, 8.0, 16.0), (0.98, 0.99, 0.995), 0.001),   # Ultra
    5: ((30.0, 60.0), (1.0, 2.0, 4.0), (0.90, 0.95, 0.98), 0.005),       # Continuous
}
PHASE_WEIGHTS = {1: (0.1, 0.2, 0.3, 0.4), 2: (0.25, 0.25, 0.25, 0.25), 3: (0.5, 0.3, 0.1, 0.1)}
