"""Times one cpq_scorer_score call -- 18 candidates x 16 segments per learner, 16 bits, 48 kHz -- for 1 and 64 learners, split into
the lattice stage and the spectrum stage by the scorer's own events (cpq_scorer_last_timing), next to the call's wall time.
These are the figures of RESULTS.md, "Shaper scorer".

    python tools/score_bench.py [--learners 1 64] [--calls 10] [--warmup 3] [--out profiles/score_bench.json]

Every learner holds seeded noise at its own level, long enough for all 16 segments; the candidates are stable sets within +-0.3."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--learners", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--candidates", type=int, default=18)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import convopeq_amd as amd
    from convopeq_amd import _capi as K

    rows = []
    for n_learners in a.learners:
        sc = amd.ShaperScorer(n_learners, a.candidates, 48000.0, 16)
        for l in range(n_learners):
            rng = np.random.default_rng(l)
            x = rng.standard_normal((2, K.CPQ_SCORE_RECENT)) * (0.02 + 0.2 * rng.random())
            assert sc.buildTrainingSegments(l, np.clip(x[0], -1.0, 1.0), np.clip(x[1], -1.0, 1.0)) == K.CPQ_SCORE_MAX_SEGMENTS
        k = np.random.default_rng(1000).uniform(-0.3, 0.3, (n_learners, a.candidates, 9)) / (1.0 + 0.25 * np.arange(9))
        lattice, spectrum, wall = [], [], []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            scores = sc.score(k)
            t1 = time.perf_counter()
            if i >= a.warmup:
                ms = sc.last_timing()
                lattice.append(ms[0])
                spectrum.append(ms[1])
                wall.append((t1 - t0) * 1e3)
        assert np.isfinite(scores).all() and (scores < K.CPQ_SCORE_UNSTABLE).all()
        sc.close()
        evals = n_learners * a.candidates * K.CPQ_SCORE_MAX_SEGMENTS
        row = {"learners": n_learners, "candidates": a.candidates, "chains": 2 * evals, "evaluations": evals, "calls": a.calls}
        for name, v in (("lattice_ms", lattice), ("spectrum_ms", spectrum), ("wall_ms", wall)):
            row[name] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        row["lattice_us_per_step"] = row["lattice_ms"]["median"] * 1e3 / K.CPQ_SCORE_SEGMENT_LEN
        row["spectrum_us_per_evaluation"] = row["spectrum_ms"]["median"] * 1e3 / evals
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
