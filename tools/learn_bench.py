"""Times a generation of the shaper learner -- 18 candidates x 16 segments per learner, 16 bits, 48 kHz -- two ways on the same
scorer: cpq_learner_run(G), which enqueues G generations and is waited for once, and the loop a caller had to write before it,
cpq_learn_ask_host -> cpq_scorer_score_raw -> cpq_learn_tell_host per generation with the states on the host.  Reported per
learner count: milliseconds per generation of both (median over repeats of a whole run of G), the event times of ask and of tell
(cpq_learner_last_timing) and of the scorer's two stages (cpq_scorer_last_timing) of a run's last generation.  These are the
figures of RESULTS.md, "Shaper learner".

    python tools/learn_bench.py [--learners 1 64 1024] [--generations 8] [--repeats 5] [--warmup 1] [--out profiles/learn_bench.json]

Every learner holds seeded noise at its own level, long enough for all 16 segments (tools/score_bench.py's inputs)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT = [-0.003796, -0.006752, 0.008418, -0.010546, 0.004716, -0.007624, -0.020750, -0.002049, -0.003632]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--learners", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--generations", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import convopeq_amd as amd
    from convopeq_amd import _capi as K
    from convopeq_amd import learner as L
    lib = K.load()

    rows = []
    for n in a.learners:
        sc = amd.ShaperScorer(n, 18, 48000.0, 16)
        for l in range(n):
            rng = np.random.default_rng(l)
            x = rng.standard_normal((2, K.CPQ_SCORE_RECENT)) * (0.02 + 0.2 * rng.random())
            assert sc.buildTrainingSegments(l, np.clip(x[0], -1.0, 1.0), np.clip(x[1], -1.0, 1.0)) == K.CPQ_SCORE_MAX_SEGMENTS
        ln = amd.ShaperLearner(sc)
        params = L.make_params()
        device, host, ask, tell, lattice, spectrum = [], [], [], [], [], []
        for i in range(a.warmup + a.repeats):
            ln.init(DEFAULT, 1)
            t0 = time.perf_counter()
            ln.run(a.generations)
            ln.get_state(0)                                     # the wait
            t1 = time.perf_counter()
            if i >= a.warmup:
                device.append((t1 - t0) * 1e3 / a.generations)
                at, tt = ln.last_timing()
                lt, st = sc.last_timing()
                ask.append(at), tell.append(tt), lattice.append(lt), spectrum.append(st)
        assert all(ln.get_state(l)["generations"] == a.generations for l in (0, n - 1))
        for i in range(a.warmup + a.repeats):
            # the library's entries on its own structs: three calls per learner and generation, no conversion in between
            states = (K.LearnState * n)(*[L.state_from_dict(L.init_host(DEFAULT, 1 + l)) for l in range(n)])
            cand, z = np.empty((n, 18, 9)), np.empty((18, 9))
            cp = [cand[l].ctypes.data_as(K.c_double_p) for l in range(n)]
            zp, pp = z.ctypes.data_as(K.c_double_p), C.byref(params)
            t0 = time.perf_counter()
            for _ in range(a.generations):
                for l in range(n):
                    lib.cpq_learn_normals_host(C.byref(states[l]), zp, None)
                    lib.cpq_learn_ask_host(C.byref(states[l]), zp, cp[l])
                scores = sc.score_raw(cand)
                for l in range(n):
                    lib.cpq_learn_tell_host(C.byref(states[l]), pp, cp[l], None, scores[l].ctypes.data_as(K.c_double_p), None)
            t1 = time.perf_counter()
            if i >= a.warmup:
                host.append((t1 - t0) * 1e3 / a.generations)
        ln.close()
        sc.close()
        row = {"learners": n, "generations": a.generations, "repeats": a.repeats}
        for name, v in (("device_ms_per_generation", device), ("host_loop_ms_per_generation", host), ("ask_ms", ask), ("tell_ms", tell),
                        ("lattice_ms", lattice), ("spectrum_ms", spectrum)):
            row[name] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        row["host_over_device"] = row["host_loop_ms_per_generation"]["median"] / row["device_ms_per_generation"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
