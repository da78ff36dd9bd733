#!/usr/bin/env python3
"""Wall time of one lorads_hip_round_stable call at theta(4000, 40000, seed): seeded rank-40 factors (no
solve), K = 1024 trials, with the swap search off and on -- the median of --reps calls after one warm-up call each, the host
synchronised at both ends of a call (the call returns after its last read-back).  Appends one JSON line to --out (default
profiles/stable_time.jsonl).  Not part of bench.py."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lorads_amd import host, instances  # noqa: E402
from tests import common  # noqa: E402


def write_theta(path, n, n_edges, seed):
    """instances.theta(n, n_edges, seed) written line by line (the generator's list of 8 million tuples is not built)"""
    edges = instances._rand_edges(n, n_edges, np.random.default_rng(seed))
    with open(path, "w") as f:
        f.write("%d\n1\n%d\n" % (n_edges + 1, n))
        f.write("1.0 " + " ".join(["0.0"] * n_edges) + "\n")
        for i in range(1, n + 1):
            f.write("".join("0 1 %d %d 1.0\n" % (i, j) for j in range(i, n + 1)))
        f.write("".join("1 1 %d %d 1.0\n" % (i, i) for i in range(1, n + 1)))
        f.write("".join("%d 1 %d %d 1.0\n" % (k + 2, min(i, j) + 1, max(i, j) + 1) for k, (i, j) in enumerate(edges.tolist())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--edges", type=int, default=40000)
    ap.add_argument("--rank", type=int, default=40)
    ap.add_argument("--trials", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stable_time.jsonl"))
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="lorads_stable_time_")
    path = os.path.join(d, "theta.dat-s")
    t0 = time.perf_counter()
    write_theta(path, a.n, a.edges, a.seed)
    s = common.hip_session(path, timesLogRank=1e-3)
    rec = dict(n=a.n, edges=a.edges, rank=a.rank, trials=a.trials, reps=a.reps, setup_s=None)
    try:
        s.be.resize_rank([a.rank])
        rng = np.random.default_rng(a.seed)
        common.load_r_state(s.be, [rng.standard_normal((a.n, a.rank)) / np.sqrt(a.rank)], np.zeros(s.m))
        rec["setup_s"] = time.perf_counter() - t0
        for L in (0, 100):
            times, out = [], None
            for rep in range(a.reps + 1):
                lib, ctx = s._hip()
                lib.lorads_hip_sync(ctx)
                t = time.perf_counter()
                rc, out = s.be.round_stable(host.PAIR_RR, a.trials, a.seed, L)
                dt = time.perf_counter() - t
                assert rc == 0
                if rep:
                    times.append(dt)
            key = "search_%d" % L
            rec[key + "_ms"] = [1e3 * x for x in times]
            rec[key + "_median_ms"] = 1e3 * float(np.median(times))
            rec[key + "_best_size"] = int(out["sizes"][0, out["best"]])
            rec[key + "_trial0_size"] = int(out["sizes"][0, 0])
            rec[key + "_rounds"] = int(out["rounds"])
    finally:
        s.close()
        import shutil
        shutil.rmtree(d, True)
    print(json.dumps(rec))
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
