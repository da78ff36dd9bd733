#!/usr/bin/env python3
"""Wall time of one lorads_hip_round_bisect call at instances.bisection(n, 6 n, seed) for n = 800 and
n = 2000: seeded rank-32 factors (no solve), K = 1024 trials, with the swap search off (L = 0) and on (L = 1000) -- the median of
--reps calls after one warm-up call each, the host synchronised at both ends of a call (the call returns after its last
read-back).  Appends one JSON line per n to --out (default profiles/bisect_time.jsonl), with the hash of the HIP sources.  Not part
of bench.py."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lorads_amd import host, instances  # noqa: E402
from tests import common  # noqa: E402


def write_bisection(path, n, n_edges, seed):
    """instances.bisection(n, n_edges, seed) with the sum row written line by line (its n (n + 1) / 2 tuples are not built)"""
    prob = instances.maxcut(n, n_edges, seed)
    with open(path, "w") as f:
        f.write("%d\n1\n%d\n" % (n + 1, n))
        f.write(" ".join(["1.0"] * n) + " 0.0\n")
        for mat, blk, i, j, v in prob["entries"]:
            f.write("%d %d %d %d %r\n" % (mat, blk, i, j, float(-v if mat == 0 else v)))
        for i in range(1, n + 1):
            f.write("".join("%d 1 %d %d 1.0\n" % (n + 1, i, j) for j in range(i, n + 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[800, 2000])
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--trials", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bisect_time.jsonl"))
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="lorads_bisect_time_")
    try:
        for n in a.n:
            path = os.path.join(d, "bisect%d.dat-s" % n)
            t0 = time.perf_counter()
            write_bisection(path, n, 6 * n, a.seed)
            s = common.hip_session(path, timesLogRank=1e-3)
            rec = dict(hip_source_sha256=bench.hip_source_hash(), n=n, edges=6 * n, rank=a.rank, trials=a.trials, reps=a.reps)
            try:
                s.be.resize_rank([a.rank])
                rng = np.random.default_rng(a.seed)
                common.load_r_state(s.be, [rng.standard_normal((n, a.rank)) / np.sqrt(a.rank)], np.zeros(s.m))
                rec["setup_s"] = time.perf_counter() - t0
                for L in (0, 1000):
                    times, out = [], None
                    for rep in range(a.reps + 1):
                        lib, ctx = s._hip()
                        lib.lorads_hip_sync(ctx)
                        t = time.perf_counter()
                        rc, out = s.be.round_bisect(host.PAIR_RR, a.trials, a.seed, L)
                        dt = time.perf_counter() - t
                        assert rc == 0
                        if rep:
                            times.append(dt)
                    key = "search_%d" % L
                    rec[key + "_ms"] = [1e3 * x for x in times]
                    rec[key + "_median_ms"] = 1e3 * float(np.median(times))
                    rec[key + "_best_f"] = float(out["obj"][out["best"]])
                    rec[key + "_rounds"] = int(out["rounds"])
                    rec["largest_imbalance"] = int(np.abs(out["imbalance"]).max())
            finally:
                s.close()
            print(json.dumps(rec))
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
    finally:
        shutil.rmtree(d, True)


if __name__ == "__main__":
    main()
