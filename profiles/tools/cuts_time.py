#!/usr/bin/env python3
"""Cost of Session.triangle_cuts at a Max-Cut instance's shape: --workload at --timesLogRank, after phase 1 and
--admm-steps ADMM iterations (as bench.py: phase1Tol 1e-2 ends phase 1 early), then --max-cuts cuts at --min-violation.  Warm (one call
first), median of --reps wall times per call; the violated count, the enumeration passes, and the triples enumerated per second
(passes x C(n, 3) / time) next to what the FP64 vector peak would allow at the loop's six additions and comparisons per triple.
rocprofv3 --kernel-trace --stats around a --quick run gives the kernels alone.  Appends one JSON line to --out.  Not part of bench.py."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lorads_amd import host, instances  # noqa: E402
from tests import common  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12   # MI355X data sheet, FLOP/s with an FMA counted as two: 39.3e12 additions per second
OPS_PER_TRIPLE = 6           # two additions, two additions of absolute values, a maximum, a comparison


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="maxcut800")
    ap.add_argument("--timesLogRank", type=float, default=2.0)
    ap.add_argument("--max-cuts", type=int, default=1000)
    ap.add_argument("--min-violation", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--admm-steps", type=int, default=10)
    ap.add_argument("--phase1Tol", type=float, default=1e-2)
    ap.add_argument("--quick", action="store_true", help="one timed call (for a rocprofv3 run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cuts_time.jsonl"))
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    d = tempfile.mkdtemp(prefix="cuts_time_")
    path = os.path.join(d, a.workload + ".dat-s")
    instances.write_sdpa(instances.NAMED[a.workload](), path)
    s = common.hip_session(path, timesLogRank=a.timesLogRank, phase1Tol=a.phase1Tol)
    res = {"workload": a.workload, "timesLogRank": a.timesLogRank, "phase1Tol": a.phase1Tol, "max_cuts": a.max_cuts,
           "min_violation": a.min_violation, "hip_source_sha256": bench.hip_source_hash()}
    try:
        t0 = time.time()
        s.alm()
        s.alm_to_admm()
        s.be.init_constr(host.PAIR_UV)
        err1 = s.be.update_dimacs(host.PAIR_UV)
        rho = min(s.results()["alm_rho"], 5000.0)
        s.admm_steps(a.admm_steps, rho, err1)
        res["state"] = "after phase 1 and %d ADMM iterations" % a.admm_steps
        res["t_setup_s"] = time.time() - t0
        res["shapes"] = [list(s.block_shape(k)) for k in range(s.nblk)]
        t0 = time.perf_counter()
        cuts = s.triangle_cuts(max_cuts=a.max_cuts, min_violation=a.min_violation)   # (the first call also makes the scratch)
        res["first_call_ms"] = 1e3 * (time.perf_counter() - t0)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            again = s.triangle_cuts(max_cuts=a.max_cuts, min_violation=a.min_violation)
            ts.append(1e3 * (time.perf_counter() - t0))
            assert again.violation.tobytes() == cuts.violation.tobytes() and again.count.tobytes() == cuts.count.tobytes()
        t0 = time.perf_counter()
        s.triangle_cuts(max_cuts=0, min_violation=a.min_violation)
        res["count_only_ms"] = 1e3 * (time.perf_counter() - t0)
        triples = sum(n * (n - 1) * (n - 2) // 6 for n, _ in res["shapes"])
        ms = float(np.median(ts))
        res.update(call_ms=ms, calls_ms=ts, count=[int(x) for x in cuts.count], kept=len(cuts), passes=cuts.passes,
                   largest_violation=float(cuts.violation[0]) if len(cuts) else 0.0, triples=triples,
                   triples_per_s=cuts.passes * triples / (ms * 1e-3), count_only_triples_per_s=triples / (res["count_only_ms"] * 1e-3),
                   peak_triples_per_s=FP64_VECTOR_PEAK / 2 / OPS_PER_TRIPLE)
    finally:
        s.close()
        os.remove(path)
        os.rmdir(d)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
