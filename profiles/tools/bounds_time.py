#!/usr/bin/env python3
"""Cost of Session.entry_bounds at an instance's shape: --workload at bench.py's settings for it (timesLogRank,
phase1Tol 1e-2 ends phase 1 early, reoptLevel 0), after phase 1 and --admm-steps ADMM iterations, then --max-cuts cuts of
[--lower, --upper] at --min-violation.  Warm (one call first), median of --reps wall times per call, full and count-only; the violated
count, the enumeration passes, and the pairs enumerated per second of one enumeration pass (the count-only call is one pass plus the
pack and one synchronisation) next to what the FP64 matrix cores' peak allows at 2 r4 FLOP per pair (r4: the rank rounded up to a
multiple of four).  Appends one JSON line to --out.  Not part of bench.py."""
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

FP64_MATRIX_PEAK = 78.6e12   # MI355X data sheet, FLOP/s with an FMA counted as two (the FP64 matrix rate equals the vector rate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="theta50")
    ap.add_argument("--timesLogRank", type=float, default=None)
    ap.add_argument("--max-cuts", type=int, default=1000)
    ap.add_argument("--lower", type=float, default=0.0)
    ap.add_argument("--upper", type=float, default=float("inf"))
    ap.add_argument("--min-violation", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--admm-steps", type=int, default=10)
    ap.add_argument("--phase1Tol", type=float, default=1e-2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bounds_time.jsonl"))
    a = ap.parse_args()
    tlr = a.timesLogRank if a.timesLogRank is not None else {"matcomp50000": 5.5, "blk16x4000": 2.0}.get(a.workload, 4.0)
    d = tempfile.mkdtemp(prefix="bounds_time_")
    path = os.path.join(d, a.workload + ".dat-s")
    instances.write_sdpa(instances.NAMED[a.workload](), path)
    params = dict(timesLogRank=tlr, phase1Tol=a.phase1Tol, reoptLevel=0)
    if a.workload == "matcomp50000":
        params["dyrankLevel"] = 0   # (as bench.py: the rank stays at 60)
    s = common.hip_session(path, **params)
    res = {"workload": a.workload, "timesLogRank": tlr, "phase1Tol": a.phase1Tol, "max_cuts": a.max_cuts,
           "lower": a.lower if np.isfinite(a.lower) else None, "upper": a.upper if np.isfinite(a.upper) else None,
           "min_violation": a.min_violation, "hip_source_sha256": bench.hip_source_hash()}
    kw = dict(lower=a.lower, upper=a.upper, min_violation=a.min_violation)
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
        lp = s._lp_blocks()
        res["shapes"] = [list(s.block_shape(k)) for k in range(s.nblk) if not lp[k]]
        t0 = time.perf_counter()
        b = s.entry_bounds(max_cuts=a.max_cuts, **kw)   # (the first call also makes the scratch)
        res["first_call_ms"] = 1e3 * (time.perf_counter() - t0)
        ts, tc = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            again = s.entry_bounds(max_cuts=a.max_cuts, **kw)
            ts.append(1e3 * (time.perf_counter() - t0))
            assert again.violation.tobytes() == b.violation.tobytes() and again.count.tobytes() == b.count.tobytes()
        for _ in range(a.reps):
            t0 = time.perf_counter()
            cnt = s.entry_bounds(max_cuts=0, **kw)
            tc.append(1e3 * (time.perf_counter() - t0))
            assert cnt.count.tobytes() == b.count.tobytes()
        pairs = sum(n * (n - 1) // 2 for n, _ in res["shapes"])
        flop = sum(n * (n - 1) // 2 * 2 * ((r + 3) // 4 * 4) for n, r in res["shapes"])
        ms, mc = float(np.median(ts)), float(np.median(tc))
        res.update(call_ms=ms, calls_ms=ts, count_only_ms=mc, count_only_calls_ms=tc, count=[int(x) for x in b.count], kept=len(b),
                   passes=b.passes, largest_violation=float(b.violation[0]) if len(b) else 0.0, pairs=pairs,
                   pairs_per_s=pairs / (mc * 1e-3), pairs_per_s_full_call=b.passes * pairs / (ms * 1e-3),
                   peak_pairs_per_s=FP64_MATRIX_PEAK * pairs / flop, share_of_peak=(flop / (mc * 1e-3)) / FP64_MATRIX_PEAK)
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
