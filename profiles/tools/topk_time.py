#!/usr/bin/env python3
"""Cost of Session.primal_topk at cfg5: matcomp50000 at bench.py's settings for it, after phase 1 and five ADMM
steps.  Wall time per call with the host's share (the skip lists, the read-back), warm, median of --reps, for
  users   all 25000 user rows over the item columns, k = 10 and k = 100, with skip_constrained
  rows32  32 rows over all columns, k = 10
  row1    1 row over all columns, k = 10
and, as yardsticks in the same run, Session.entry_bounds with max_cuts = 0 on the same cone (the bare enumeration: pairs per second)
and the read-back route for the 32-row case: Session.primal_apply on a panel of 32 unit vectors plus numpy.argpartition.  Appends
one JSON line to --out (default profiles/topk_time.jsonl).  Not part of bench.py.

--quick: one call per case, for a `rocprofv3 --kernel-trace --stats` run of its own.  --stats-csv FILE (no GPU work) reads that
run's kernel_stats.csv and appends, for the last --quick record of --out, calls and total time of the k_topk_*, k_bnd_* and k_pack_* kernels
and the scan's pairs per second."""
import argparse
import csv
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lorads_amd import host, instances  # noqa: E402
from tests import common  # noqa: E402

FP64_MATRIX_PEAK = 78.6e12   # as section 15


def kernel_stats(path):
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            hit = re.search(r"\bk_(topk|bnd|pack)_[a-z0-9_]+", name)
            if not hit:
                continue
            d = out.setdefault(hit.group(0), {"calls": 0, "total_ms": 0.0})
            d["calls"] += int(float(row.get("Calls") or row.get("Count") or 0))
            d["total_ms"] += 1e-6 * float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or row.get("Total Duration") or 0.0)
    return out


def timed(fn, reps, warm):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return r, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="matcomp50000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--admm-steps", type=int, default=5)
    ap.add_argument("--phase1Tol", type=float, default=1e-2)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_time.jsonl"))
    a = ap.parse_args()
    if a.stats_csv:   # no GPU work
        with open(a.out) as fh:
            quick = [r for r in map(json.loads, fh) if r.get("quick") and "scan_pairs" in r][-1]
        ks = kernel_stats(a.stats_csv)
        res = {"workload": quick["workload"], "hip_source_sha256": quick["hip_source_sha256"], "shape": quick["shape"], "kernels": ks}
        if "k_topk_scan" in ks and ks["k_topk_scan"]["total_ms"] > 0:
            rate = quick["scan_pairs"] / (ks["k_topk_scan"]["total_ms"] * 1e-3)
            res["scan_pairs_per_s"] = rate
            res["scan_share_of_fp64_matrix_peak"] = rate * 2 * ((quick["shape"][1] + 3) // 4 * 4) / FP64_MATRIX_PEAK
        if "k_bnd_enum" in ks and ks["k_bnd_enum"]["total_ms"] > 0:
            res["enum_pairs_per_s"] = quick["enum_pairs"] / (ks["k_bnd_enum"]["total_ms"] * 1e-3)
        print(json.dumps(res))
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")
        return
    reps, warm = (1, False) if a.quick else (a.reps, True)
    d = tempfile.mkdtemp(prefix="topk_time_")
    path = os.path.join(d, a.workload + ".dat-s")
    instances.write_sdpa(instances.NAMED[a.workload](), path)
    params = dict(timesLogRank={"matcomp50000": 5.5}.get(a.workload, 4.0), phase1Tol=a.phase1Tol, reoptLevel=0)
    if a.workload == "matcomp50000":
        params["dyrankLevel"] = 0   # (as bench.py: the rank stays at 60)
    s = common.hip_session(path, **params)
    res = {"workload": a.workload, "hip_source_sha256": bench.hip_source_hash(), "quick": bool(a.quick)}
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
        n, r = s.block_shape(0)
        res["shape"] = [n, r]
        half = n // 2
        users = np.arange(half, dtype=np.int32)
        rows32 = np.arange(0, 32 * (half // 32), half // 32, dtype=np.int32)[:32]
        cases = []
        scan_pairs = 0
        calls = (1 if a.quick else reps + 1)

        def case(name, rows, k, cols, sc):
            nonlocal scan_pairs
            out, ts = timed(lambda: s.primal_topk(0, rows, k, cols=cols, skip_constrained=sc), reps, warm)
            lo, hi = cols if cols else (0, n)
            pairs = len(rows) * (hi - lo)
            scan_pairs += pairs * calls
            cases.append(dict(case=name, queries=len(rows), k=k, window=[lo, hi], skip_constrained=sc, ms_median=float(np.median(ts)),
                              ms_all=ts, found=int(out[2].sum()), pairs=pairs, pairs_per_s=pairs / (1e-3 * float(np.median(ts)))))
            print(json.dumps(cases[-1]), flush=True)
            return out

        case("users", users, 10, (half, n), True)
        case("users", users, 100, (half, n), True)
        case("users, no skip list", users, 10, (half, n), False)
        got32 = case("rows32", rows32, 10, None, False)
        case("row1", rows32[:1], 10, None, False)
        # the bare enumeration of the same cone
        b, tc = timed(lambda: s.entry_bounds(max_cuts=0, lower=0.0, upper=None), reps, warm)
        pairs = n * (n - 1) // 2
        res["enum_pairs"] = pairs * calls
        cases.append(dict(case="entry_bounds, count only", ms_median=float(np.median(tc)), ms_all=tc, pairs=pairs,
                          pairs_per_s=pairs / (1e-3 * float(np.median(tc)))))
        print(json.dumps(cases[-1]), flush=True)

        # the read-back route for the 32 rows: X E on the device, the selection on the host
        def readback():
            E = np.zeros((n, 32), order="F")
            E[rows32, np.arange(32)] = 1.0
            Y = s.primal_apply(0, E)
            Y[rows32, np.arange(32)] = -np.inf
            part = np.argpartition(-Y, 10, axis=0)[:10]
            return part, Y
        (part, Y), tr = timed(readback, reps, warm)
        agree = sum(len(set(part[:, j].tolist()) & set(got32[0][j].tolist())) for j in range(32))
        cases.append(dict(case="rows32 by primal_apply + argpartition", ms_median=float(np.median(tr)), ms_all=tr,
                          columns_in_common_with_primal_topk=agree, of=320))
        print(json.dumps(cases[-1]), flush=True)
        res["cases"] = cases
        res["scan_pairs"] = scan_pairs
    finally:
        s.close()
        os.remove(path)
        os.rmdir(d)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
