#!/usr/bin/env python3
"""Cost of Session.round_kcut at cfg3a: maxcut20000, r = 40 (--timesLogRank 4.0), after phase 1 and five ADMM
steps.  Times parts in {2, 3, 8} x K in {64, 1024, 8192} with the local search off and on (median of --reps calls after one warm-up
call each) and, as the yardstick, Session.round_pm1 at the same K in the same run.  Appends one JSON line to --out (default
profiles/kcut_time.jsonl).  Not part of bench.py.

--quick: one call per case at K = 1024 only, for a `rocprofv3 --kernel-trace --stats` run of its own.  --stats-csv FILE (no GPU
work) reads that run's kernel_stats.csv and appends, for the last --quick record of --out, per kernel of the two roundings the calls
and the total time, and for k_kcut_label and k_rnd_sign the time per score (row x trial x vector) and the share of the FP64 matrix
peak as section 15 computes it (2 rl flops per score against 78.6 TFLOP/s)."""
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

PEAK_FP64_MATRIX = 78.6e12


def kernel_stats(path, n, rl, scores):
    """{kernel: {calls, total_ms}} of the rounding kernels; scores = {kernel: scores computed over the whole run}"""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            hit = re.search(r"\bk_(kcut|rnd)_[a-z0-9_]+", name)
            if not hit:
                continue
            short = hit.group(0)
            calls = int(float(row.get("Calls") or row.get("Count") or 0))
            total_ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or row.get("Total Duration") or 0.0)
            d = out.setdefault(short, {"calls": 0, "total_ms": 0.0})
            d["calls"] += calls
            d["total_ms"] += total_ns * 1e-6
    for k, sc in scores.items():
        if k in out and sc:
            out[k]["scores"] = sc
            out[k]["ns_per_score"] = out[k]["total_ms"] * 1e6 / sc
            out[k]["share_of_fp64_matrix_peak"] = 2.0 * rl * sc / (out[k]["total_ms"] * 1e-3) / PEAK_FP64_MATRIX
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--admm-steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kcut_time.jsonl"))
    a = ap.parse_args()
    if a.stats_csv:   # no GPU work: the kernel statistics of the last --quick record of --out, appended as a record of their own
        with open(a.out) as fh:
            quick = [r for r in map(json.loads, fh) if r.get("quick") and "scores" in r][-1]
        res = {"workload": quick["workload"], "hip_source_sha256": quick["hip_source_sha256"], "n": quick["n"], "rank": quick["rank"],
               "kernels": kernel_stats(a.stats_csv, quick["n"], quick["rank"], quick["scores"])}
        print(json.dumps(res))
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")
        return
    reps = 1 if a.quick else a.reps
    d = tempfile.mkdtemp(prefix="kcut_time_")
    path = os.path.join(d, "maxcut20000.dat-s")
    instances.write_sdpa(instances.NAMED["maxcut20000"](), path)
    s = common.hip_session(path, timesLogRank=4.0)
    res = {"workload": "maxcut20000 (cfg3a)", "hip_source_sha256": bench.hip_source_hash(), "quick": bool(a.quick)}
    scores = {"k_kcut_label": 0, "k_rnd_sign": 0}
    try:
        t0 = time.time()
        s.alm()
        s.alm_to_admm()
        res["t_phase1_s"] = time.time() - t0
        s.be.init_constr(host.PAIR_UV)
        e0 = s.be.update_dimacs(host.PAIR_UV)
        s.admm_steps(a.admm_steps, 1.0, e0)
        n, rl = s.block_shape(0)
        res["n"], res["rank"] = n, rl
        cases = []
        for K in ((1024,) if a.quick else (64, 1024, 8192)):
            for L in (0, 100):
                if not a.quick:
                    s.round_pm1(trials=K, seed=1, local_search_rounds=L, tol=0)   # warm-up (first use: check, colouring, scratch)
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    r = s.round_pm1(trials=K, seed=1, local_search_rounds=L, tol=0)
                    ts.append(time.perf_counter() - t0)
                scores["k_rnd_sign"] += n * K * (reps + (0 if a.quick else 1))
                cases.append(dict(call="round_pm1", K=K, L=L, ms_median=1e3 * float(np.median(ts)), ms_min=1e3 * min(ts),
                                  rounds=r.rounds, f_best=r.f_best))
                print(json.dumps(cases[-1]), flush=True)
                for parts in (2, 3, 8):
                    try:
                        if not a.quick:
                            s.round_kcut(parts, trials=K, seed=1, local_search_rounds=L, tol=0)
                        ts = []
                        for _ in range(reps):
                            t0 = time.perf_counter()
                            r = s.round_kcut(parts, trials=K, seed=1, local_search_rounds=L, tol=0)
                            ts.append(time.perf_counter() - t0)
                    except RuntimeError as e:   # (the scratch does not fit)
                        cases.append(dict(call="round_kcut", parts=parts, K=K, L=L, error=str(e)))
                        continue
                    scores["k_kcut_label"] += n * K * parts * (reps + (0 if a.quick else 1))
                    cases.append(dict(call="round_kcut", parts=parts, K=K, L=L, ms_median=1e3 * float(np.median(ts)),
                                      ms_min=1e3 * min(ts), rounds=r.rounds, f_best=r.f_best,
                                      cut_weight=-2.0 * r.f_best * (parts - 1) / parts))
                    print(json.dumps(cases[-1]), flush=True)
        res["cases"] = cases
        res["scores"] = scores
    finally:
        s.close()
        os.remove(path)
        os.rmdir(d)
    line = json.dumps(res)
    print(line)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
