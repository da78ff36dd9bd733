#!/usr/bin/env python3
"""Cost and effect of Session.spectrum / Session.compress_rank on a large instance: --workload maxcut20000
(cfg3a), rand20000 (cfg3b) or matcomp50000 (cfg5) at --timesLogRank, after phase 1 and --admm-steps ADMM iterations (--solve: after
the whole solve).  Times spectrum() and a full compress_rank at the current ranks (a pure rotation, so it can be repeated: median of
--reps calls after one warm-up call each), the ADMM iterations per second and -- on Max-Cut -- a rounding call before and after the
reduction at --tol, and numpy on the host for scale (the get_mat copy, the Gram, eigvalsh).  Prints one JSON object (and writes it
to --out).  Not part of bench.py.  --quick: one call per case (for a rocprofv3 --kernel-trace --stats run)."""
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


def _its_per_s(s, rho, err1, steps):
    s.admm_steps(3, rho, err1)
    s.hip_sync()
    t0 = time.perf_counter()
    out = s.admm_steps(steps, rho, err1)
    s.hip_sync()
    return steps / (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="maxcut20000")
    ap.add_argument("--timesLogRank", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--admm-steps", type=int, default=50)
    ap.add_argument("--phase1Tol", type=float, default=None, help="as bench.py: 1e-2 ends phase 1 early")
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    d = tempfile.mkdtemp(prefix="spectral_time_")
    path = os.path.join(d, a.workload + ".dat-s")
    instances.write_sdpa(instances.NAMED[a.workload](), path)
    kw = {} if a.phase1Tol is None else dict(phase1Tol=a.phase1Tol)
    s = common.hip_session(path, timesLogRank=a.timesLogRank, **kw)
    res = {"workload": a.workload, "timesLogRank": a.timesLogRank, "phase1Tol": a.phase1Tol, "hip_source_sha256": bench.hip_source_hash()}
    try:
        t0 = time.time()
        if a.solve:
            r = s.solve()
            rho, err1 = min(r["admm_rho"], 5000.0), r["constrVio1"]
            res["state"] = "after solve(): status %d" % r["status"]
        else:
            s.alm()
            s.alm_to_admm()
            s.be.init_constr(host.PAIR_UV)
            err1 = s.be.update_dimacs(host.PAIR_UV)
            r = s.results()
            rho = min(r["alm_rho"], 5000.0)
            err1 = s.admm_steps(a.admm_steps, rho, err1)[0]
            res["state"] = "after phase 1 and %d ADMM iterations" % a.admm_steps
        res["t_setup_s"] = time.time() - t0
        res["shapes"] = [list(s.block_shape(k)) for k in range(s.nblk)]
        res["err1"] = err1
        lam, sweeps = s.spectrum(sweeps=True)   # warm-up (first use: the scratch)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            lam, sweeps = s.spectrum(sweeps=True)
            ts.append(time.perf_counter() - t0)
        res["spectrum_ms_median"], res["spectrum_ms_min"], res["sweeps"] = 1e3 * float(np.median(ts)), 1e3 * min(ts), sweeps
        res["spectrum_rel"] = [[float(x / l[0]) for x in l] for l in lam if len(l)]
        res["ranks_kept"] = {str(t): [int(max(1, np.sum(l > t * l[0]))) for l in lam if len(l)] for t in (1e-12, 1e-8, 1e-4)}
        # numpy on the host, for scale: the copy, the Gram, the eigenvalues
        t0 = time.perf_counter()
        F = [(s.be.get_mat(host.MAT_U, k) + s.be.get_mat(host.MAT_V, k)) / 2 for k in range(s.nblk)]
        t1 = time.perf_counter()
        G = [f.T @ f for f in F]
        t2 = time.perf_counter()
        w = [np.linalg.eigvalsh(g)[::-1] for g in G]
        t3 = time.perf_counter()
        res["numpy_host_ms"] = dict(get_mat=1e3 * (t1 - t0), gram=1e3 * (t2 - t1), eigvalsh=1e3 * (t3 - t2))
        res["eig_vs_numpy_rel"] = max(float(np.abs(x - y).max() / y[0]) for x, y in zip([l for l in lam if len(l)], w))
        if not a.quick:
            res["admm_it_per_s_before"] = _its_per_s(s, rho, err1, 40)[0]
        rounding = a.workload.startswith("maxcut")
        if rounding:
            s.round_pm1(trials=1024, seed=1, local_search_rounds=0, tol=0)
            t0 = time.perf_counter()
            s.round_pm1(trials=1024, seed=1, local_search_rounds=0, tol=0)
            res["round_K1024_ms_before"] = 1e3 * (time.perf_counter() - t0)
        ranks = [s.block_shape(k)[1] for k in range(s.nblk)]
        s.compress_rank(ranks=ranks)   # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            s.compress_rank(ranks=ranks)
            ts.append(time.perf_counter() - t0)
        res["compress_rotation_ms_median"], res["compress_rotation_ms_min"] = 1e3 * float(np.median(ts)), 1e3 * min(ts)
        rep = s.compress_rank(tol=a.tol)
        res["reduction"] = dict(tol=a.tol, ranks_before=[c["rank_before"] for c in rep["cones"]],
                                ranks_after=[c["rank_after"] for c in rep["cones"]], frob_lost=[c["frob_lost"] for c in rep["cones"]],
                                pobj_before=rep["pobj_before"], pobj_after=rep["pobj_after"], err1_before=rep["err1_before"],
                                err1_after=rep["err1_after"])
        if not a.quick:
            ips, out = _its_per_s(s, rho, rep["err1_after"], 40)
            res["admm_it_per_s_after"], res["err1_after_43_steps"] = ips, out[0]
        if rounding:
            s.round_pm1(trials=1024, seed=1, local_search_rounds=0, tol=0)
            t0 = time.perf_counter()
            s.round_pm1(trials=1024, seed=1, local_search_rounds=0, tol=0)
            res["round_K1024_ms_after"] = 1e3 * (time.perf_counter() - t0)
    finally:
        s.close()
        os.remove(path)
        os.rmdir(d)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
