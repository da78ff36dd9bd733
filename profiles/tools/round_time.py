#!/usr/bin/env python3
"""Cost of Session.round_pm1 at cfg3a: maxcut20000, r = 40 (--timesLogRank 4.0), after phase 1 and a few ADMM
steps.  Times K in {64, 1024, 8192} with the local search off and on (median of --reps calls after one warm-up call each), and the
numpy model's signs + f on the host on the same state at K = 1024, for scale.  Prints one JSON object (and writes it to --out).
Not part of bench.py.  --quick: one call per case (for a rocprofv3 --kernel-trace --stats run)."""
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
from lorads_amd import instances  # noqa: E402
from tests import common  # noqa: E402
from tests import rounding_model as rm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--admm-steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    d = tempfile.mkdtemp(prefix="round_time_")
    path = os.path.join(d, "maxcut20000.dat-s")
    prob = instances.NAMED["maxcut20000"]()
    instances.write_sdpa(prob, path)
    s = common.hip_session(path, timesLogRank=4.0)
    res = {"workload": "maxcut20000 (cfg3a)", "hip_source_sha256": bench.hip_source_hash()}
    try:
        t0 = time.time()
        s.alm()
        s.alm_to_admm()
        res["t_phase1_s"] = time.time() - t0
        from lorads_amd import host
        s.be.init_constr(host.PAIR_UV)
        e0 = s.be.update_dimacs(host.PAIR_UV)
        s.admm_steps(a.admm_steps, 1.0, e0)
        res["rank"] = s.block_info(0)["rank"]
        cases = []
        for K in (64, 1024, 8192):
            for L in (0, 100):
                s.round_pm1(trials=K, seed=1, local_search_rounds=L, tol=0)  # warm-up (first use: check, colouring, scratch)
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    r = s.round_pm1(trials=K, seed=1, local_search_rounds=L, tol=0)
                    ts.append(time.perf_counter() - t0)
                cases.append(dict(K=K, L=L, ms_median=1e3 * float(np.median(ts)), ms_min=1e3 * min(ts), rounds=r.rounds,
                                  f_best=r.f_best, f_best0=r.f_best0))
                print(json.dumps(cases[-1]), flush=True)
        res["cases"] = cases
        t0 = time.perf_counter()
        r = s.round_pm1(trials=1024, seed=1, local_search_rounds=100, tol=1e-8)
        res["ms_K1024_L100_with_bound_tol1e-8"] = 1e3 * (time.perf_counter() - t0)
        res["bound"], res["f_best"] = r.bound, r.f_best
        if not a.quick:  # the numpy model on the host (signs and f, sparse C) on the same state
            import scipy.sparse as sp
            R = s.solution(tol=0).cones[0].R
            m, b, dims, ent = rm.read_sdpa(path)
            rows = [(i - 1, j - 1, -v) for mat, blk, i, j, v in ent if mat == 0]
            ii, jj, vv = (np.array(x) for x in zip(*rows))
            off = ii != jj
            Cs = sp.coo_matrix((np.concatenate([vv, vv[off]]), (np.concatenate([ii, jj[off]]), np.concatenate([jj, ii[off]]))),
                               shape=(dims[0], dims[0])).tocsr()
            t0 = time.perf_counter()
            G = rm.hyperplanes(1, 0, R.shape[1], 1024)
            t1 = time.perf_counter()
            X = np.where(R @ G >= 0, 1.0, -1.0)
            f = np.einsum("pt,pt->t", X, Cs @ X)
            t2 = time.perf_counter()
            res["numpy_model_K1024"] = dict(ms_hyperplanes=1e3 * (t1 - t0), ms_signs_and_f=1e3 * (t2 - t1),
                                             f_min=float(f.min()))
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
