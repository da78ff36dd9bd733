#!/usr/bin/env python3
"""Cost of Session.primal_entries / Session.primal_apply at a large instance's shape: --workload matcomp50000
(cfg5) at --timesLogRank, after phase 1 and --admm-steps ADMM iterations, the factor then padded with zero columns to --rank (the rank
the whole solve ends at: the gathers move the same bytes).  Warm (one call of each kind first), median of --reps:
  entries   --count random positions of the off-diagonal block without and with reference values, from (U + V) / 2 (four row gathers
            per entry) and from R (two: what averaging F once into a scratch would leave per entry, beside one streaming pass)
  apply     1, 16 and 64 random columns: the Python call on a C-ordered and on a column-major B, and the library call alone
  host      the same work through get_mat + numpy
and the gathered row bytes per second of the entry kernel's share (rocprofv3 --kernel-trace --stats gives the kernel alone).  Appends
one JSON line to --out.  Not part of bench.py.  --quick: one call per case (for a rocprofv3 run)."""
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


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="matcomp50000")
    ap.add_argument("--timesLogRank", type=float, default=5.5)
    ap.add_argument("--rank", type=int, default=135)
    ap.add_argument("--count", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--admm-steps", type=int, default=10)
    ap.add_argument("--phase1Tol", type=float, default=1e-2, help="as bench.py: 1e-2 ends phase 1 early")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "primal_time.jsonl"))
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    d = tempfile.mkdtemp(prefix="primal_time_")
    path = os.path.join(d, a.workload + ".dat-s")
    instances.write_sdpa(instances.NAMED[a.workload](), path)
    s = common.hip_session(path, timesLogRank=a.timesLogRank, phase1Tol=a.phase1Tol)
    res = {"workload": a.workload, "timesLogRank": a.timesLogRank, "phase1Tol": a.phase1Tol, "hip_source_sha256": bench.hip_source_hash()}
    try:
        t0 = time.time()
        s.alm()
        s.alm_to_admm()
        s.be.init_constr(host.PAIR_UV)
        err1 = s.be.update_dimacs(host.PAIR_UV)
        rho = min(s.results()["alm_rho"], 5000.0)
        s.admm_steps(a.admm_steps, rho, err1)
        ranks = [s.block_shape(k)[1] for k in range(s.nblk)]
        if a.rank > ranks[0]:
            s.be.resize_rank([a.rank] + ranks[1:])
        res["state"] = "after phase 1 and %d ADMM iterations, rank %d -> %d by zero columns" % (a.admm_steps, ranks[0], max(a.rank, ranks[0]))
        res["t_setup_s"] = time.time() - t0
        n, r = s.block_shape(0)
        res["shape"] = [n, r]
        rdev = r + (r & 1)
        n1 = n // 2
        rng = np.random.default_rng(1)
        rows = rng.integers(0, n1, a.count).astype(np.int32)
        cols = (n1 + rng.integers(0, n - n1, a.count)).astype(np.int32)
        ref = rng.standard_normal(a.count)
        be, UV, RR = s.be, host.PAIR_UV, host.PAIR_RR
        ent = {}
        for tag, src, gathers in (("uv", UV, 4), ("rr", RR, 2)):
            t_val = _median_ms(lambda: be.primal_entries(src, 0, rows, cols), reps)
            t_ref = _median_ms(lambda: be.primal_entries(src, 0, rows, cols, ref=ref), reps)
            t_score = _median_ms(lambda: be.primal_entries(src, 0, rows, cols, ref=ref, want_val=False), reps)
            gb = a.count * gathers * rdev * 8 / 1e9
            ent[tag] = dict(ms_val=t_val, ms_val_and_stats=t_ref, ms_stats_only=t_score, gathered_GB=gb,
                            call_TBps=gb / t_val, score_call_TBps=gb / t_score)
        res["entries"] = dict(count=a.count, **ent)
        v_dev, _ = s.primal_entries(0, rows, cols)
        # Session.primal_apply on a C-ordered B (numpy's default: the wrapper transposes it), on a column-major B, and the library call
        # alone on column-major buffers that exist and have been touched
        import ctypes as C
        dp = C.POINTER(C.c_double)
        ap_ms, ap_f, ap_lib, to_f = {}, {}, {}, {}
        for nc in (1, 16, 64):
            B = rng.standard_normal((n, nc))
            Bf, Y = np.asfortranarray(B), np.ones((n, nc), order="F")
            ap_ms[str(nc)] = _median_ms(lambda: s.primal_apply(0, B), reps)
            ap_f[str(nc)] = _median_ms(lambda: s.primal_apply(0, Bf), reps)
            ap_lib[str(nc)] = _median_ms(lambda: s.lib.lrd_session_primal_apply(s.h, 0, nc, Bf.ctypes.data_as(dp), Y.ctypes.data_as(dp), None), reps)
            to_f[str(nc)] = _median_ms(lambda: np.asfortranarray(B), reps)
        res["apply_ms"], res["apply_colmajor_ms"], res["apply_library_ms"], res["asfortranarray_ms"] = ap_ms, ap_f, ap_lib, to_f
        # the host route: the copy, then numpy
        t0 = time.perf_counter()
        F = (be.get_mat(host.MAT_U, 0) + be.get_mat(host.MAT_V, 0)) / 2
        t1 = time.perf_counter()
        v_host = np.einsum("ij,ij->i", F[rows], F[cols])
        t2 = time.perf_counter()
        hs = dict(get_mat=1e3 * (t1 - t0), entries=1e3 * (t2 - t1))
        for nc in (1, 16, 64):
            B = rng.standard_normal((n, nc))
            t0 = time.perf_counter()
            F @ (F.T @ B)
            hs["apply_%d" % nc] = 1e3 * (time.perf_counter() - t0)
        res["numpy_host_ms"] = hs
        res["entries_vs_numpy_abs"] = float(np.abs(v_dev - v_host).max())
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
