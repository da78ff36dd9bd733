#!/usr/bin/env python3
"""bench.py -- ADMM iterations/s (+ inner CG iterations/s) of the low-rank ADMM hot path on MI355X.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 launched by
torch.distributed.run with one rank per GPU.  Prints ONE JSON line on rank 0.

Workload (BASELINE.json configs[2]): one dense-cone block n = 20000, r = 40
(--timesLogRank 4.0), m = 5000 random sparse A_i (2 diagonal + 8 off-diagonal entries each),
C = L/4 + I/4 of a 120000-edge random graph, b = A(R0 R0^T); generated with fixed seeds by
lorads_amd/instances.py.  N GPUs = N such blocks (block-diagonal SDP, block-separable constraints),
one block per GPU; the deal is block-separable, so every rank works on the sub-problem over its own constraints and ONE
all-reduce of four scalars per ADMM iteration is all the ranks share (weak scaling; LORADS_SEPARABLE=0: the general form, one
all-reduce of the shared m-vector).

A step = one ADMM iteration = admmUpdateVar (U- and V-solve by CG) + objective + dual objective +
DIMACS refresh + dual update (reference lorads_admm.c:76-81,120), with rho fixed at its hand-off
value and the CG tolerance min(1e-2 * err1, 1e-8) refreshed every iteration.  The factors come from
the solver's own phase 1 run on the GPU beforehand (untimed): --phase1Tol 1e-2 as in BASELINE.md.
Everything is resident in HBM when the timed region starts.
"""
import argparse
import atexit
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
DUMP_BYTES = 64 << 20  # --dump-outputs: the most all .npy files together may take


def traffic_from_profiles(workload):
    """The committed PMC summary of this workload (profiles/*_pmc_<workload>.json: fabric-side bytes per launch of the operator's
    and the front's kernels, collected with separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this same command; see
    profiles/pmc_summary.py) and its path"""
    best = None
    pdir = os.path.join(ROOT, "profiles")
    for f in sorted(os.listdir(pdir)) if os.path.isdir(pdir) else []:
        if f.endswith("_pmc_%s.json" % workload):
            best = os.path.join(pdir, f)
    if not best:
        return None, None
    with open(best) as fh:
        d = json.load(fh)
    return d, os.path.relpath(best, ROOT)


def rocprof_from_profiles(workload, op_kernels):
    """Average duration (ms) of one launch group (the kernels named in op_kernels, e.g. "k_front_cw" or "k_wsum+k_spmm_ell") according
    to the committed rocprofv3 --kernel-trace --stats summary of this same command (profiles/*_<workload>_kernel_stats.csv): sum over
    the kernels of the average of their most-called instantiation.  None if there is no such file."""
    import csv
    import re
    pdir = os.path.join(ROOT, "profiles")
    best = None
    # (the newest round's profile of the DEFAULT run: the kernels as the timed iterations launch them)
    for f in sorted(os.listdir(pdir)) if os.path.isdir(pdir) else []:
        if f.endswith("_%s_kernel_stats.csv" % workload) and "general_form" not in f:
            best = os.path.join(pdir, f)
    if not best:
        return None, None
    names = re.findall(r"k_\w+", op_kernels)
    tot = 0.0
    with open(best) as fh:
        rows = list(csv.DictReader(fh))
    for k in sorted(set(names)):
        # (a kernel named twice = two instantiations per application, e.g. the two sides of k_op_entry_bip: the two most-called rows)
        cand = sorted((r for r in rows if re.search(r"\b%s\b" % k, r["Name"])), key=lambda r: -int(r["Calls"]))
        if len(cand) < names.count(k):
            return None, None
        tot += sum(float(r["AverageNs"]) * 1e-6 for r in cand[:names.count(k)])
    return tot, os.path.relpath(best, ROOT)


def pin_to_gpu_numa(torch, dev_index):
    """One process per GPU, on the GPU's own socket: the host thread enqueues ~20 short kernels per ADMM iteration and
    polls a word in pinned memory for the result, so launch doorbells and that poll are latency-bound; from the far
    socket of the two-socket box a sharded ADMM iteration took 0.25 ms instead of 0.18 ms (profiles/tools/numa_probe.sh).
    Restricts the calling thread to the CPUs sysfs lists as local to the device (LORADS_NO_PIN=1: leave it alone).
    Returns the number of CPUs pinned to, 0 if nothing was done."""
    if os.environ.get("LORADS_NO_PIN") == "1":
        return 0
    try:
        p = torch.cuda.get_device_properties(dev_index)
        path = "/sys/bus/pci/devices/%04x:%02x:%02x.0/local_cpulist" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
        with open(path) as fh:
            txt = fh.read().strip()
        cpus = set()
        for part in txt.split(","):
            if "-" in part:
                lo, hi = part.split("-")
                cpus.update(range(int(lo), int(hi) + 1))
            elif part:
                cpus.add(int(part))
        target = cpus & os.sched_getaffinity(0)
        if not target or len(target) == len(os.sched_getaffinity(0)):
            return 0
        os.sched_setaffinity(0, target)
        return len(target)
    except Exception:  # noqa: BLE001  (no sysfs, no such attribute, not permitted: run unpinned)
        return 0


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def build_instance(name, path):
    from lorads_amd import instances
    if not os.path.exists(path):
        t0 = time.time()
        instances.write_sdpa(instances.NAMED[name](), path + ".tmp")
        os.replace(path + ".tmp", path)
        log("generated %s in %.1fs" % (name, time.time() - t0))
    return path


def replicate_blocks(path, nblk, out):
    """N identical blocks, constraint i of block k -> index k*m + i (block-separable)."""
    if os.path.exists(out):
        return out
    with open(path) as f:
        lines = f.read().split("\n")
    m = int(lines[0])
    n = int(lines[2].split()[0])
    b = lines[3].split()
    ents = [ln.split() for ln in lines[4:] if ln.strip()]
    with open(out + ".tmp", "w") as f:
        f.write("%d\n%d\n%s\n%s\n" % (m * nblk, nblk, " ".join([str(n)] * nblk), " ".join(b * nblk)))
        for k in range(nblk):
            for e in ents:
                mat = int(e[0])
                f.write("%d %d %s %s %s\n" % (mat if mat == 0 else mat + k * m, k + 1, e[2], e[3], e[4]))
    os.replace(out + ".tmp", out)
    return out


def write_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy in float64.  When all of them together would exceed DUMP_BYTES (with
    room for the .npy headers), every array of more than 16 values keeps the same seeded sample of its rows."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    big = [k for k, v in arrays.items() if v.size > 16]
    small = sum(v.nbytes for k, v in arrays.items() if k not in big)
    keep = min(1.0, (DUMP_BYTES - 4096 * len(arrays) - small) / max(1, sum(arrays[k].nbytes for k in big)))
    for k, v in arrays.items():
        if k in big and keep < 1.0:
            rows = np.random.default_rng(0).choice(v.shape[0], int(v.shape[0] * keep), replace=False)
            v = v[np.sort(rows)]
        np.save(os.path.join(out_dir, k + ".npy"), v)


def admm_steps(be, host, rho, err1, steps, session=None):
    """`steps` ADMM iterations through the operator table; returns (err1, cg_iters, pobj, dobj).
    With a session the loop itself runs in the C host (lrd_session_admm_steps), as it does in a solve."""
    if session is not None:
        return session.admm_steps(steps, rho, err1)
    cg = 0
    pobj = dobj = 0.0
    fused = be.has_admm_step
    for _ in range(steps):
        tol = min(err1 * 1e-2, 1e-8)
        if fused:   # same four calls behind one C-ABI entry with a single host sync
            c, pobj, dobj, err1 = be.admm_step(rho, tol, 800)
            cg += c
        else:
            cg += be.admm_update_var(rho, tol, 800)
            pobj = be.cal_obj(host.PAIR_UV)
            dobj = be.cal_dual_obj()
            err1 = be.update_dimacs(host.PAIR_UV)
        be.update_dual_var(rho)
    return err1, cg, pobj, dobj


def make_allreduce(dist, torch, device, ext_stream=None):
    """All-reduce hook for the library.  With `ext_stream` (the library's own HIP stream wrapped as a
    torch ExternalStream) the RCCL collective is enqueued in stream order -- no host synchronisation --
    otherwise the library has synchronised its stream and we synchronise after the collective."""
    class _Dev:
        def __init__(self, ptr, n):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}

    views = {}  # (address, count) -> tensor view of the library's buffer (the buffers live as long as the context)
    if ext_stream is not None:
        # the hook runs once per ADMM iteration between two kernel launches of the library: keep its host time small
        # (no per-call stream context, no per-call tensor construction) -- the library's stream simply IS this
        # process's current torch stream from here on
        torch.cuda.set_stream(ext_stream)

    def fn(ptr, count, on_device):
        if on_device:
            if ext_stream is not None:
                t = views.get((ptr, count))
                if t is None:
                    t = views[(ptr, count)] = torch.as_tensor(_Dev(ptr, count), device=device)
                dist.all_reduce(t)   # ordered after the kernels already on the stream; later kernels wait for it
            else:
                t = torch.as_tensor(_Dev(ptr, count), device=device)
                dist.all_reduce(t)
                torch.cuda.synchronize()
        else:
            a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(count,))
            t = torch.from_numpy(a.copy()).to(device)
            dist.all_reduce(t)
            a[:] = t.cpu().numpy()
    return fn


def install_native_rccl(s, dist, torch, device, world, rank):
    """Creates an RCCL communicator of our own (unique id from rank 0, shipped with torch.distributed) inside the RCCL
    PyTorch has already loaded, and registers liblorads_rccl.so's C function as the library's all-reduce hook.  Every
    rank learns whether ALL ranks succeeded (otherwise all fall back together).  Returns True on success."""
    from lorads_amd import host as _h
    # loading and binding happen INSIDE the agreed section: a rank that fails here reports ok = False through the MIN
    # all-reduce below instead of raising while the others are already in a collective
    lib, ok = None, False
    ident = C.create_string_buffer(128)
    try:
        lib = C.CDLL(os.path.join(_h.LIB_DIR, "liblorads_rccl.so"))
        lib.lorads_rccl_last_error.restype = C.c_char_p
        lib.lorads_rccl_comm_create.restype = C.c_void_p
        lib.lorads_rccl_comm_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        lib.lorads_rccl_comm_destroy.argtypes = [C.c_void_p]
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        ok = lib.lorads_rccl_open(path.encode() if os.path.exists(path) else b"") == 0
        if ok and rank == 0:
            ok = lib.lorads_rccl_unique_id(ident) == 0
    except Exception as e:  # noqa: BLE001
        log("rank %d: native RCCL hook: %s" % (rank, e))
        ok = False
    box = [bytes(ident.raw) if (ok and rank == 0) else None]
    dist.broadcast_object_list(box, src=0)
    # the communicator is created collectively: a rank that cannot take part (library or symbol missing) must be known to
    # all BEFORE anybody enters ncclCommInitRank, or the others would wait for it for ever
    ready = torch.tensor([1.0 if (ok and box[0] is not None) else 0.0], dtype=torch.float64, device=device)
    dist.all_reduce(ready, op=dist.ReduceOp.MIN)
    if ready.item() != 1.0:
        if not ok and lib is not None:
            log("rank %d: native RCCL hook: %s" % (rank, (lib.lorads_rccl_last_error() or b"").decode()))
        return False
    try:
        handle = lib.lorads_rccl_comm_create(box[0], rank, world, C.c_void_p(s.hip_stream()))
    except Exception as e:  # noqa: BLE001
        log("rank %d: native RCCL hook: %s" % (rank, e))
        handle = None
    flag = torch.tensor([1.0 if handle else 0.0], dtype=torch.float64, device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    torch.cuda.synchronize()
    if flag.item() != 1.0:
        if not handle:
            log("rank %d: native RCCL hook: %s" % (rank, (lib.lorads_rccl_last_error() or b"").decode()))
        else:
            lib.lorads_rccl_comm_destroy(handle)
        return False
    s.set_allreduce_native(C.cast(lib.lorads_rccl_allreduce_hook, C.c_void_p), handle)
    s.hip_allreduce_stream_ordered(1)
    s._rccl_native = (lib, handle)  # destroyed with the session (bench.py: before s.close())
    return True


def install_scalar_exchange(s, dist, torch, device, world, rank):
    """Separable shards on the GPUs of one node: the four scalars of an ADMM iteration's evaluation go from host to host through a
    page of shared memory (lorads_hip_set_scalar_exchange, csrc/host/shmx.c) -- no collective kernel between two iterations; the
    all-reduce hook stays for phase 1 and for the m-vector form.  Checked before use (the ranks' numbers 1..N must sum to N(N+1)/2
    on every rank); LORADS_SHM_EXCHANGE=0 keeps the collective.  Returns a word for the bench line."""
    if not getattr(s, "separable", False) or world < 2 or os.environ.get("LORADS_SHM_EXCHANGE", "1") == "0":
        return None
    if int(os.environ.get("LOCAL_WORLD_SIZE", world)) != world:     # ranks on several nodes: the collective
        return None
    # the segment's name: the same on every rank without a message (the rendezvous port is this run's own); rank 0 makes the segment
    # -- a leftover of that name goes first -- BEFORE the others open it
    name = "/lorads_%d_%s" % (os.getuid(), os.environ.get("MASTER_PORT", "0"))
    ok = 1.0
    try:
        if rank == 0:
            s.set_scalar_exchange_shm(name, world, rank)
    except Exception as e:  # noqa: BLE001
        log("rank %d: shared-memory scalar exchange not usable: %s" % (rank, e))
        ok = 0.0
    t = torch.tensor([ok], dtype=torch.float64, device=device)    # (doubles as the barrier between rank 0's create and the others' open)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    if t.item() != 1.0:
        return None
    try:
        if rank != 0:
            s.set_scalar_exchange_shm(name, world, rank)
    except Exception as e:  # noqa: BLE001
        log("rank %d: shared-memory scalar exchange not usable: %s" % (rank, e))
        ok = 0.0
    t = torch.tensor([ok], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    if t.item() == 1.0:      # every rank is attached: the ranks' numbers 1..N must sum to N(N+1)/2 on every rank
        try:
            got = s.shmx_allreduce([rank + 1.0, 1.0])
            if got != [world * (world + 1) / 2.0, float(world)]:
                ok = 0.0
        except Exception as e:  # noqa: BLE001
            log("rank %d: shared-memory scalar exchange failed its check: %s" % (rank, e))
            ok = 0.0
    else:
        ok = 0.0
    t = torch.tensor([ok], dtype=torch.float64, device=device)    # all ranks take the same branch
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    if t.item() != 1.0:
        s.clear_scalar_exchange()
        return None
    log("rank %d: evaluation scalars of separable shards: host exchange through shared memory %s" % (rank, name))
    return "host shared memory"


def install_allreduce(s, dist, torch, device, world, rank, backend):
    """Registers the hook; uses the stream-ordered form with RCCL after a self-check through the library
    (constrValSum filled with rank+1 must come back as world*(world+1)/2), else the synchronising form.
    Returns (mode, ranks_seen): ranks_seen = the N that solves N(N+1)/2 = what the library's own hook returned, so a
    run that silently has fewer ranks than --gpus cannot pass as N."""
    from lorads_amd import host as _h
    want = world * (world + 1) / 2.0
    seen = [0]

    def check():
        s.be.set_vec(_h.VEC_CONSTR_SUM, np.full(max(s.m, 1), rank + 1.0)[:s.m])
        s.hip_selfcheck_allreduce()
        got = s.be.get_vec(_h.VEC_CONSTR_SUM)
        g0 = float(got[0]) if len(got) else want
        seen[0] = int(round((np.sqrt(8.0 * g0 + 1.0) - 1.0) / 2.0))
        ok = torch.tensor([1.0 if np.all(got == want) else 0.0], dtype=torch.float64, device=device)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        return bool(ok.item() == 1.0)

    def drop_native():
        native = getattr(s, "_rccl_native", None)
        if native:
            s.hip_sync()
            native[0].lorads_rccl_comm_destroy(native[1])
            s._rccl_native = None

    mode = "sync"
    if backend == "nccl" and os.environ.get("LORADS_ALLREDUCE_SYNC", "0") != "1" and os.environ.get("LORADS_AR_TORCH") != "1":
        # first choice: the native hook (liblorads_rccl.so): ncclAllReduce on the library's own stream, no Python and no
        # second stream between two kernel launches of an ADMM iteration
        if install_native_rccl(s, dist, torch, device, world, rank) and check():
            return "rccl-native", seen[0]
        drop_native()
        log("rank %d: native RCCL hook not usable, trying torch.distributed in stream order" % rank)
    if backend == "nccl" and os.environ.get("LORADS_ALLREDUCE_SYNC", "0") != "1":
        try:
            ext = torch.cuda.ExternalStream(s.hip_stream(), device=device)
            s.set_allreduce(make_allreduce(dist, torch, device, ext))
            s.hip_allreduce_stream_ordered(1)
            okl = 1.0
        except Exception as e:  # noqa: BLE001
            log("stream-ordered all-reduce unavailable: %s" % e)
            okl = 0.0
        t = torch.tensor([okl], dtype=torch.float64, device=device)   # all ranks take the same branch
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        if t.item() == 1.0 and check():
            mode = "stream-ordered"
    if mode == "sync":
        s.hip_allreduce_stream_ordered(0)
        s.set_allreduce(make_allreduce(dist, torch, device, None))
        if not check():
            raise RuntimeError("all-reduce hook self-check failed")
    return mode, seen[0]


def cpu_baseline(path, tlr, rho, state_file, budget_s, log_fn, n_max=0, ranks=None):
    """Times the CPU path on the host cores, rank 0 / N = 1 only: the compiled reference
    (oracle/_ref, kind "reference") when it is present, else the plain-C restatement (kind "port").
    A cone with n^2 > 2^31 (cfg5) overflows the packed index of the reference's default 32-bit build
    (io/lorads_file_io.c:281): there the 64-bit build of the same sources (oracle/Makefile ref64: lorads_int = int64_t,
    MKL's ILP64 interface layer) is the one that can read the file."""
    wide = n_max * n_max > 2**31 - 1
    drv = os.path.join(ROOT, "oracle", "_ref", "ref_driver64" if wide else "ref_driver")
    env = dict(os.environ, MKL_NUM_THREADS="1", OMP_NUM_THREADS="1")
    if wide:
        env["MKL_INTERFACE_LAYER"] = "ILP64"
    if ranks:   # the device's phase 1 may have grown the ranks (AUG_RANK): the reference must load factors of that shape
        env["LORADS_REF_UV_RANKS"] = ",".join(str(int(r)) for r in ranks)
    if os.path.exists(drv):
        try:
            its = 2
            for attempt in range(2):
                t0 = time.time()
                r = subprocess.run([drv, path, "admmbench", "-", "--timesLogRank", repr(tlr), "--rho", repr(rho), "--uv", state_file,
                                    "--nADMM", str(its)], env=env, capture_output=True, text=True, timeout=900)
                wall = time.time() - t0
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("@@REF_ADMM_BENCH")]
                if r.returncode != 0 or not line:
                    raise RuntimeError("ref_driver failed: " + r.stderr[-500:])
                kv = dict(x.split("=") for x in line[0].split()[1:])
                sec = float(kv["seconds"])
                if attempt == 0 and sec < budget_s / 3:
                    its = int(max(2, min(64, its * budget_s / 2 / max(sec, 1e-3))))
                    continue
                break
            log_fn("cpu reference: %d ADMM its in %.2fs (setup+run wall %.1fs), %s CG its" % (its, sec, wall, kv["cg_iters"]))
            return {"value": its / sec, "unit": "ADMM iters/s", "cores": 1, "kind": "reference",
                    "cg_iters_per_s": int(kv["cg_iters"]) / sec,
                    # where the reference stands after those iterations (compared with the device path below)
                    "check": {"iterations": its, "cg_iters": int(kv["cg_iters"]), "pObj": float(kv["pObj"]),
                              "dObj": float(kv["dObj"]), "err1": float(kv["err1"])},
                    "sample": "%d ADMM iterations (%s CG iterations) of the same workload from the state the device run has reached, "
                              "compiled reference%s (MKL sequential, 1 thread) on the host"
                              % (its, kv["cg_iters"], ", 64-bit lorads_int build" if wide else "")}
        except Exception as e:  # noqa: BLE001
            log_fn("reference baseline unavailable (%s); timing the C restatement" % e)
    from lorads_amd import host
    from tests import common
    s = common.oracle_session(path, timesLogRank=tlr)
    try:
        raw = np.fromfile(state_file, dtype=np.float64)
        o = 0
        if ranks and [s.block_shape(k)[1] for k in range(s.nblk)] != list(ranks):
            s.be.resize_rank(list(ranks))
        for k in range(s.nblk):
            n, r = s.block_shape(k)
            s.be.set_mat(host.MAT_U, k, raw[o:o + n * r].reshape(r, n).T)
            s.be.set_mat(host.MAT_V, k, raw[o + n * r:o + 2 * n * r].reshape(r, n).T)
            o += 2 * n * r
        s.be.set_vec(host.VEC_LAMBDA, raw[o:o + s.m])
        s.be.init_constr(host.PAIR_UV)
        s.be.cal_obj(host.PAIR_UV)
        err1 = s.be.update_dimacs(host.PAIR_UV)
        its, t0 = 0, time.time()
        cg = 0
        while time.time() - t0 < budget_s / 2 and its < 64:
            err1, c, _, _ = admm_steps(s.be, host, rho, err1, 1)
            cg += c
            its += 1
        sec = time.time() - t0
    finally:
        s.close()
    return {"value": its / sec, "unit": "ADMM iters/s", "cores": 1, "kind": "port", "cg_iters_per_s": cg / sec,
            "sample": "%d ADMM iterations (%d CG iterations) of the same workload from the state the device run has reached, "
                      "plain-C restatement (oracle/) on 1 host core" % (its, cg)}


def parity_sharded(s, path, tlr, rho, dist, torch, device, world, rank, host, iters=5):
    """The sharded run against the SINGLE-RANK run of the same problem from the same state: every rank re-installs
    its own (U, V, lambda), evaluates and runs `iters` ADMM iterations with the cross-rank sums of this run; rank 0 then opens the whole
    problem on its own GPU, loads the ranks' state into it and runs the same iterations.  Block-separable constraints: the ranks'
    Jacobi sweep is the single rank's Gauss-Seidel sweep, so the CG iteration counts must be EQUAL and the objectives
    agree to 1e-10.  Returns the block for the JSON line (rank 0; None elsewhere); "ok" is what the exit code follows."""
    be = s.be
    nloc = s.nblk
    UV = [(be.get_mat(host.MAT_U, j), be.get_mat(host.MAT_V, j)) for j in range(nloc)]
    lam = be.get_vec(host.VEC_LAMBDA)
    ranks_loc = [s.block_info(j)["rank"] for j in range(nloc)]

    def run(sess, mats, lam_vec):
        b = sess.be
        for j, (U, V) in enumerate(mats):
            b.set_mat(host.MAT_U, j, U)
            b.set_mat(host.MAT_V, j, V)
        b.set_vec(host.VEC_LAMBDA, lam_vec)
        b.init_constr(host.PAIR_UV)
        b.cal_obj(host.PAIR_UV)
        e0 = b.update_dimacs(host.PAIR_UV)
        e1, cg, p, d = admm_steps(b, host, rho, e0, iters, sess)
        return e0, e1, int(cg), p, d

    e0, e1, cg, p, d = run(s, UV, lam)
    t = torch.tensor([float(cg)], dtype=torch.float64, device=device)
    dist.all_reduce(t)
    cg_all = int(t.item())
    box = [None] * world
    dist.gather_object((rank, UV, lam, np.asarray(s.constraint_map), ranks_loc), box if rank == 0 else None, dst=0)
    out = None
    if rank == 0:
        try:
            one = host.Session.open(path)
            one.set_params(verbose=0, timesLogRank=tlr, phase1Tol=1e-2, reoptLevel=0)
            one.prepare(1, 0, separable=False)
            one.attach_hip()
            try:
                nb = one.nblk
                mats, rk = [None] * nb, [None] * nb
                lam_all = np.zeros(one.m)
                for (r_, uv, lm, cmap, rl) in box:
                    for j, m_ in enumerate(uv):      # cones are dealt round robin: local cone j of rank r is cone r + j * world of the file
                        mats[r_ + j * world] = m_
                        rk[r_ + j * world] = rl[j]
                    lam_all[cmap] = lm
                if [one.block_info(k)["rank"] for k in range(nb)] != rk:   # (phase 1 has grown the ranks: AUG_RANK)
                    one.be.resize_rank(rk)
                f0, f1, cg1, p1, d1 = run(one, mats, lam_all)
            finally:
                one.close()
            rel = lambda x, y: abs(x - y) / (1.0 + abs(y))  # noqa: E731
            out = {"what": "%d ADMM iterations from the same (U, V, lambda): %d ranks against ONE rank holding the whole problem" % (iters, world),
                   "iterations": iters, "cg_iters_sharded": cg_all, "cg_iters_single_rank": cg1,
                   "pObj_sharded": p, "pObj_single_rank": p1, "pObj_rel_diff": rel(p, p1),
                   "dObj_sharded": d, "dObj_single_rank": d1, "dObj_rel_diff": rel(d, d1),
                   "err1_start_sharded": e0, "err1_start_single_rank": f0, "err1_sharded": e1, "err1_single_rank": f1}
            out["ok"] = bool(cg_all == cg1 and out["pObj_rel_diff"] <= 1e-10 and out["dObj_rel_diff"] <= 1e-10 and
                             abs(e1 - f1) <= 1e-6 * abs(f1) + 1e-13)
        except Exception as e:  # noqa: BLE001
            out = {"ok": False, "what": "failed: %s" % e}
    dist.barrier()
    return out


def hip_source_hash():
    """sha256 over the HIP sources the kernels are built from (what a committed profile must have been taken from)"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "lorads_amd", "csrc", "hip")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".inc", ".cpp")):
            with open(os.path.join(d, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()


def profile_stamp_ok(relpath):
    """A committed profile file may be replayed into the JSON line only if the stamp written next to it when it was
    collected (profiles/<round>_stamp.json: hash of the HIP sources, git head) matches the sources of THIS run."""
    rnd = os.path.basename(relpath).split("_")[0]
    stamp = os.path.join(ROOT, "profiles", "%s_stamp.json" % rnd)
    if not os.path.exists(stamp):
        return False, None
    with open(stamp) as fh:
        st = json.load(fh)
    return st.get("hip_source_sha256") == hip_source_hash(), st.get("git_head")


def run_workload(a, workload, torch, dist, device, world, rank, host, with_cpu, workdir, tlr=None, dump=None):
    """One workload: untimed phase 1, then the timed ADMM steps.  Every rank writes its own copy of the seeded instance into
    `workdir` (this process's own directory), so the input depends on the arguments alone.  With `dump` (a dict) rank 0 adds
    what the timed path computed in its last step."""
    tlr = a.times_log_rank if tlr is None else tlr
    strong = a.scaling == "strong"
    path = build_instance(workload, os.path.join(workdir, "%s.dat-s" % workload))
    if world > 1 and not strong:
        path = replicate_blocks(path, world, os.path.join(workdir, "%s_x%d.dat-s" % (workload, world)))
    if dist:
        dist.barrier()

    t_setup0 = time.time()
    s = host.Session.open(path)
    s.set_params(verbose=0, timesLogRank=tlr, phase1Tol=1e-2, reoptLevel=0)
    if workload == "matcomp50000" and os.environ.get("LORADS_BENCH_RANK_GROWTH") != "1":
        # BASELINE cfg5 names r = 60: with the default rank-growth rule phase 1 takes this instance to r = 90 before the timed
        # ADMM iterations start (LORADS_BENCH_RANK_GROWTH=1: let it)
        s.set_params(dyrankLevel=0)
    # cones dealt round-robin over the ranks; a block-separable deal (both workloads here) leaves each rank the sub-problem over
    # its own constraints, and the ranks share four scalars per ADMM iteration instead of the m-vector (LORADS_SEPARABLE=0: that)
    # (LORADS_FORCE_DIST=1: the sharded code path on ONE rank -- the form's own cost, hook included -- takes the separable form too)
    s.prepare(world, rank, separable=dist is not None and os.environ.get("LORADS_SEPARABLE", "1") != "0")
    t_setup1 = time.time()
    s.attach_hip()
    t_setup2 = time.time()
    ar_mode, ranks_seen, sx_mode = None, 1, None
    if dist:
        ar_mode, ranks_seen = install_allreduce(s, dist, torch, device, world, rank, os.environ.get("LORADS_DIST_BACKEND", "nccl"))
        log("rank %d: all-reduce hook mode: %s, ranks seen through the library's hook: %d" % (rank, ar_mode, ranks_seen))
        sx_mode = install_scalar_exchange(s, dist, torch, device, world, rank)
    be = s.be
    info = s.block_info(0)
    nloc = s.nblk
    # ---- untimed set-up: phase 1 on the GPU gives the factors, then the hand-off
    # (the counting window is opened in front of phase 1: opening it creates the event pool, tens of milliseconds in which the GPU idles
    # and clocks down -- between phase 1 and the warm-up that idle time showed in the first timed steps; the timed region's counts are
    # differences of two reads.  With --sample-every the window opens after phase 1, whose applications would use up the pool.)
    prof_early = a.sample_every <= 0
    if prof_early:
        s.hip_profile(1, 1 << 30)
    t0 = time.time()
    s.hip_sync()
    n_l0 = s.hip_launch_count()
    t_p1 = time.perf_counter()
    s.alm()
    s.hip_sync()
    t_p1 = time.perf_counter() - t_p1
    n_l_p1 = s.hip_launch_count() - n_l0
    s.alm_to_admm()
    res = s.results()
    rho = min(res["admm_rho"] if res["admm_rho"] > 0 else res["alm_rho"], 5000.0)
    be.init_constr(host.PAIR_UV)
    be.cal_obj(host.PAIR_UV)
    err1 = be.update_dimacs(host.PAIR_UV)
    r_start = info["rank"]
    info = s.block_info(0)   # (phase 1 may have grown the rank)
    log("rank %d: phase 1 took %.2fs (%d inner its), rho=%.4g err1=%.3e, %d local cone(s), n=%d r=%d" %
        (rank, time.time() - t0, int(res["alm_inner"]), rho, err1, nloc, info["n"], info["rank"]))
    state_file = os.path.join(workdir, "state_%s.bin" % workload)
    # (the state the CPU reference and the full-size parity check start from is taken AFTER the timed region and its untimed passes:
    # fetching the factors and writing them out idles the GPU for tens of milliseconds, and taken here -- right in front of the warm-up
    # -- that idle time showed in the timed steps as a clock ramp: 0.127 against 0.124 ms per step)

    # ---- warm-up, then exactly K timed steps
    if not prof_early:
        s.hip_profile(1, a.sample_every if a.sample_every > 0 else 1 << 30)
    err1, _, _, _ = admm_steps(be, host, rho, err1, a.warmup, s)
    prof0 = s.hip_profile_read()
    n_samp0 = len(s.hip_profile_samples())
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    n_l0 = s.hip_launch_count()
    t0 = time.perf_counter()
    err1, cg_iters, pobj, dobj = admm_steps(be, host, rho, err1, a.steps, s)
    s.hip_sync()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    n_l_timed = s.hip_launch_count() - n_l0
    prof = s.hip_profile_read()
    for k_ in ("matvec_launches", "speculation_misses", "cg_iters", "cg_solves", "sampled", "sampled_ms", "spmm_sampled", "spmm_sampled_ms"):
        prof[k_] -= prof0[k_]
    samples_timed = s.hip_profile_samples()[n_samp0:]
    s.hip_profile(0, 1)
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        c = torch.tensor([float(cg_iters)], dtype=torch.float64, device=device)
        dist.all_reduce(c)
        cg_iters = int(c.item())
    if dump is not None and rank == 0:
        # the state the timed steps leave (rank 0's cones and multipliers) and the last step's scalars, before anything else runs
        for k in range(nloc):
            dump["%s_U%d" % (workload, k)] = be.get_mat(host.MAT_U, k)
            dump["%s_V%d" % (workload, k)] = be.get_mat(host.MAT_V, k)
        dump["%s_lambda" % workload] = be.get_vec(host.VEC_LAMBDA)
        dump["%s_scalars" % workload] = np.array([pobj, dobj, err1, cg_iters], dtype=np.float64)  # pObj, dObj, err1, CG its of the timed steps
    # ---- further windows of K steps each (outside the contract's timed region): spread of ms_per_step
    win_ms = [1e3 * elapsed / a.steps]
    for _ in range(max(0, a.windows - 1)):
        if dist:
            dist.barrier()
        s.hip_sync()
        tw = time.perf_counter()
        err1, _, _, _ = admm_steps(be, host, rho, err1, a.steps, s)
        s.hip_sync()
        if dist:
            dist.barrier()
        w = time.perf_counter() - tw
        if dist:
            t = torch.tensor([w], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            w = float(t.item())
        win_ms.append(1e3 * w / a.steps)
    # ---- untimed roofline pass: the launches the timed iterations make anyway, between two HIP events each, until enough samples
    # exist -- first every CG operator application, then every solve front (right-hand side + initial residual) -- and the live
    # operator back to back with nothing riding along (boundaries included, no event latency).  Nothing runs differently
    # because it is timed.
    roof_samples, front_samples, alone_ms = [], [], None
    fronts_per_step = 2.0 * nloc
    pstat = s.hip_persist_stats()
    one_launch = pstat["available"] == 1 and pstat["iterations"] > 0   # (the whole iteration is one launch: that launch is what is timed)
    if a.roofline_samples > 0:
        per_step = prof["matvec_launches"] / max(a.steps, 1)
        if dist:   # every rank must run the same number of (collective-carrying) iterations
            t = torch.tensor([per_step], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            per_step = float(t.item())
        per_step = max(per_step, 0.25)
        for target, per, sink in ((0, 1.0 if one_launch else per_step, roof_samples), (1, fronts_per_step, front_samples)):
            if one_launch and target == 1:
                continue
            todo = int(min(4000, np.ceil(a.roofline_samples / per))) + 2
            chunk = int(max(1, min(todo, 600 // max(1.0, 1.5 * per))))  # (event pool: 1024 samples)
            s.hip_profile_target(target)
            s.hip_profile(1, 1)
            while todo > 0:
                err1, _, _, _ = admm_steps(be, host, rho, err1, min(chunk, todo), s)
                sink.extend(s.hip_profile_samples())   # (drains the event pool)
                todo -= chunk
            s.hip_profile(0, 1)
        s.hip_profile_target(0)
        try:
            reps = 200
            alone_ms = None if one_launch else s.hip_time_operator(reps) / reps
        except Exception as e:  # noqa: BLE001
            log("rank %d: back-to-back operator run unavailable: %s" % (rank, e))
    b_mv = b_cg = 0.0
    for k in range(nloc):
        x, y = s.hip_algorithmic_bytes(k)
        b_mv += x
        b_cg += y
    op_kernels = s.hip_operator_kind(0)
    out = None
    if rank == 0:
        # weak: N blocks, every ADMM iteration of the N-block problem advances N blocks -> block-iterations / s (equal to
        # iterations / s at N = 1); strong: ONE problem -> iterations / s
        units = a.steps if strong else world * a.steps
        med = lambda v: float(np.median(v)) if len(v) else None  # noqa: E731
        cfg_txt = ("%s: %d cone(s) of n=%d r=%d dealt over %d GPU(s) (%d on rank 0)" % (workload, s.nblk_global, info["n"], info["rank"], world, nloc)
                   if strong else
                   "%s: %d block(s) n=%d r=%d, %d constraints/block, NA=%d, NC=%d; one block per GPU"
                   % (workload, world, info["n"], info["rank"], info["nrow"], info["na"], info["nc"]))
        out = {
            "metric": "ADMM iters/sec (+ inner CG-iters/sec), single-block n=20000 r=40" if workload == "rand20000"
                      else "ADMM iters/sec (+ inner CG-iters/sec), %s" % workload,
            "value": units / elapsed,
            "unit": "ADMM iters/s" if (strong or world == 1) else "ADMM block-iters/s (N blocks x iterations / s)",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": 1e3 * elapsed / a.steps,
            "ms_per_step_windows": win_ms, "ms_per_step_median": med(win_ms),
            "higher_is_better": True, "scaling": a.scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "ranks_seen": ranks_seen,
            "scalar_exchange": sx_mode,
            "admm_iters_per_s_of_the_sharded_problem": a.steps / elapsed,
            "speculation_misses_in_timed_region": int(prof["speculation_misses"]),   # (solves resumed after a host round trip)
            "cg_iters_per_s": cg_iters / elapsed,
            "cg_iters_per_admm_iter": cg_iters / units,
            "config": {"workload": cfg_txt,
                       "n": info["n"], "r": info["rank"], "r_at_start": r_start, "m_per_block": info["nrow"], "blocks": s.nblk_global,
                       "parallelism": ("%s, 1 all-reduce of %s per ADMM iteration (%s)"
                                       % ("cones dealt over the ranks" if strong else "block-per-GPU",
                                          "four scalars (separable shards: every rank holds its own constraints)" if s.separable
                                          else "the shared m-vector", ar_mode)) if world > 1 else "single GPU",
                       "separable_shards": bool(s.separable) if dist is not None else None,
                       "flags": "--timesLogRank %g --phase1Tol 1e-2 (phase 1 untimed), fixed rho=%.6g" % (tlr, rho)},
            "state": {"pObj": pobj, "dObj": dobj, "err1_end": err1},
            # start-up cost, untimed: reader + host pre-solve (rank rule, start point), then the device image
            # (patterns, adjacency, slot lists, uploads) built inside lorads_hip_create
            "setup_seconds": {"read_and_presolve_host": t_setup1 - t_setup0, "device_image_in_create": t_setup2 - t_setup1},
            "roofline": None,
            # BM / ALM warm start (phase 1; lorads_alm.c:1066-1131), untimed by the contract, reported beside it: the
            # solver's own phase 1 on the GPU from the reference's start point to --phase1Tol 1e-2
            "phase1": None if not res["alm_inner"] else {
                "inner_iters": int(res["alm_inner"]), "outer_iters": int(res["alm_outer"]), "seconds": t_p1,
                "inner_iters_per_s": res["alm_inner"] / t_p1, "us_per_inner_iter": 1e6 * t_p1 / res["alm_inner"],
                # (every kernel of phase 1 -- the outer iterations' own few included -- over its inner iterations)
                "launches_per_inner_iter": n_l_p1 / res["alm_inner"],
                "one_launch_direction": s.hip_lbfgs_team_stats()},
            "launches_per_step": n_l_timed / max(a.steps, 1),
            "one_launch_iteration": None if not one_launch else {
                "what": "every cone of Max-Cut type: one launch per ADMM iteration, teams of resident workgroups (csrc/hip/persist.inc)",
                "workgroups": pstat["workgroups"], "rows_per_lane_group": pstat["rows"], "column_steps": pstat["column_steps"],
                "lds_bytes_per_workgroup": pstat["lds_bytes"]},
        }
        # ---- roofline of the DOMINANT kernel of the timed iterations, from the launches those iterations make (events on the
        # library's stream, untimed pass): algorithmic bytes per launch / median launch duration / 8 TB/s
        F = 8.0 * info["n"] * info["rank"] * nloc
        na, nc, m_ = info["na"] * nloc, info["nc"] * nloc, info["nrow"] * nloc
        b_rhs = 16.0 * (nc + na) + 8.0 * m_ + 3.0 * F           # assemble S, S V, fuse -rho V and 1 / rho
        b_half = 2.0 * F + 16.0 * na + 8.0 * m_                 # the A(sym(x V^T)) half of an operator application
        stat = lambda v: None if not v else {  # noqa: E731
            "launches_timed": len(v), "event_ms_median": med(v), "event_ms_mean": float(np.mean(v)),
            "event_ms_p10_p90": [float(np.percentile(v, 10)), float(np.percentile(v, 90))]}
        op_ms, fr_ms = med(roof_samples), med(front_samples)
        cw_front = op_kernels.startswith("k_cw")   # (the one-kernel front also leaves iteration 0's constraint-value contributions)
        groups = {}
        if one_launch and op_ms:
            # the whole ADMM iteration is ONE launch (k_admm_diag): its algorithmic bytes are SURVEY 8d's per-iteration sum with the CG
            # iteration counts this run measured -- solves (K + 1 + ceil(K / 20)) B_mv + 9 F K + 3 F each, two right-hand sides, four
            # constraint evaluations, the objective, the m-vector passes -- although most of them never leave the chip here
            k_loc = cg_iters / max(a.steps, 1) / world   # CG iterations per ADMM iteration in this rank's cones (average over the ranks)
            b_obj = 3.0 * F + 16.0 * nc
            b_iter = b_mv * (k_loc / nloc + 4.0) + 9.0 * (F / nloc) * k_loc + 6.0 * F + 2.0 * b_rhs + 4.0 * b_half + b_obj + 32.0 * m_
            groups["admm_iteration_one_launch"] = {
                "kernel": "k_admm_diag: fronts, CG solves, constraint refresh, evaluation and hand-over of one ADMM iteration in one launch",
                "algorithmic_bytes_per_launch": b_iter, "avg_launch_ms": op_ms, "achieved": b_iter / (op_ms * 1e-3) / 1e9,
                "frac": b_iter / (op_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "launches_per_step": 1.0, "events": stat(roof_samples),
                "bytes": "SURVEY 8d per-iteration sum at %.2f CG iterations per iteration: the bytes the launch-by-launch algorithm "
                         "moves; the factors stay in registers here, so the launch's own HBM traffic (PMC) is a fraction of it" % k_loc}
        elif op_ms:
            groups["cg_operator"] = {
                "kernel": "CG operator application x + A_V^*(A_V x) as the iterations run it: %s" %
                          ("k_wsum + k_spmm_ell (iteration 0: the constraint values come out of the front), k_cw + k_spmm_ell otherwise"
                           if cw_front else op_kernels),
                "algorithmic_bytes_per_launch": b_mv, "avg_launch_ms": op_ms, "achieved": b_mv / (op_ms * 1e-3) / 1e9,
                "frac": b_mv / (op_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "launches_per_step": prof["matvec_launches"] / max(a.steps, 1),
                "events": stat(roof_samples),
                "alone_back_to_back": None if alone_ms is None else {
                    "avg_ms": alone_ms, "frac": b_mv / (alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "what": "200 applications of the live operator (general form) back to back between ONE event pair, no scalar "
                            "step riding along (kernel boundaries included, no per-sample event latency)"}}
        if fr_ms:
            fb = b_rhs + b_mv + (b_half if cw_front else 0.0)
            groups["solve_front"] = {
                "kernel": ("k_front_cw: rhs = V - (C + sum M1_i A_i) V / rho, initial residual, and the slot contributions of "
                           "A(sym(r0 V^T)) (iteration 0's constraint values)" if cw_front else
                           "front of a CG solve: right-hand side and initial residual in one pass (k_spmm2<FRONT> / k_sval + k_spmm2 + operator)"),
                "algorithmic_bytes_per_launch": fb, "avg_launch_ms": fr_ms, "achieved": fb / (fr_ms * 1e-3) / 1e9,
                "frac": fb / (fr_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "launches_per_step": fronts_per_step,
                "bytes": "B_rhs + B_mv%s (SURVEY 8d)" % (" + half of B_mv" if cw_front else ""), "events": stat(front_samples)}
        share = {k: g["avg_launch_ms"] * g["launches_per_step"] for k, g in groups.items()}
        dom = max(share, key=share.get) if share else None
        if dom:
            g = groups[dom]
            out["roofline"] = {"bound": "hbm", "kernel": g["kernel"], "achieved": g["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": g["frac"], "algorithmic_bytes_per_launch": g["algorithmic_bytes_per_launch"],
                               "avg_launch_ms": g["avg_launch_ms"], "traffic": None,
                               "dominant": "%s: %.1f %% of the step (%.1f us x %.1f launches of %.1f us)" %
                                           (dom, 100 * share[dom] / (1e3 * elapsed / a.steps) if elapsed else 0.0, 1e3 * g["avg_launch_ms"],
                                            g["launches_per_step"], 1e6 * elapsed / a.steps),
                               "how": "median over %d launches, each between two HIP events on the library's stream, in an untimed pass "
                                      "after the timed region that runs the same iterations (events add ~1-3 us of marker latency per "
                                      "sample); the kernel group with the largest share of the step" % g["events"]["launches_timed"],
                               "in_timed_region": {"launches_timed": int(prof["sampled"]), "launches_total": int(prof["matvec_launches"])},
                               "cg_iter_bytes": b_cg,
                               "cg_iter_frac_of_hbm": (b_cg * cg_iters / world / elapsed / 1e9 / HBM_PEAK_GBS),
                               "groups": groups}
        else:
            out["roofline"] = {"bound": "hbm", "kernel": None, "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None,
                               "traffic": None, "how": "no launches were timed (--roofline-samples 0)", "cg_iter_bytes": b_cg,
                               "cg_iter_frac_of_hbm": (b_cg * cg_iters / world / elapsed / 1e9 / HBM_PEAK_GBS)}
        # committed rocprofv3 / PMC summaries of this same command: replayed ONLY when their stamp matches the HIP sources
        # of this run (a profile of older kernels is not this run's evidence)
        if dom:
            pm, tsrc = traffic_from_profiles(workload)
            tr = (pm or {}).get({"solve_front": "solve_front", "admm_iteration_one_launch": "admm_iteration_one_launch"}.get(dom, "cg_operator_application"), {}).get("traffic_bytes")
            dom_kernels = "k_admm_diag" if dom == "admm_iteration_one_launch" else \
                          ("k_front_cw" if cw_front else "k_spmm2") if dom == "solve_front" else \
                          ("k_wsum+k_spmm_ell" if cw_front else op_kernels)
            pms, psrc = rocprof_from_profiles(workload, dom_kernels)
            for val, src, key in ((tr, tsrc, "traffic"), (pms, psrc, "rocprofv3")):
                if val is None:
                    continue
                ok, head = profile_stamp_ok(src)
                if not ok:
                    out["roofline"][key + "_source"] = "%s is stale (HIP sources changed since it was collected): not replayed" % src
                    continue
                if key == "traffic":
                    out["roofline"]["traffic"] = val
                    out["roofline"]["traffic_source"] = "%s (committed, collected at %s from these sources; not measured in this run)" % (src, head)
                else:
                    out["roofline"]["rocprofv3_avg_launch_ms"] = val
                    out["roofline"]["rocprofv3_frac"] = out["roofline"]["algorithmic_bytes_per_launch"] / (val * 1e-3) / 1e9 / HBM_PEAK_GBS
                    out["roofline"]["rocprofv3_source"] = "%s (committed, collected at %s from these sources; not measured in this run)" % (src, head)
        if world == 1 and with_cpu:
            try:
                UV0 = [(be.get_mat(host.MAT_U, k), be.get_mat(host.MAT_V, k)) for k in range(nloc)]
                lam0 = be.get_vec(host.VEC_LAMBDA)
                with open(state_file, "wb") as f:
                    for U, V in UV0:
                        f.write(np.asfortranarray(U).tobytes(order="F"))
                        f.write(np.asfortranarray(V).tobytes(order="F"))
                    f.write(lam0.tobytes())
                cb = cpu_baseline(path, tlr, rho, state_file, a.cpu_budget, log, n_max=info["n"],
                                  ranks=[s.block_info(k)["rank"] for k in range(nloc)])
                cb["host_cores_total"] = os.cpu_count()
                try:
                    with open("/proc/cpuinfo") as fh:
                        cb["host_cpu_model"] = next(l.split(":", 1)[1].strip() for l in fh if l.startswith("model name"))
                except Exception:  # noqa: BLE001
                    cb["host_cpu_model"] = None
                out["cpu_baseline"] = cb
                out["speedup_vs_cpu_1core"] = out["value"] / cb["value"]
                # (advisor r3: the CPU sample starts from the state the device has REACHED, where an ADMM iteration may hold another
                # number of CG iterations than in the timed window: the ratio of CG iterations per second compares like with like)
                if cb.get("cg_iters_per_s"):
                    out["speedup_vs_cpu_1core_cg_normalised"] = out["cg_iters_per_s"] / cb["cg_iters_per_s"]
                chk = cb.pop("check", None)
                if chk:
                    # parity at the full size: the device path replays the same number of ADMM iterations from the very
                    # state the reference started from (same rho, same tolerance rule) and must stand where it stands
                    for k, (U, V) in enumerate(UV0):
                        be.set_mat(host.MAT_U, k, U)
                        be.set_mat(host.MAT_V, k, V)
                    be.set_vec(host.VEC_LAMBDA, lam0)
                    be.init_constr(host.PAIR_UV)
                    be.cal_obj(host.PAIR_UV)
                    e0 = be.update_dimacs(host.PAIR_UV)
                    e1, cg1, p1, d1 = admm_steps(be, host, rho, e0, chk["iterations"], s)
                    rel = lambda x, y: abs(x - y) / (1.0 + abs(y))  # noqa: E731
                    out["parity_full_size"] = {
                        "what": "%d ADMM iterations from the same (U, V, lambda), reference (CPU) vs this path (GPU)" % chk["iterations"],
                        "pObj_ref": chk["pObj"], "pObj_gpu": p1 / 1.0, "pObj_rel_diff": rel(p1, chk["pObj"]),
                        "dObj_ref": chk["dObj"], "dObj_gpu": d1 / 1.0, "dObj_rel_diff": rel(d1, chk["dObj"]),
                        "err1_ref": chk["err1"], "err1_gpu": e1, "cg_iters_ref": chk["cg_iters"], "cg_iters_gpu": int(cg1)}
            except Exception as e:  # noqa: BLE001
                out["cpu_baseline"] = {"value": None, "unit": "ADMM iters/s", "cores": 1, "kind": "port", "sample": "failed: %s" % e}
            finally:
                if os.path.exists(state_file):
                    os.remove(state_file)
        else:
            out["cpu_baseline"] = {"value": None, "unit": "ADMM iters/s", "cores": 0, "kind": "reference",
                                   "sample": "timed at N=1 only"}
    if dist and world > 1 and s.separable and os.environ.get("LORADS_BENCH_PARITY", "1") != "0":
        ps = parity_sharded(s, path, tlr, rho, dist, torch, device, world, rank, host)
        if out is not None:
            out["parity_sharded"] = ps
    if os.environ.get("LORADS_PRINT_CPU"):
        with open("/proc/self/stat") as fh:
            cpu_now = int(fh.read().rsplit(")", 1)[1].split()[36])
        log("rank %d: cpu at end %d, affinity %d cpus" % (rank, cpu_now, len(os.sched_getaffinity(0))))
    if dist:  # (the hook made the library's stream this process's current torch stream: hand torch its own back first)
        torch.cuda.set_stream(torch.cuda.default_stream(device))
    native = getattr(s, "_rccl_native", None)
    if native:
        s.hip_sync()
        native[0].lorads_rccl_comm_destroy(native[1])
        s._rccl_native = None
    s.close()
    if out is not None and world == 1 and out.get("phase1") and not os.environ.get("LORADS_BENCH_NO_PHASE1_RERUN"):
        # The phase 1 above is the first GPU work of this process: the run-time loads every kernel on its first launch and the
        # clocks come up from idle inside it (maxcut800: 33 ms for 127 inner iterations the first time, 8 ms every later time).
        # The same phase 1 once more, in a fresh context, now that neither is the case -- what an inner iteration costs.
        try:
            s2 = host.Session.open(path)
            s2.set_params(verbose=0, timesLogRank=tlr, phase1Tol=1e-2, reoptLevel=0)
            if workload == "matcomp50000" and os.environ.get("LORADS_BENCH_RANK_GROWTH") != "1":
                s2.set_params(dyrankLevel=0)
            s2.prepare(1, 0, separable=False)
            s2.attach_hip()
            s2.hip_sync()
            n0 = s2.hip_launch_count()
            t2 = time.perf_counter()
            s2.alm()
            s2.hip_sync()
            t2 = time.perf_counter() - t2
            r2 = s2.results()
            if r2["alm_inner"]:
                out["phase1"]["again_in_a_warm_process"] = {
                    "inner_iters": int(r2["alm_inner"]), "seconds": t2, "us_per_inner_iter": 1e6 * t2 / r2["alm_inner"],
                    "launches_per_inner_iter": (s2.hip_launch_count() - n0) / r2["alm_inner"]}
            s2.close()
        except Exception as e:  # noqa: BLE001
            out["phase1"]["again_in_a_warm_process"] = {"error": str(e)}
    return out


def spawn_ranks(a, argv):
    """`python bench.py --gpus N` without a launcher: this process -- which has made NO GPU call and has not even
    imported torch -- starts N children with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set (what torch.distributed.run
    would export), waits for them, forwards rank 0's JSON line and fails if any child fails.  Children are separate
    processes (subprocess, no exec from a process that touched the GPU)."""
    import socket
    import __graft_entry__
    __graft_entry__.build()   # once, before the ranks start (they only load the built libraries)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for rk in range(a.gpus):
        env = dict(os.environ, RANK=str(rk), LOCAL_RANK=str(rk), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LORADS_BENCH_CHILD="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if rk == 0 else subprocess.DEVNULL, text=True))
    out0, _ = procs[0].communicate()
    rcs = [procs[0].returncode]
    deadline = time.time() + 120
    for pr in procs[1:]:
        try:
            rcs.append(pr.wait(timeout=max(1.0, deadline - time.time())))
        except subprocess.TimeoutExpired:   # rank 0 is gone and this one is still in a collective: end exactly it
            pr.kill()
            rcs.append(pr.wait())
    line = [ln for ln in (out0 or "").splitlines() if ln.startswith("{")]
    if line:
        print(line[-1], flush=True)   # (also when a check failed: the line says which)
    if any(rcs) or not line:
        log("bench.py: ranks exited with codes %s%s" % (rcs, "" if line else "; no JSON line from rank 0"))
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default=None, help="rand20000 (headline, cfg3b; default) | maxcut20000 (cfg3a) | "
                    "matcomp50000 (cfg5) | blk16x4000 (cfg4; default of --scaling strong) | any NAMED instance")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: N copies of the block, one per GPU (value = N x iterations / s); strong: the cones of ONE "
                         "problem (blk16x4000: 16 cones, BASELINE cfg4) dealt over the N ranks (value = iterations / s)")
    ap.add_argument("--times-log-rank", type=float, default=None)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the Max-Cut n=20000 companion run")
    ap.add_argument("--cpu-budget", type=float, default=20.0)
    ap.add_argument("--sample-every", type=int, default=0, help="time every n-th operator application with HIP events INSIDE the "
                    "timed region (0 = none there: the roofline figures come from the untimed pass after it, and a timed "
                    "application always takes the operator's general form, which the headline's iteration 0 otherwise shortcuts)")
    ap.add_argument("--windows", type=int, default=5, help="after the timed region: this many further windows of --steps "
                    "steps (reported as ms_per_step_windows / _median; the headline value is the FIRST window)")
    ap.add_argument("--roofline-samples", type=int, default=200, help="untimed pass after the timed region: every operator "
                    "application timed with HIP events until this many samples exist")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what they computed in the last "
                    "step as DIR/<workload>_<name>.npy (float64, at most 64 MB in all; rank 0's cones): U<k>, V<k>, lambda and "
                    "scalars = [pObj, dObj, err1, CG iterations of the timed steps]")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    explicit_workload = a.workload is not None or a.scaling == "strong"
    if a.workload is None:
        a.workload = "blk16x4000" if a.scaling == "strong" else "rand20000"
    if a.times_log_rank is None:
        a.times_log_rank = {"matcomp50000": 5.5, "blk16x4000": 2.0}.get(a.workload, 4.0)

    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        return spawn_ranks(a, sys.argv[1:])

    import torch
    import __graft_entry__
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world and world > 1:
        log("warning: --gpus %d but WORLD_SIZE %d" % (a.gpus, world))
    dist = None
    # rehearsal knobs (1-GPU box): LORADS_DIST_BACKEND=gloo LORADS_FORCE_DEVICE=0 run N ranks on one card
    backend = os.environ.get("LORADS_DIST_BACKEND", "nccl")
    if "LORADS_FORCE_DEVICE" in os.environ and world > 1:   # several ranks on one card: their one-launch iterations take turns (persist.inc)
        os.environ.setdefault("LORADS_SHARED_GPU", "1")
    dev_index = int(os.environ.get("LORADS_FORCE_DEVICE", local_rank if world > 1 else 0))
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    npin = pin_to_gpu_numa(torch, dev_index)
    log("rank %d: cuda:%d, host thread pinned to %s" % (rank, dev_index, ("the GPU's %d local CPUs" % npin) if npin else "nothing (no NUMA information)"))
    if world > 1 or os.environ.get("LORADS_FORCE_DIST") == "1":  # (the knob measures the hook's own cost on one rank)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
    if rank == 0:
        __graft_entry__.build()
    if dist:
        dist.barrier()
    from lorads_amd import host

    workdir = tempfile.mkdtemp(prefix="lorads_bench_")
    atexit.register(shutil.rmtree, workdir, True)
    dump = {} if a.dump_outputs else None
    out = run_workload(a, a.workload, torch, dist, device, world, rank, host, not a.no_cpu, workdir, dump=dump)
    if world > 1 and not a.no_extra and not explicit_workload:
        # N > 1 as the driver calls it (no --workload / --scaling): the weak replica line above AND BASELINE config 4 -- the 16 cones of
        # ONE blk16x4000 problem dealt over the N ranks (strong scaling) -- as `extra`, each with ranks_seen, the exchange and a sharded
        # parity block
        import copy
        a2 = copy.copy(a)
        a2.scaling = "strong"
        ex = run_workload(a2, "blk16x4000", torch, dist, device, world, rank, host, False, workdir, tlr=2.0, dump=dump)
        if rank == 0:
            keys = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "ms_per_step_median", "scaling", "ranks_seen",
                    "scalar_exchange", "cg_iters_per_s", "cg_iters_per_admm_iter", "config", "roofline", "state", "parity_sharded",
                    "one_launch_iteration", "phase1", "launches_per_step")
            out["extra"] = [{k: ex[k] for k in keys if k in ex}]
    if rank == 0 and world == 1 and a.workload == "rand20000" and not a.no_extra:
        # the north-star target sentence is phrased on Max-Cut n = 20000, r = 40 (cfg3a): reported beside the headline
        keys = ("value", "unit", "ms_per_step", "ms_per_step_median", "cg_iters_per_s", "cg_iters_per_admm_iter", "config", "roofline",
                "cpu_baseline", "state", "parity_full_size", "speedup_vs_cpu_1core", "speedup_vs_cpu_1core_cg_normalised", "phase1",
                "one_launch_iteration", "launches_per_step")
        ex = run_workload(a, "maxcut20000", torch, dist, device, world, rank, host, not a.no_cpu, workdir, tlr=4.0, dump=dump)
        out["extra"] = [{k: ex[k] for k in keys if k in ex}]
    if dist:
        dist.barrier()
        dist.destroy_process_group()
    rc = 0
    if rank == 0:
        if dump is not None:
            write_outputs(a.dump_outputs, dump)
        print(json.dumps(out), flush=True)
        # a run that silently had fewer ranks than --gpus, or whose sharded iterations differ from the single-rank ones, must not pass
        for line in [out] + list(out.get("extra") or []):
            if world > 1 and line.get("ranks_seen") not in (None, world):
                log("bench.py: ranks_seen %s != %d" % (line.get("ranks_seen"), world))
                rc = 2
            if line.get("parity_sharded") is not None and not line["parity_sharded"].get("ok"):
                log("bench.py: sharded parity check failed: %s" % json.dumps(line["parity_sharded"]))
                rc = 2
    if rc:
        sys.exit(rc)


if __name__ == "__main__":
    main()
