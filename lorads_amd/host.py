"""ctypes mirror of the plain-C host (lorads_amd/csrc/host) and of its operator table.

The table `Backend` is field-for-field `lrd_backend` (csrc/host/lorads_host.h), which itself is
slot-for-slot the reference's `lorads_func` (src_semi/data/def_lorads_solver.h:109-127) plus the
non-table calls on the path.  Tests read like the reference's own call sites:

    be.init_constr(PAIR_RR); lag = be.alm_cal_grad(rho); be.lbfgs_direction(it); ...

The product attaches ONLY the HIP table (`Session.attach_hip`), which raises if the HIP library is
missing -- there is no CPU fallback here.
"""
import ctypes as C
import importlib
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
DEV_LIB = os.path.join(LIB_DIR, "liblorads_hip_dev.so")   # development build: the product library + lorads_hip_ubench (csrc/Makefile `dev`)

PAIR_RR, PAIR_UV = 0, 1
MAT_R, MAT_U, MAT_V, MAT_GRAD = 0, 1, 2, 3
VEC_LAMBDA, VEC_CONSTR_SUM, VEC_Q1, VEC_Q2 = 0, 1, 2, 3

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int)


class BackendStruct(C.Structure):
    _fields_ = [
        ("ctx", C.c_void_p),
        ("name", C.c_char_p),
        ("init_constr", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int)),
        ("alm_cal_grad", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, _dp)),
        ("lbfgs_direction", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int)),
        ("alm_q12p12", C.CFUNCTYPE(C.c_int, C.c_void_p, _dp)),
        ("alm_linesearch_coeffs", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, _dp)),
        ("set_y_as_neg_grad", C.CFUNCTYPE(C.c_int, C.c_void_p)),
        ("alm_update_var", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double)),
        ("set_lbfgs_his_two", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double)),
        ("update_dimacs", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _dp)),
        ("cal_obj", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _dp)),
        ("admm_update_var", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int, _ip)),
        ("update_dual_var", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double)),
        ("cal_dual_obj", C.CFUNCTYPE(C.c_int, C.c_void_p, _dp)),
        ("alm_to_admm", C.CFUNCTYPE(C.c_int, C.c_void_p)),
        ("average_uv_to_v", C.CFUNCTYPE(C.c_int, C.c_void_p)),
        ("scale_obj", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double)),
        ("resize_rank", C.CFUNCTYPE(C.c_int, C.c_void_p, _ip)),
        ("set_mat", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, _dp)),
        ("get_mat", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, _dp)),
        ("set_vec", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _dp)),
        ("get_vec", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _dp)),
        ("set_allreduce", C.CFUNCTYPE(C.c_int, C.c_void_p, ALLREDUCE_FN, C.c_void_p)),
        ("destroy", C.CFUNCTYPE(None, C.c_void_p)),
        ("admm_step", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int, _dp)),
        ("dual_infeasibility", C.CFUNCTYPE(C.c_int, C.c_void_p, _dp)),
        ("alm_front", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_int, _dp)),
        ("alm_step", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int, _dp)),
        ("certificate", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_double, _dp, _dp, _dp, _dp)),
        ("round_bisect", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int, _dp, _dp, _ip, _ip,
                                     C.POINTER(C.c_int8), _ip, _ip, _dp, _dp, _ip)),
        ("get_slack", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int64), _ip, _ip, _dp)),
        ("round_stable", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int, _dp, _dp, _ip, _ip,
                                     C.POINTER(C.c_uint8), _ip, _ip, _dp, _dp)),
        ("round_pm1", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int, _dp, _dp, _ip, _ip,
                                  C.POINTER(C.c_int8), _ip, _dp)),
        ("round_kcut", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, _dp, _dp, _ip, _ip,
                                   C.POINTER(C.c_uint8), _ip, _dp, _dp, _dp)),
        ("primal_entries", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, _ip, _ip, _dp, _dp, _dp)),
        ("primal_apply", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp)),
        ("primal_topk", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(C.c_int64), _ip, _ip, _dp, _ip)),
        ("triangle_cuts", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int64), _ip, _ip, _ip,
                                      C.POINTER(C.c_int8), _dp, _ip, _ip)),
        ("entry_bounds", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                     C.POINTER(C.c_int64), _ip, _ip, C.POINTER(C.c_int8), _dp, _ip, _ip)),
        ("spectrum", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _dp, _dp, _ip)),
        ("compress_rank", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _ip, _dp)),
    ]


class SpectralConeStruct(C.Structure):
    """lrd_spectral_cone (csrc/host/lorads_host.h)"""
    _fields_ = [("n", C.c_int), ("is_lp", C.c_int), ("rank_before", C.c_int), ("rank_after", C.c_int), ("sweeps", C.c_int),
                ("eig", _dp), ("trace_lost", C.c_double), ("frob_lost", C.c_double)]


class SpectralReportStruct(C.Structure):
    """lrd_spectral_report (csrc/host/lorads_host.h)"""
    _fields_ = [("nblk", C.c_int), ("src", C.c_int), ("tol", C.c_double), ("cap", C.c_int),
                ("pobj_before", C.c_double), ("pobj_after", C.c_double), ("err1_before", C.c_double), ("err1_after", C.c_double),
                ("cone", C.POINTER(SpectralConeStruct))]


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (what, rc))


class Backend:
    """Pythonic view of one operator table (the one a Session owns after attach)."""

    def __init__(self, struct_ptr, session):
        self._s = struct_ptr.contents
        self._session = session

    @property
    def name(self):
        return self._s.name.decode()

    def init_constr(self, pair):
        _check(self._s.init_constr(self._s.ctx, pair), "init_constr")

    def alm_cal_grad(self, rho):
        v = C.c_double()
        _check(self._s.alm_cal_grad(self._s.ctx, rho, C.byref(v)), "alm_cal_grad")
        return v.value

    def lbfgs_direction(self, inner_iter):
        _check(self._s.lbfgs_direction(self._s.ctx, inner_iter), "lbfgs_direction")

    def alm_q12p12(self):
        p = (C.c_double * 2)()
        _check(self._s.alm_q12p12(self._s.ctx, p), "alm_q12p12")
        return p[0], p[1]

    def alm_linesearch_coeffs(self, rho, p1, p2):
        k = (C.c_double * 4)()
        _check(self._s.alm_linesearch_coeffs(self._s.ctx, rho, p1, p2, k), "alm_linesearch_coeffs")
        return [k[i] for i in range(4)]

    def set_y_as_neg_grad(self):
        _check(self._s.set_y_as_neg_grad(self._s.ctx), "set_y_as_neg_grad")

    def alm_update_var(self, tau):
        _check(self._s.alm_update_var(self._s.ctx, tau), "alm_update_var")

    def set_lbfgs_his_two(self, tau):
        _check(self._s.set_lbfgs_his_two(self._s.ctx, tau), "set_lbfgs_his_two")

    def update_dimacs(self, pair):
        v = C.c_double()
        _check(self._s.update_dimacs(self._s.ctx, pair, C.byref(v)), "update_dimacs")
        return v.value

    def cal_obj(self, pair):
        v = C.c_double()
        _check(self._s.cal_obj(self._s.ctx, pair, C.byref(v)), "cal_obj")
        return v.value

    def admm_update_var(self, rho, cg_tol, cg_max_iter=800):
        it = C.c_int()
        _check(self._s.admm_update_var(self._s.ctx, rho, cg_tol, cg_max_iter, C.byref(it)), "admm_update_var")
        return it.value

    @property
    def has_admm_step(self):
        return bool(self._s.admm_step)

    def admm_step(self, rho, cg_tol, cg_max_iter=800):
        """fused ADMM iteration (optional slot): returns (cg_iters, pobj, dobj, err1)"""
        o = (C.c_double * 4)()
        _check(self._s.admm_step(self._s.ctx, rho, cg_tol, cg_max_iter, o), "admm_step")
        return int(o[0]), o[1], o[2], o[3]

    def update_dual_var(self, rho):
        _check(self._s.update_dual_var(self._s.ctx, rho), "update_dual_var")

    def cal_dual_obj(self):
        v = C.c_double()
        _check(self._s.cal_dual_obj(self._s.ctx, C.byref(v)), "cal_dual_obj")
        return v.value

    @property
    def has_alm_step(self):
        return bool(self._s.alm_step) and bool(self._s.alm_front)

    def alm_front(self, rho, inner):
        """(p1, p2, [a, b, c, d]) of the direction for inner-iteration counter `inner` (optional slot)"""
        o = (C.c_double * 6)()
        _check(self._s.alm_front(self._s.ctx, rho, inner, o), "alm_front")
        return o[0], o[1], [o[2], o[3], o[4], o[5]]

    def alm_step(self, rho, tau, next_inner):
        """finish the inner iteration with step tau and pre-compute the next direction (optional slot):
        (lagNormSq, err1, p1, p2, [a, b, c, d])"""
        o = (C.c_double * 8)()
        _check(self._s.alm_step(self._s.ctx, rho, tau, next_inner, o), "alm_step")
        return o[0], o[1], o[2], o[3], [o[4], o[5], o[6], o[7]]

    @property
    def has_dual_infeasibility(self):
        return bool(self._s.dual_infeasibility)

    def dual_infeasibility(self):
        """sum over the table's cones of |min(lambda_min(C_k - A_k^*(lambda)), 0)| (optional slot)"""
        v = C.c_double()
        _check(self._s.dual_infeasibility(self._s.ctx, C.byref(v)), "dual_infeasibility")
        return v.value

    def alm_to_admm(self):
        _check(self._s.alm_to_admm(self._s.ctx), "alm_to_admm")

    def average_uv_to_v(self):
        _check(self._s.average_uv_to_v(self._s.ctx), "average_uv_to_v")

    def scale_obj(self, s):
        _check(self._s.scale_obj(self._s.ctx, s), "scale_obj")

    def resize_rank(self, new_rank):
        arr = (C.c_int * len(new_rank))(*[int(x) for x in new_rank])
        _check(self._s.resize_rank(self._s.ctx, arr), "resize_rank")
        self._session._rank_override = [int(x) for x in new_rank]

    def has_spectrum(self):
        return bool(self._s.spectrum) and bool(self._s.compress_rank)

    def _sdp_ranks(self):
        lp = self._session._lp_blocks()
        return [0 if lp[k] else self._session.block_shape(k)[1] for k in range(self._session.nblk)]

    def spectrum(self, src, vectors=False):
        """the table's slot as it is: per block the eigenvalues (descending) of F^T F, the Jacobi sweep counts and, with
        vectors=True, the eigenvectors (columns); an empty array for the LP block.  Returns (code, eigenvalues, sweeps, eigenvectors):
        code != 0 is the slot's refusal and the rest is None; eigenvectors is None without vectors=True."""
        ranks = self._sdp_ranks()
        eig = np.zeros(max(sum(ranks), 1))
        q = np.zeros(max(sum(r * r for r in ranks), 1)) if vectors else None
        sw = np.zeros(max(len(ranks), 1), dtype=np.int32)
        rc = self._s.spectrum(self._s.ctx, src, eig.ctypes.data_as(_dp), q.ctypes.data_as(_dp) if vectors else None, sw.ctypes.data_as(_ip))
        if rc:
            return rc, None, None, None
        lam, Q, at, qat = [], [], 0, 0
        for r in ranks:
            lam.append(eig[at:at + r].copy())
            if vectors:
                Q.append(q[qat:qat + r * r].reshape(r, r).T.copy())  # (column-major on the wire)
            at += r
            qat += r * r
        return 0, lam, [int(x) for x in sw[:len(ranks)]], (Q if vectors else None)

    def compress_rank(self, src, new_rank):
        """the table's slot as it is (constraint values are the caller's to refresh): returns (code, eigenvalues per block)"""
        ranks = self._sdp_ranks()
        eig = np.zeros(max(sum(ranks), 1))
        arr = (C.c_int * len(new_rank))(*[int(x) for x in new_rank])
        rc = self._s.compress_rank(self._s.ctx, src, arr, eig.ctypes.data_as(_dp))
        if rc:
            return rc, None
        self._session._rank_override = [int(x) for x in new_rank]
        lam, at = [], 0
        for r in ranks:
            lam.append(eig[at:at + r].copy())
            at += r
        return 0, lam

    def has_primal(self):
        return bool(self._s.primal_entries) and bool(self._s.primal_apply)

    def primal_entries(self, src, blk, rows, cols, ref=None, want_val=True, count=None):
        """the table's slot as it is: val[e] = F_rows[e] . F_cols[e] of block blk's X = F F^T (0-based positions) and, with ref, the
        statistics {sum (val - ref)^2, sum |val - ref|, max |val - ref|, sum ref^2} formed on the device.  Returns (code, val, stats);
        code != 0 is the slot's refusal.  rows / cols None, want_val=False and count pass a NULL / another count down as they are."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        c = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
        n = int(count) if count is not None else (0 if r is None else len(r))
        f = None if ref is None else np.ascontiguousarray(ref, dtype=np.float64)
        val = np.zeros(max(n, 1)) if want_val else None
        st = np.zeros(4) if f is not None else None
        ptr = lambda a, t: a.ctypes.data_as(t) if a is not None else None  # noqa: E731
        rc = self._s.primal_entries(self._s.ctx, src, blk, n, ptr(r, _ip), ptr(c, _ip), ptr(val, _dp), ptr(f, _dp), ptr(st, _dp))
        if rc:
            return rc, None, None
        return 0, (val[:max(n, 0)] if want_val else None), st

    def primal_apply(self, src, blk, B, want_t=False, ncols=None):
        """the table's slot as it is: Y = X_blk B and, with want_t, T = F^T B for B (n, ncols) or (n,).  Returns (code, Y, T)."""
        if 0 <= int(blk) < self._session.nblk:
            n, rank = self._session.block_shape(blk)
        else:   # (a block the session does not know: the slot's to refuse)
            n, rank = (len(B) if B is not None else 1), 1
        if B is None:
            Bf, nc = None, int(ncols or 1)
        else:
            Bf = np.asfortranarray(np.asarray(B, dtype=np.float64).reshape(n, -1))
            nc = int(ncols) if ncols is not None else Bf.shape[1]
        Y = np.zeros((n, max(nc, 1)), order="F")
        T = np.zeros((rank, max(nc, 1)), order="F") if want_t else None
        rc = self._s.primal_apply(self._s.ctx, src, blk, nc, Bf.ctypes.data_as(_dp) if Bf is not None else None, Y.ctypes.data_as(_dp),
                                  T.ctypes.data_as(_dp) if want_t else None)
        if rc:
            return rc, None, None
        return 0, Y[:, :nc], (T[:, :nc] if want_t else None)

    def has_primal_topk(self):
        return bool(self._s.primal_topk)

    def primal_topk(self, src, blk, rows, col_lo, col_hi, k, smallest=0, include_diag=0, skip_ptr=None, skip_col=None, nq=None,
                    want_arrays=True):
        """the table's slot as it is: per query row the k best columns of the window [col_lo, col_hi) of block blk's X = F F^T.
        Returns (code, idx [nq, k], val [nq, k], found [nq]); code != 0 is the slot's refusal.  rows / skip_ptr / skip_col None, nq
        and want_arrays=False pass a NULL / another count down as they are."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        n = int(nq) if nq is not None else (0 if r is None else len(r))
        sp = None if skip_ptr is None else np.ascontiguousarray(skip_ptr, dtype=np.int64)
        sc = None if skip_col is None else np.ascontiguousarray(skip_col, dtype=np.int32)
        if sc is not None and len(sc) == 0:
            sc = np.zeros(1, dtype=np.int32)   # (an empty list is still a list: not NULL)
        kk = int(k) if 1 <= int(k) <= 128 else 1
        idx = np.full((max(n, 1), kk), -2, dtype=np.int32)
        val = np.full((max(n, 1), kk), np.nan)
        found = np.full(max(n, 1), -2, dtype=np.int32)
        ptr = lambda a, t: a.ctypes.data_as(t) if a is not None else None  # noqa: E731
        out = (ptr(idx, _ip), ptr(val, _dp), ptr(found, _ip)) if want_arrays else (None, None, None)
        rc = self._s.primal_topk(self._s.ctx, int(src), int(blk), n, ptr(r, _ip), int(col_lo), int(col_hi), int(k), int(smallest),
                                 int(include_diag), ptr(sp, C.POINTER(C.c_int64)), ptr(sc, _ip), *out)
        if rc:
            return rc, None, None, None
        return 0, idx[:max(n, 0)], val[:max(n, 0)], found[:max(n, 0)]

    def has_triangle_cuts(self):
        return bool(self._s.triangle_cuts)

    def triangle_cuts(self, src, blk, min_violation, max_cuts, want_arrays=True):
        """the table's slot as it is: the (triple, class) pairs of cone blk whose triangle inequality is violated by more than
        min_violation.  Returns (code, count, p, q, s, cls, violation, passes) with the min(count, max_cuts) largest pairs in the
        order (violation descending, p, q, s, cls ascending); code != 0 is the slot's refusal.  want_arrays=False passes NULL
        arrays down."""
        cap = max(int(max_cuts), 1) if -1 < max_cuts <= (1 << 20) else 1
        cnt, kept, passes = C.c_int64(0), C.c_int(0), C.c_int(0)
        p, q, s = (np.zeros(cap, dtype=np.int32) for _ in range(3))
        cls, v = np.zeros(cap, dtype=np.int8), np.zeros(cap)
        i8 = C.POINTER(C.c_int8)
        if want_arrays:
            rc = self._s.triangle_cuts(self._s.ctx, src, blk, float(min_violation), int(max_cuts), C.byref(cnt), p.ctypes.data_as(_ip),
                                       q.ctypes.data_as(_ip), s.ctypes.data_as(_ip), cls.ctypes.data_as(i8), v.ctypes.data_as(_dp),
                                       C.byref(kept), C.byref(passes))
        else:
            rc = self._s.triangle_cuts(self._s.ctx, src, blk, float(min_violation), int(max_cuts), C.byref(cnt), None, None, None, None,
                                       None, None, C.byref(passes))
        if rc:
            return (rc,) + (None,) * 7
        k = kept.value
        return 0, cnt.value, p[:k], q[:k], s[:k], cls[:k], v[:k], passes.value

    def has_entry_bounds(self):
        return bool(self._s.entry_bounds)

    def entry_bounds(self, src, blk, lower, upper, min_violation, max_cuts, want_arrays=True):
        """the table's slot as it is: the (pair, class) of cone blk whose bound lower <= X_pq <= upper is violated by more than
        min_violation.  Returns (code, count, p, q, cls, violation, passes) with the min(count, max_cuts) largest in the order
        (violation descending, p, q, cls ascending); code != 0 is the slot's refusal.  want_arrays=False passes NULL arrays down."""
        cap = max(int(max_cuts), 1) if -1 < max_cuts <= (1 << 20) else 1
        cnt, kept, passes = C.c_int64(0), C.c_int(0), C.c_int(0)
        p, q = (np.zeros(cap, dtype=np.int32) for _ in range(2))
        cls, v = np.zeros(cap, dtype=np.int8), np.zeros(cap)
        i8 = C.POINTER(C.c_int8)
        args = (self._s.ctx, src, blk, float(lower), float(upper), float(min_violation), int(max_cuts), C.byref(cnt))
        if want_arrays:
            rc = self._s.entry_bounds(*args, p.ctypes.data_as(_ip), q.ctypes.data_as(_ip), cls.ctypes.data_as(i8), v.ctypes.data_as(_dp),
                                      C.byref(kept), C.byref(passes))
        else:
            rc = self._s.entry_bounds(*args, None, None, None, None, None, C.byref(passes))
        if rc:
            return (rc,) + (None,) * 6
        k = kept.value
        return 0, cnt.value, p[:k], q[:k], cls[:k], v[:k], passes.value

    def _round_slot(self, fn, src, lead, trials, seed, max_rounds, outs, rest):
        """a round_* slot of the table as it is: fn(ctx, src, *lead, trials, seed, max_rounds, obj, obj0, &best, &best0, *outs, &rounds,
        *rest).  Returns (code, what every rounding returns: obj, obj0, best, best0, rounds)."""
        K = max(int(trials), 0)
        obj, obj0 = np.zeros(max(K, 1)), np.zeros(max(K, 1))
        best, best0, rounds = C.c_int(0), C.c_int(0), C.c_int(0)
        rc = fn(self._s.ctx, int(src), *lead, int(trials), int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_rounds), obj.ctypes.data_as(_dp),
                obj0.ctypes.data_as(_dp), C.byref(best), C.byref(best0), *outs, C.byref(rounds), *rest)
        return rc, dict(obj=obj[:K], obj0=obj0[:K], best=best.value, best0=best0.value, rounds=rounds.value)

    def _stored_trial(self, name, trial, ntot, dtype):
        """one trial of the last round_stable / round_bisect call on this table's HIP context: lorads_hip_<name>, one byte per vertex"""
        lib, ctx = self._session._hip()
        out = np.zeros(max(ntot, 1), dtype=dtype)
        ptr = C.POINTER(np.ctypeslib.as_ctypes_type(dtype))
        fn = getattr(lib, "lorads_hip_" + name)
        fn.argtypes = [C.c_void_p, C.c_int, ptr]
        _check(fn(ctx, int(trial), out.ctypes.data_as(ptr)), name)
        return out[:ntot]

    def has_round_kcut(self):
        return bool(self._s.round_kcut)

    def round_kcut(self, src, parts, trials, seed=0, max_rounds=0, want_vectors=False):
        """the table's slot as it is (values in the backend's terms): returns (code, dict) with obj, obj0, best, best0, label, rounds,
        t, lp_upper and -- want_vectors -- vectors (flat: per SDP cone parts x rank x trials); code != 0 is the slot's refusal (the
        dict is then None).  trials = 0 checks applicability and still gives t and lp_upper."""
        ses = self._session
        lp = ses._lp_blocks()
        sdp = [k for k in range(ses.nblk) if not lp[k]]
        ntot = sum(ses.block_shape(k)[0] for k in sdp)
        nlp = sum(ses.block_shape(k)[0] for k in range(ses.nblk) if lp[k])
        K = max(int(trials), 0)
        ok = 2 <= parts <= 64 and K * parts <= (1 << 20)
        label, t, lpu = np.zeros(max(ntot, 1), dtype=np.uint8), np.zeros(max(ntot, 1)), np.zeros(max(nlp, 1))
        glen = sum(ses.block_shape(k)[1] for k in sdp) * K * parts if want_vectors and ok else 0
        vec = np.zeros(max(glen, 1))
        rc, d = self._round_slot(self._s.round_kcut, src, [int(parts)], trials, seed, max_rounds, [label.ctypes.data_as(C.POINTER(C.c_uint8))],
                                 [vec.ctypes.data_as(_dp) if glen else None, t.ctypes.data_as(_dp), lpu.ctypes.data_as(_dp)])
        if rc:
            return rc, None
        return 0, dict(d, label=label[:ntot], t=t[:ntot], lp_upper=lpu[:nlp], vectors=vec[:glen] if glen else None)

    def has_round_stable(self):
        return bool(self._s.round_stable)

    def round_stable(self, src, trials, seed=0, max_rounds=0, want_scores=False):
        """the table's slot as it is (values in the backend's terms): returns (code, dict) with obj, obj0, best, best0, member (0/1
        per vertex, SDP cone after SDP cone), sizes (cones x trials), rounds, T (per SDP cone), lp_upper and -- want_scores -- scores
        (per SDP cone an n x trials array); code != 0 is the slot's refusal (the dict is then None).  trials = 0 checks
        applicability and still gives T and lp_upper."""
        ses = self._session
        lp = ses._lp_blocks()
        ns = [ses.block_shape(k)[0] for k in range(ses.nblk) if not lp[k]]
        ntot, ncone = sum(ns), len(ns)
        nlp = sum(ses.block_shape(k)[0] for k in range(ses.nblk) if lp[k])
        K = max(int(trials), 0)
        ok = K <= 65536
        member, Tu = np.zeros(max(ntot, 1), dtype=np.uint8), np.zeros(max(ncone + nlp, 1))
        sizes = np.zeros(max(ncone * K, 1) if ok else 1, dtype=np.int32)
        slen = ntot * K if want_scores and ok else 0
        sc = np.zeros(max(slen, 1))
        rc, d = self._round_slot(self._s.round_stable, src, [], trials, seed, max_rounds,
                                 [member.ctypes.data_as(C.POINTER(C.c_uint8)), sizes.ctypes.data_as(_ip)],
                                 [sc.ctypes.data_as(_dp) if slen else None, Tu.ctypes.data_as(_dp)])
        if rc:
            return rc, None
        scores, at = None, 0
        if slen:
            scores = []
            for n in ns:
                scores.append(sc[at * K:(at + n) * K].reshape(K, n).T.copy())
                at += n
        return 0, dict(d, member=member[:ntot], sizes=sizes[:ncone * K].reshape(ncone, K), T=Tu[:ncone], lp_upper=Tu[ncone:ncone + nlp],
                       scores=scores)

    def stable_trial(self, trial):
        """the sets of one trial of the last round_stable call on this table's HIP context (0/1 per vertex, SDP cone after SDP cone)"""
        ses = self._session
        lp = ses._lp_blocks()
        return self._stored_trial("stable_trial", trial, sum(ses.block_shape(k)[0] for k in range(ses.nblk) if not lp[k]), np.uint8)

    def has_round_bisect(self):
        return bool(self._s.round_bisect)

    def round_bisect(self, src, trials, seed=0, max_rounds=0, want_hyperplanes=False):
        """the table's slot as it is (values in the backend's terms): returns (code, dict) with obj, obj0, best, best0, sign (cone
        after cone), imbalance (cones x trials), rounds, t and diff (per cone) and -- want_hyperplanes -- hyperplanes (per cone a
        rank x trials array); code != 0 is the slot's refusal (the dict is then None).  trials = 0 checks applicability and still
        gives t and diff."""
        ses = self._session
        ns = [ses.block_shape(k)[0] for k in range(ses.nblk)]
        rk = [ses.block_shape(k)[1] for k in range(ses.nblk)]
        ntot, ncone = sum(ns), len(ns)
        K = max(int(trials), 0)
        ok = K <= 65536
        sign, t, diff = np.zeros(max(ntot, 1), dtype=np.int8), np.zeros(max(ncone, 1)), np.zeros(max(ncone, 1), dtype=np.int32)
        imb = np.zeros(max(ncone * K, 1) if ok else 1, dtype=np.int32)
        glen = sum(rk) * K if want_hyperplanes and ok else 0
        g = np.zeros(max(glen, 1))
        rc, d = self._round_slot(self._s.round_bisect, src, [], trials, seed, max_rounds,
                                 [sign.ctypes.data_as(C.POINTER(C.c_int8)), imb.ctypes.data_as(_ip)],
                                 [g.ctypes.data_as(_dp) if glen else None, t.ctypes.data_as(_dp), diff.ctypes.data_as(_ip)])
        if rc:
            return rc, None
        planes, at = None, 0
        if glen:
            planes = []
            for r in rk:
                planes.append(g[at:at + r * K].reshape(r, K).copy())
                at += r * K
        return 0, dict(d, sign=sign[:ntot], imbalance=imb[:ncone * K].reshape(ncone, K), t=t[:ncone], diff=diff[:ncone], hyperplanes=planes)

    def bisect_trial(self, trial):
        """the signs of one trial of the last round_bisect call on this table's HIP context (cone after cone)"""
        ses = self._session
        return self._stored_trial("bisect_trial", trial, sum(ses.block_shape(k)[0] for k in range(ses.nblk)), np.int8)

    def set_mat(self, which, blk, a):
        """a: (n, r) array, any layout; sent column-major like the reference's matElem."""
        a = np.asfortranarray(a, dtype=np.float64)
        _check(self._s.set_mat(self._s.ctx, which, blk, a.ctypes.data_as(_dp)), "set_mat")

    def get_mat(self, which, blk):
        n, r = self._session.block_shape(blk)
        out = np.empty((n, r), dtype=np.float64, order="F")
        _check(self._s.get_mat(self._s.ctx, which, blk, out.ctypes.data_as(_dp)), "get_mat")
        return out

    def set_vec(self, which, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        _check(self._s.set_vec(self._s.ctx, which, v.ctypes.data_as(_dp)), "set_vec")

    def get_vec(self, which):
        out = np.empty(self._session.m, dtype=np.float64)
        _check(self._s.get_vec(self._s.ctx, which, out.ctypes.data_as(_dp)), "get_vec")
        return out


def _bind(lib):
    lib.lrd_session_open.restype = C.c_void_p
    lib.lrd_session_open.argtypes = [C.c_char_p]
    lib.lrd_session_from_triplets.restype = C.c_void_p
    lib.lrd_session_from_triplets.argtypes = [C.c_int, _dp, C.c_int, _ip, C.c_int64, _ip, _ip, _ip, _ip, _dp]
    lib.lrd_session_set_param.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    lib.lrd_session_prepare.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.lrd_session_problem.restype = C.c_void_p
    lib.lrd_session_problem.argtypes = [C.c_void_p]
    lib.lrd_session_backend.restype = C.POINTER(BackendStruct)
    lib.lrd_session_backend.argtypes = [C.c_void_p]
    lib.lrd_session_attach.argtypes = [C.c_void_p, C.POINTER(BackendStruct)]
    lib.lrd_session_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p]
    lib.lrd_session_solve.argtypes = [C.c_void_p]
    lib.lrd_session_alm.argtypes = [C.c_void_p]
    lib.lrd_session_alm_to_admm.argtypes = [C.c_void_p]
    lib.lrd_session_alm_to_admm.restype = None
    lib.lrd_session_admm.argtypes = [C.c_void_p, C.c_int]
    lib.lrd_session_results.argtypes = [C.c_void_p, _dp]
    lib.lrd_session_results2.argtypes = [C.c_void_p, _dp]
    lib.lrd_session_dual_infeasibility.argtypes = [C.c_void_p, _dp]
    lib.lrd_session_block_info.argtypes = [C.c_void_p, C.c_int] + [_ip] * 8
    lib.lrd_session_dims.argtypes = [C.c_void_p, _ip, _ip, _ip]
    lib.lrd_session_start.restype = _dp
    lib.lrd_session_start.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.lrd_session_current_rank.argtypes = [C.c_void_p, C.c_int]
    lib.lrd_session_primal_entries.argtypes = [C.c_void_p, C.c_int, C.c_int64, _ip, _ip, _dp, _dp, _dp]
    lib.lrd_session_primal_apply.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]
    lib.lrd_session_close.argtypes = [C.c_void_p]
    lib.lrd_session_close.restype = None
    lib.lrd_session_params_ptr = None
    return lib


_host_lib = None


def host_lib():
    """liblorads_host.so: the product's plain-C host, built by __graft_entry__.build()."""
    global _host_lib
    if _host_lib is None:
        path = os.path.join(LIB_DIR, "liblorads_host.so")
        if not os.path.exists(path):
            raise RuntimeError("%s is missing: run `python __graft_entry__.py` (build()) first" % path)
        _host_lib = _bind(C.CDLL(path, mode=C.RTLD_GLOBAL))
        _host_lib.lrd_hip_backend_create.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(BackendStruct)]
    return _host_lib


RESULT_KEYS = ["pObj", "dObj", "constrVio1", "pdGap", "alm_outer", "alm_inner", "alm_rho", "admm_iter", "cg_iter",
               "admm_rho", "t_alm", "t_admm", "status", "admm_iters_first", "cg_iters_first", "constrVioInf"]


# The four roundings of a Session (Session._rounded): the module of the result, its ctypes struct and result class, the host library's
# driver, free and writer, the name in ValueError and backend-error texts, whether the arguments are range-checked here, and what a
# refusal (code 2) says before " or the <name> backend cannot round".
_ROUNDINGS = {
    "pm1": dict(module="rounding", struct="RoundingStruct", result="Rounding", run="lrd_session_round_ex", free="lrd_rounding_free",
                write="lrd_rounding_write", name="round", checked=False,
                refusal="the problem cannot be rounded: it is not +-1-structured (no LP block; every constraint "
                        "a_i X[p,p] = b_i with b_i / a_i > 0, one per diagonal)"),
    "kcut": dict(module="kcut", struct="KCutStruct", result="KCut", run="lrd_session_kcut", free="lrd_kcut_free", write="lrd_kcut_write",
                 name="round_kcut", checked=True,
                 refusal="the problem cannot be rounded into parts: it is not k-cut-structured (every diagonal fixed by one "
                         "constraint a_i X[p,p] = b_i with b_i / a_i > 0; LP columns only in bound rows 2 a X[p,q] + c x_j = b)"),
    "stable": dict(module="stable", struct="StableStruct", result="StableSet", run="lrd_session_round_stable", free="lrd_stable_free",
                   write="lrd_stable_write", name="round_stable", checked=True,
                   refusal="no stable set can be read off the solution: the problem is not theta-structured (per cone one trace row "
                           "a tr(X) = b with a, b > 0, every other constraint an edge row X[p,q] = 0; LP columns only in bound rows "
                           "2 a X[p,q] + c x_j = b)"),
    "bisection": dict(module="bisection", struct="BisectionStruct", result="Bisection", run="lrd_session_round_bisect",
                      free="lrd_bisection_free", write="lrd_bisection_write", name="round_bisection", checked=True,
                      refusal="no balanced partition can be read off the solution: the problem is not bisection-structured (no LP block; "
                              "per cone one constraint a X[p,p] = b on every diagonal with one value of b / a > 0, and one sum row "
                              "a <11^T, X> = b with b / (a t^2) = d^2, d = n (mod 2))"),
}


class Session:
    """One problem + parameter block + start point (+ solver once a table is attached)."""

    def __init__(self, lib, handle):
        if not handle:
            raise RuntimeError("could not open the problem")
        self.lib = lib
        self.h = C.c_void_p(handle)
        self.be = None
        self._rank_override = None
        self._keep = []

    @classmethod
    def open(cls, fname, lib=None):
        lib = lib or host_lib()
        return cls(lib, lib.lrd_session_open(os.fsencode(fname)))

    @classmethod
    def from_triplets(cls, m, b, dims, mat, blk, row, col, val, lib=None):
        lib = lib or host_lib()
        b = np.ascontiguousarray(b, dtype=np.float64)
        dims = np.ascontiguousarray(dims, dtype=np.int32)
        arrs = [np.ascontiguousarray(x, dtype=np.int32) for x in (mat, blk, row, col)]
        val = np.ascontiguousarray(val, dtype=np.float64)
        h = lib.lrd_session_from_triplets(int(m), b.ctypes.data_as(_dp), len(dims), dims.ctypes.data_as(_ip),
                                          len(val), *[a.ctypes.data_as(_ip) for a in arrs], val.ctypes.data_as(_dp))
        return cls(lib, h)

    def set_params(self, **kw):
        for k, v in kw.items():
            if isinstance(v, (bool, np.bool_)) or (isinstance(v, (int, np.integer)) and not isinstance(v, bool)):
                txt = str(int(v))
            elif isinstance(v, (float, np.floating)):
                txt = repr(float(v))  # repr(np.float64(x)) is not a number literal
            else:
                txt = str(v)
            if self.lib.lrd_session_set_param(self.h, k.encode(), txt.encode()):
                raise KeyError("unknown parameter %s" % k)

    def prepare(self, world=1, rank=0, separable=False):
        """separable=True (HIP backend only): when no constraint touches cones of two ranks, this process keeps the sub-problem
        over its own constraints (m, b, row indices local) and the library shares only scalars with the other ranks
        (lorads_hip_set_separable); self.separable tells whether the deal was, self.constraint_map[i] = index of local
        constraint i in the file, self.m_global = constraints of the file."""
        self.lib.lrd_session_prepare_sharded.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        _check(self.lib.lrd_session_prepare_sharded(self.h, world, rank, int(bool(separable))), "prepare")
        m, nb, nbg = C.c_int(), C.c_int(), C.c_int()
        self.lib.lrd_session_dims(self.h, C.byref(m), C.byref(nb), C.byref(nbg))
        self.m, self.nblk, self.nblk_global = m.value, nb.value, nbg.value
        mg = C.c_int()
        cmap = np.zeros(max(self.m, 1), dtype=np.int32)
        self.lib.lrd_session_separable.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self.separable = bool(self.lib.lrd_session_separable(self.h, C.byref(mg), cmap.ctypes.data_as(C.POINTER(C.c_int))))
        self.m_global = mg.value
        self.constraint_map = cmap[:self.m] if self.separable else np.arange(self.m, dtype=np.int32)

    def block_info(self, k):
        v = [C.c_int() for _ in range(8)]
        _check(self.lib.lrd_session_block_info(self.h, k, *[C.byref(x) for x in v]), "block_info")
        keys = ["n", "rank", "nrow", "na", "nc", "np", "dense_mode", "cone_sparse"]
        d = dict(zip(keys, [x.value for x in v]))
        if self._rank_override is not None:
            d["rank"] = self._rank_override[k]
        elif self.be is not None:
            d["rank"] = self.lib.lrd_session_current_rank(self.h, k)
        return d

    def block_shape(self, k):
        d = self.block_info(k)
        return d["n"], d["rank"]

    def start_point(self, which, k):
        d = self.block_info(k)
        p = self.lib.lrd_session_start(self.h, which, k)
        return np.ctypeslib.as_array(p, shape=(d["rank"], d["n"])).T.copy()

    def problem_ptr(self):
        return self.lib.lrd_session_problem(self.h)

    def attach(self, struct):
        _check(self.lib.lrd_session_attach(self.h, C.byref(struct)), "attach")
        self.be = Backend(self.lib.lrd_session_backend(self.h), self)
        return self.be

    def attach_hip(self, lbfgs_len=2, libpath=None):
        """Wire the operator table to the HIP C-ABI library (include/lorads_hip.h).  Raises when the
        library or a GPU is missing: the product has no other backend."""
        st = BackendStruct()
        path = libpath or os.path.join(LIB_DIR, "liblorads_hip.so")
        self._hip_path = path
        rc = self.lib.lrd_hip_backend_create(self.problem_ptr(), lbfgs_len, os.fsencode(path), C.byref(st))
        if rc != 0:
            raise RuntimeError("HIP backend unavailable (code %d): %s -- the product has no CPU fallback" % (rc, path))
        return self.attach(st)

    # ---- measurement hooks of the HIP library (bench.py)
    def _hip(self):
        if getattr(self, "_hiplib", None) is None:
            lib = C.CDLL(getattr(self, "_hip_path", None) or os.path.join(LIB_DIR, "liblorads_hip.so"))
            lib.lorads_hip_profile.argtypes = [C.c_void_p, C.c_int, C.c_int]
            lib.lorads_hip_profile_read.argtypes = [C.c_void_p, _dp]
            lib.lorads_hip_algorithmic_bytes.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
            lib.lorads_hip_sync.argtypes = [C.c_void_p]
            lib.lorads_hip_operator_kind.argtypes = [C.c_void_p, C.c_int, _ip]
            lib.lorads_hip_stream.restype = C.c_void_p
            lib.lorads_hip_stream.argtypes = [C.c_void_p]
            lib.lorads_hip_set_allreduce_stream_ordered.argtypes = [C.c_void_p, C.c_int]
            self.lib.lrd_hip_backend_raw_ctx.restype = C.c_void_p
            self.lib.lrd_hip_backend_raw_ctx.argtypes = [C.POINTER(BackendStruct)]
            self._hiplib = lib
            self._hipctx = C.c_void_p(self.lib.lrd_hip_backend_raw_ctx(self.lib.lrd_session_backend(self.h)))
        return self._hiplib, self._hipctx

    def hip_profile(self, enable, sample_every=8):
        lib, ctx = self._hip()
        _check(lib.lorads_hip_profile(ctx, int(enable), int(sample_every)), "profile")

    def hip_profile_target(self, target):
        """0: time CG operator applications (default), 1: time solve fronts"""
        lib, ctx = self._hip()
        lib.lorads_hip_profile_target.argtypes = [C.c_void_p, C.c_int]
        _check(lib.lorads_hip_profile_target(ctx, int(target)), "profile_target")

    def hip_profile_read(self):
        lib, ctx = self._hip()
        out = (C.c_double * 8)()
        _check(lib.lorads_hip_profile_read(ctx, out), "profile_read")
        keys = ["matvec_launches", "speculation_misses", "cg_iters", "cg_solves", "sampled", "sampled_ms", "spmm_sampled",
                "spmm_sampled_ms"]
        return dict(zip(keys, [out[i] for i in range(8)]))

    def hip_profile_samples(self, cap=4096):
        """milliseconds of every operator application timed since hip_profile(1, ...) (drains the event pool)"""
        lib, ctx = self._hip()
        lib.lorads_hip_profile_samples.argtypes = [C.c_void_p, _dp, C.c_int, _ip]
        buf, n = (C.c_double * cap)(), C.c_int()
        _check(lib.lorads_hip_profile_samples(ctx, buf, cap, C.byref(n)), "profile_samples")
        return [buf[i] for i in range(min(cap, n.value))]

    def hip_time_operator(self, reps):
        """milliseconds of `reps` applications of the live CG operator of cone 0, back to back (see lorads_hip_dev.h)"""
        lib, ctx = self._hip()
        ms = C.c_double()
        lib.lorads_hip_time_operator.argtypes = [C.c_void_p, C.c_int, _dp]
        rc = lib.lorads_hip_time_operator(ctx, int(reps), C.byref(ms))
        if rc:
            lib.lorads_hip_last_error.restype = C.c_char_p
            raise RuntimeError("time_operator: %s" % (lib.lorads_hip_last_error() or b"?").decode())
        return ms.value

    def hip_ubench(self, which, reps):
        """milliseconds of `reps` back-to-back launches of kernel variant `which`: DEVELOPMENT build only -- the session must have
        been attached with attach_hip(libpath=host.DEV_LIB) (profiles/tools/ubench.py)"""
        lib, ctx = self._hip()
        if not hasattr(lib, "lorads_hip_ubench"):
            raise RuntimeError("ubench: not in the product library (attach the session to host.DEV_LIB)")
        lib.lorads_hip_ubench.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        ms = C.c_double()
        rc = lib.lorads_hip_ubench(ctx, int(which), int(reps), C.byref(ms))
        if rc:
            lib.lorads_hip_last_error.restype = C.c_char_p
            raise RuntimeError("ubench: %s" % (lib.lorads_hip_last_error() or b"?").decode())
        return ms.value

    def hip_algorithmic_bytes(self, blk=0):
        lib, ctx = self._hip()
        a, b = C.c_double(), C.c_double()
        _check(lib.lorads_hip_algorithmic_bytes(ctx, blk, C.byref(a), C.byref(b)), "algorithmic_bytes")
        return a.value, b.value

    def hip_dual_infeasibility(self, tol=1e-2, ncv=40, max_restarts=600):
        """(sum_k |min(lambda_min_k, 0)|, per-cone lambda_min, S x products) straight from the C ABI"""
        lib, ctx = self._hip()
        lib.lorads_hip_dual_infeasibility.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, _dp, _dp, _ip]
        nb = self.nblk
        v, lm, mv = C.c_double(), (C.c_double * max(nb, 1))(), C.c_int()
        _check(lib.lorads_hip_dual_infeasibility(ctx, tol, ncv, max_restarts, C.byref(v), lm, C.byref(mv)), "dual_infeasibility")
        return v.value, [lm[i] for i in range(nb)], mv.value

    def hip_certificate(self, src, tol=1e-8, ncv=40, max_restarts=600):
        """(out[LORADS_HIP_CERT_N], per-cone lambda_min, A(X) - b, the multipliers of the certificate) straight from the C ABI;
        src: PAIR_UV (R = (U + V) / 2) or PAIR_RR; tol <= 0: no eigen-solves (NaN)"""
        lib, ctx = self._hip()
        lib.lorads_hip_certificate.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, _dp, _dp, _dp, _dp]
        nb, m = self.nblk, self.m
        out, lm = (C.c_double * 10)(), (C.c_double * max(nb, 1))()
        res, lam = (C.c_double * max(m, 1))(), (C.c_double * max(m, 1))()
        _check(lib.lorads_hip_certificate(ctx, int(src), tol, ncv, max_restarts, out, lm, res, lam), "certificate")
        return (np.array(out[:10]), np.array(lm[:nb]), np.array(res[:m]), np.array(lam[:m]))

    def hip_get_slack(self, blk):
        """(row, col, val) of S_blk as lower-triangle triplets, straight from the C ABI (lorads_hip_get_slack)"""
        lib, ctx = self._hip()
        i32p = C.POINTER(C.c_int32)
        lib.lorads_hip_get_slack.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), i32p, i32p, _dp]
        nnz = C.c_int64()
        _check(lib.lorads_hip_get_slack(ctx, int(blk), C.byref(nnz), None, None, None), "get_slack")
        row, col, val = np.zeros(nnz.value, dtype=np.int32), np.zeros(nnz.value, dtype=np.int32), np.zeros(nnz.value)
        _check(lib.lorads_hip_get_slack(ctx, int(blk), C.byref(nnz), row.ctypes.data_as(i32p), col.ctypes.data_as(i32p),
                                        val.ctypes.data_as(_dp)), "get_slack")
        return row, col, val

    def hip_block_image(self, blk=0):
        """what lorads_hip_create built for cone blk (see lorads_hip_dev.h)"""
        lib, ctx = self._hip()
        out = (C.c_int64 * 16)()
        lib.lorads_hip_block_image.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_block_image(ctx, blk, out), "block_image")
        keys = ["n", "rank", "nrow", "na", "nc", "pattern_a", "pattern_union", "dense_c", "dense_a", "diag_only", "entry_only", "use_cw",
                "has_gram", "front_cw", "slot_width", "bip_rows0"]
        return dict(zip(keys, [int(out[i]) for i in range(16)]))

    def hip_cw_layout(self, blk=0):
        """{ca_ell, cs_w, cell_w, rows_over}: the layout of cone blk's constraint-wise operator (see lorads_hip_dev.h)"""
        lib, ctx = self._hip()
        out = (C.c_int64 * 4)()
        lib.lorads_hip_cw_layout.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_cw_layout(ctx, blk, out), "cw_layout")
        return dict(zip(["ca_ell", "cs_w", "cell_w", "rows_over"], [int(out[i]) for i in range(4)]))

    def hip_spec_front_stats(self):
        """{enqueued, adopted, discarded, blocked} of the next step's U front enqueued behind a step's hand-over (LORADS_SPEC_FRONT)"""
        lib, ctx = self._hip()
        out = (C.c_int64 * 4)()
        lib.lorads_hip_spec_front_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_spec_front_stats(ctx, out), "spec_front_stats")
        return dict(zip(["enqueued", "adopted", "discarded", "blocked"], [int(out[i]) for i in range(4)]))

    def hip_handover_stats(self):
        """{on_front, alone}: result hand-overs carried on the launch of the next step's U front / launched as kernels of their own
        (LORADS_HANDOVER_ON_FRONT)"""
        lib, ctx = self._hip()
        out = (C.c_int64 * 2)()
        lib.lorads_hip_handover_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_handover_stats(ctx, out), "handover_stats")
        return dict(zip(["on_front", "alone"], [int(out[i]) for i in range(2)]))

    def hip_row_deal_stats(self, blk=0):
        """{rpw, grid, ncu}: rows per workgroup and grid of k_front_cw / k_spmm_ell on cone `blk`, compute units dealt over (LORADS_ROW_DEAL)"""
        lib, ctx = self._hip()
        out = (C.c_int * 3)()
        lib.lorads_hip_row_deal_stats.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int)]
        _check(lib.lorads_hip_row_deal_stats(ctx, blk, out), "row_deal_stats")
        return dict(zip(["rpw", "grid", "ncu"], [int(out[i]) for i in range(3)]))

    def hip_wt_stores(self):
        """the mask of row outputs that k_front_cw / k_spmm_ell store through the L2 in this context (LORADS_WT_STORES)"""
        lib, ctx = self._hip()
        out = C.c_int(-1)
        lib.lorads_hip_wt_stores.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        _check(lib.lorads_hip_wt_stores(ctx, C.byref(out)), "wt_stores")
        return int(out.value)

    def hip_front_chain(self, effective=False):
        """the mask of cuts in the solve front's chain of dependent loads in this context (LORADS_FRONT_CHAIN); effective: 0
        unless some cone launches the form of the front that takes them (the LDS park: r <= 48, LORADS_FRONT_LDS on)"""
        lib, ctx = self._hip()
        out, eff = C.c_int(-1), C.c_int(-1)
        lib.lorads_hip_front_chain.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _check(lib.lorads_hip_front_chain(ctx, C.byref(out), C.byref(eff)), "front_chain")
        return int(eff.value if effective else out.value)

    def hip_dense_plan(self, blk=0):
        """{npad, ksplit, launches: [(col0, nt, rem), ...]}: what the dense-coefficient GEMM (k_dense_cx_b) launches for cone `blk` at
        its current device rank -- n padded to 64, the K split over workgroups, and per launch its first column, its column tiles of
        16 and its single columns (LORADS_DENSE_REM).  Zeros and no launch for a cone without dense storage.  kept: the factor whose
        products with the dense constraint matrices are kept at this moment ("", "U", "V" or "other")."""
        lib, ctx = self._hip()
        out = (C.c_int64 * 16)()
        lib.lorads_hip_dense_plan.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_dense_plan(ctx, blk, out), "dense_plan")
        return dict(npad=int(out[0]), ksplit=int(out[1]), launches=[tuple(int(out[3 + 3 * i + j]) for j in range(3)) for i in range(int(out[2]))],
                    kept=("", "U", "V", "other")[int(out[15])])

    def hip_graph_stats(self):
        """{captured, replayed, held, enabled} of the launch-chain replay (hipGraph) of this context"""
        lib, ctx = self._hip()
        out = (C.c_int64 * 4)()
        lib.lorads_hip_graph_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_graph_stats(ctx, out), "graph_stats")
        return dict(zip(["captured", "replayed", "held", "enabled"], [int(out[i]) for i in range(4)]))

    def hip_persist_stats(self):
        """the one-launch ADMM iteration of Max-Cut-type cones (csrc/hip/persist.inc): {iterations run that way, available now,
        workgroups, rows per lane group, column steps, LDS bytes}"""
        lib, ctx = self._hip()
        out = (C.c_int64 * 6)()
        lib.lorads_hip_persist_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_persist_stats(ctx, out), "persist_stats")
        return dict(zip(["iterations", "available", "workgroups", "rows", "column_steps", "lds_bytes"], [int(out[i]) for i in range(6)]))

    def hip_persist_plan(self):
        """the host's plan of the one-launch ADMM iteration: {next tag (-1: no valid plan), xcd_map (every team on one XCD's blocks; 0: dealt team by team),
        largest team, most sub-teams of a team, largest sub-team, workgroups per CU counted on, CUs, allow_l2}"""
        lib, ctx = self._hip()
        out = (C.c_int64 * 8)()
        lib.lorads_hip_persist_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_persist_plan(ctx, out), "persist_plan")
        return dict(zip(["tag", "xcd_map", "team", "sub_teams", "sub_team", "occ", "ncu", "allow_l2"], [int(out[i]) for i in range(8)]))

    def hip_persist_set_tag(self, tag):
        """measurement: the 32-bit tag the next one-launch iteration starts from (refused when no plan is valid)"""
        lib, ctx = self._hip()
        lib.lorads_hip_persist_set_tag.argtypes = [C.c_void_p, C.c_uint32]
        _check(lib.lorads_hip_persist_set_tag(ctx, int(tag)), "persist_set_tag")

    def hip_launch_count(self):
        """kernels this context has enqueued so far"""
        lib, ctx = self._hip()
        out = C.c_int64(0)
        lib.lorads_hip_launch_count.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_launch_count(ctx, C.byref(out)), "launch_count")
        return int(out.value)

    @staticmethod
    def hip_memory_stats(libpath=None):
        """device and pinned memory the HIP library's contexts of this process hold now: {device_allocations, device_bytes,
        pinned_allocations, pinned_bytes}.  Needs no session: it still answers after the last one has been closed."""
        lib = C.CDLL(libpath or os.path.join(LIB_DIR, "liblorads_hip.so"))
        out = (C.c_int64 * 4)()
        lib.lorads_hip_memory_stats.argtypes = [C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_memory_stats(out), "memory_stats")
        return dict(zip(("device_allocations", "device_bytes", "pinned_allocations", "pinned_bytes"), [int(out[i]) for i in range(4)]))

    def hip_lbfgs_team_stats(self):
        """phase 1's one-launch L-BFGS history update + direction (csrc/hip/lbfgs_team.inc): {launches, available, workgroups, pairs}"""
        lib, ctx = self._hip()
        out = (C.c_int64 * 4)()
        lib.lorads_hip_lbfgs_team_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_lbfgs_team_stats(ctx, out), "lbfgs_team_stats")
        return dict(zip(("launches", "available", "workgroups", "pairs"), [int(out[i]) for i in range(4)]))

    def hip_persist_stamps(self, enable=True):
        """100 MHz clock of cone 0's leader workgroup at the phase boundaries of the latest one-launch iteration (0: not taken)"""
        lib, ctx = self._hip()
        out = (C.c_uint64 * 16)()
        lib.lorads_hip_persist_stamps.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
        _check(lib.lorads_hip_persist_stamps(ctx, 1 if enable else 0, out), "persist_stamps")
        return [int(out[i]) for i in range(16)]

    def hip_presolve_stats(self):
        """{device: patterns built by the device sorts, checked: of these compared with the host construction}"""
        lib, ctx = self._hip()
        out = (C.c_int64 * 2)()
        lib.lorads_hip_presolve_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_presolve_stats(ctx, out), "presolve_stats")
        return {"device": int(out[0]), "checked": int(out[1])}

    def hip_operator_kind(self, blk=0):
        lib, ctx = self._hip()
        k = C.c_int()
        _check(lib.lorads_hip_operator_kind(ctx, blk, C.byref(k)), "operator_kind")
        base = ["k_pairdots+k_sgram+k_spmm2", "k_pairdots+k_cv+k_sval+k_spmm2", "k_op_diag", "k_op_entry", "k_cw+k_spmm_ell"][k.value & 15]
        if k.value & 32:   # bipartite entry graph: one launch per colour
            base = "k_op_entry_bip+k_op_entry_bip"
        return base + ("+k_dense_cx_b(dense A_i)" if k.value & 16 else "")

    def hip_stream(self):
        """hipStream_t of the library as an integer (torch.cuda.ExternalStream takes it)"""
        lib, ctx = self._hip()
        return lib.lorads_hip_stream(ctx)

    def hip_allreduce_stream_ordered(self, on):
        lib, ctx = self._hip()
        _check(lib.lorads_hip_set_allreduce_stream_ordered(ctx, int(on)), "set_allreduce_stream_ordered")

    def hip_selfcheck_allreduce(self):
        lib, ctx = self._hip()
        lib.lorads_hip_selfcheck_allreduce.argtypes = [C.c_void_p]
        _check(lib.lorads_hip_selfcheck_allreduce(ctx), "selfcheck_allreduce")

    def hip_sync(self):
        lib, ctx = self._hip()
        _check(lib.lorads_hip_sync(ctx), "sync")

    def set_allreduce(self, fn):
        """fn(ptr:int, count:int, on_device:bool) -> sums in place over ranks."""
        def _cb(user, buf, count, on_device):
            try:
                fn(buf, count, bool(on_device))
                return 0
            except Exception as e:  # noqa: BLE001 - must not unwind into C
                print("allreduce hook failed:", e)
                return 1
        cb = ALLREDUCE_FN(_cb)
        self._keep.append(cb)
        self.lib.lrd_session_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p]
        _check(self.lib.lrd_session_set_allreduce(self.h, cb, None), "set_allreduce")

    def set_allreduce_native(self, fn_ptr, user):
        """a C function of type lorads_hip_allreduce_fn (address) and its user pointer: no Python in the hook"""
        self.lib.lrd_session_set_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _check(self.lib.lrd_session_set_allreduce(self.h, fn_ptr, C.c_void_p(user)), "set_allreduce")

    def set_scalar_exchange_shm(self, name, world, rank):
        """Separable shards on one node: the evaluation's four scalars are summed by the ranks' hosts through a page of POSIX shared
        memory (csrc/host/shmx.c) instead of a collective on the stream (lorads_hip_set_scalar_exchange).  name: '/...', the same on
        every rank and unique per run.  Returns the exchange's handle (closed by close())."""
        lib, ctx = self._hip()
        h = C.c_void_p()
        self.lib.lrd_shmx_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        _check(self.lib.lrd_shmx_open(name.encode(), int(world), int(rank), C.byref(h)), "shmx_open")
        lib.lorads_hip_set_scalar_exchange.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _check(lib.lorads_hip_set_scalar_exchange(ctx, C.cast(self.lib.lrd_shmx_hook, C.c_void_p), h), "set_scalar_exchange")
        self._shmx = h
        return h

    def hip_scalar_exchange_count(self):
        lib, ctx = self._hip()
        n = C.c_int64()
        lib.lorads_hip_scalar_exchange_count.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _check(lib.lorads_hip_scalar_exchange_count(ctx, C.byref(n)), "scalar_exchange_count")
        return int(n.value)

    def clear_scalar_exchange(self):
        lib, ctx = self._hip()
        lib.lorads_hip_set_scalar_exchange.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _check(lib.lorads_hip_set_scalar_exchange(ctx, None, None), "set_scalar_exchange")

    def shmx_allreduce(self, values):
        """sums `values` (<= 16 doubles) over the ranks through the exchange opened by set_scalar_exchange_shm (tests, agreement steps)"""
        v = (C.c_double * len(values))(*values)
        self.lib.lrd_shmx_allreduce.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        _check(self.lib.lrd_shmx_allreduce(self._shmx, v, len(values)), "shmx_allreduce")
        return list(v)

    def use_fused_step(self, on):
        self.lib.lrd_session_use_fused_step.argtypes = [C.c_void_p, C.c_int]
        _check(self.lib.lrd_session_use_fused_step(self.h, int(on)), "use_fused_step")

    def solve(self):
        _check(self.lib.lrd_session_solve(self.h), "solve")
        return self.results()

    def alm(self):
        return self.lib.lrd_session_alm(self.h)

    def alm_to_admm(self):
        self.lib.lrd_session_alm_to_admm(self.h)

    def admm(self, iter_ceiling):
        return self.lib.lrd_session_admm(self.h, iter_ceiling)

    def admm_steps(self, steps, rho, err1):
        """`steps` ADMM iterations in the C host loop (no per-iteration Python); returns (err1, cg, pobj, dobj)"""
        io = (C.c_double * 4)(err1, 0.0, 0.0, 0.0)
        self.lib.lrd_session_admm_steps.argtypes = [C.c_void_p, C.c_int, C.c_double, _dp]
        _check(self.lib.lrd_session_admm_steps(self.h, int(steps), float(rho), io), "admm_steps")
        return io[0], int(io[1]), io[2], io[3]

    def results(self):
        out = (C.c_double * 16)()
        _check(self.lib.lrd_session_results(self.h, out), "results")
        res = dict(zip(RESULT_KEYS, [out[i] for i in range(16)]))
        o2 = (C.c_double * 4)()
        _check(self.lib.lrd_session_results2(self.h, o2), "results2")
        res.update(dual_infeas_l1=o2[0], dual_infeas_inf=o2[1], t_dual_infeas=o2[2], scale_obj_his=o2[3])
        return res

    def _solution_ptr(self, tol):
        from .solution import SolutionStruct
        ptr = C.POINTER(SolutionStruct)()
        self.lib.lrd_session_solution.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.POINTER(SolutionStruct))]
        self.lib.lrd_solution_free.argtypes = [C.POINTER(SolutionStruct)]
        rc = self.lib.lrd_session_solution(self.h, float(tol), C.byref(ptr))
        if rc == 2:
            raise NotImplementedError("the attached backend (%s) cannot export a solution: only the HIP backend computes the "
                                      "certificate" % (self.be.name if self.be else "none"))
        if rc == 3:
            raise NotImplementedError("exporting the solution of a sharded deal (world > 1) is not supported")
        _check(rc, "solution")
        return ptr

    def solution(self, tol=1e-8):
        """The current primal-dual point and its DIMACS certificate in the file's units (lorads_amd.solution.Solution): per cone
        R, U, V (X = R R^T) or x (LP block), y, the slack S = C - sum_i y_i A_i and the certificate.  Read-only: the next
        iteration computes what it would have computed without the call."""
        from .solution import Solution
        ptr = self._solution_ptr(tol)
        try:
            return Solution.from_struct(ptr.contents)
        finally:
            self.lib.lrd_solution_free(ptr)

    def write_solution(self, path, tol=1e-8):
        """the solution file of the command line's --solutionFile (the same C writer: the same bytes)"""
        from .solution import SolutionStruct
        ptr = self._solution_ptr(tol)
        try:
            self.lib.lrd_solution_write.argtypes = [C.c_char_p, C.POINTER(SolutionStruct)]
            _check(self.lib.lrd_solution_write(os.fsencode(path), ptr), "solution_write")
        finally:
            self.lib.lrd_solution_free(ptr)

    def _refused(self, rc, what_rc2, what_rc3):
        """the refusals of a post-solve entry point: rc 2 (what_rc2 takes the backend's name and, behind ": ", the HIP backend's own
        reason) and rc 3 (a sharded deal)"""
        if rc == 2:
            msg = None
            if self.be is not None and self.be.name == "hip-gfx950":
                lib, _ = self._hip()
                lib.lorads_hip_last_error.restype = C.c_char_p
                msg = (lib.lorads_hip_last_error() or b"").decode()
            raise NotImplementedError(what_rc2 % (self.be.name if self.be else "attached", (": " + msg) if msg else ""))
        if rc == 3:
            raise NotImplementedError(what_rc3)

    def _rounded(self, key, path, trials, seed, local_search_rounds, tol, extra=False, parts=None):
        """One call of the rounding `key` of _ROUNDINGS: its result object (path None; None for trials = 0, which checks
        applicability alone) or, through the C writer, its file at `path`.  extra: also the hyperplanes / vectors / scores."""
        R = _ROUNDINGS[key]
        mod = importlib.import_module("." + R["module"], __package__)
        st = getattr(mod, R["struct"])
        who = R["name"]
        if R["checked"]:
            trials, local_search_rounds = int(trials), int(local_search_rounds)
            if parts is not None:
                parts = int(parts)
                if not 2 <= parts <= 64:
                    raise ValueError("%s: parts %d is outside [2, 64]" % (who, parts))
            if not 0 <= trials <= 65536:
                raise ValueError("%s: trials %d is outside [0, 65536]" % (who, trials))
            if parts is not None and trials * parts > 1 << 20:
                raise ValueError("%s: trials x parts = %d is above 2^20" % (who, trials * parts))
            if local_search_rounds < 0:
                raise ValueError("%s: local_search_rounds %d is negative" % (who, local_search_rounds))
        run, free, write = (getattr(self.lib, R[f]) for f in ("run", "free", "write"))
        lead = [] if parts is None else [int(parts)]
        run.argtypes = [C.c_void_p] + [C.c_int] * len(lead) + [C.c_int, C.c_uint64, C.c_int, C.c_double, C.c_int, C.POINTER(C.POINTER(st))]
        free.argtypes, free.restype = [C.POINTER(st)], None
        ptr = C.POINTER(st)()
        rc = run(self.h, *lead, int(trials), int(seed) & 0xFFFFFFFFFFFFFFFF, int(local_search_rounds), float(tol),
                 1 if extra and trials != 0 else 0, C.byref(ptr))
        self._refused(rc, R["refusal"] + " or the %s backend cannot round%s",
                      "rounding the solution of a sharded deal (world > 1) is not supported")
        _check(rc, who)
        if path is None and trials == 0:
            return None
        try:
            if path is None:
                return getattr(mod, R["result"]).from_struct(ptr.contents)
            write.argtypes = [C.c_char_p, C.POINTER(st)]
            _check(write(os.fsencode(path), ptr), R["write"][4:])
        finally:
            free(ptr)

    def round_pm1(self, trials=1024, seed=0, local_search_rounds=100, tol=1e-8, hyperplanes=False):
        """Goemans-Williamson hyperplane rounding of the current point with a 1-flip local search, on the device
        (lorads_amd.rounding.Rounding, file units): per trial f = x^T C x before and after the search, the best trial's signs and
        x = sigma o t per cone, and the dual bound d = b.y + sum_k T_k min(0, lambda_min(S_k)) at Lanczos tolerance tol (tol <= 0:
        NaN).  On a cut-tightened problem (what write_tightened wrote) d also has the slacks' term sum_j u_j min(0, s_j), u_j = 4.
        trials = 0 checks applicability alone (None).  Read-only on the solver's state."""
        return self._rounded("pm1", None, trials, seed, local_search_rounds, tol, hyperplanes)

    def write_rounding(self, path, trials=1024, seed=0, local_search_rounds=100, tol=1e-8):
        """the rounding file of the command line's --roundFile (the same C writer: the same bytes)"""
        self._rounded("pm1", path, trials, seed, local_search_rounds, tol)

    def round_kcut(self, parts, trials=1024, seed=0, local_search_rounds=100, tol=1e-8, vectors=False):
        """Frieze-Jerrum rounding of the current point into `parts` parts with a 1-move local search, on the device
        (lorads_amd.kcut.KCut, file units): per trial f = sum <C, X(l)> before and after the search, the best trial's labels and
        part sizes per cone, and the dual bound d = b.y + sum_k T_k min(0, lambda_min(S_k)) + sum_j u_j min(0, s_j) at Lanczos
        tolerance tol (tol <= 0: NaN).  Works on +-1-structured problems and on what write_bounded makes of them.  trials = 0
        checks applicability alone (None).  Read-only on the solver's state."""
        return self._rounded("kcut", None, trials, seed, local_search_rounds, tol, vectors, parts)

    def write_kcut(self, path, parts, trials=1024, seed=0, local_search_rounds=100, tol=1e-8):
        """the k-cut file of the command line's --kcutFile (the same C writer: the same bytes)"""
        self._rounded("kcut", path, trials, seed, local_search_rounds, tol, parts=parts)

    def round_stable(self, trials=1024, seed=0, local_search_rounds=100, tol=1e-8, scores=False):
        """Stable sets of a theta-structured problem's graphs read off the current point, on the device (lorads_amd.stable.StableSet,
        file units): per trial the greedy set in the order of the vertices' priorities (trial 0: X_pp; trial t: F_p . g_t) and a
        (1, 2)-swap search, f = sum <C, X(S)> with X(S) = T 1_S 1_S^T / |S| before and after the search, the best trial's members
        and sizes per cone, and the dual bound d = b.y + sum_k T_k min(0, lambda_min(S_k)) + sum_j u_j min(0, s_j) at Lanczos
        tolerance tol (tol <= 0: NaN): for the theta files |S| <= alpha <= floor(-d).  trials = 0 checks applicability alone
        (None).  Read-only on the solver's state."""
        return self._rounded("stable", None, trials, seed, local_search_rounds, tol, scores)

    def write_stable(self, path, trials=1024, seed=0, local_search_rounds=100, tol=1e-8):
        """the stable-set file of the command line's --stableFile (the same C writer: the same bytes)"""
        self._rounded("stable", path, trials, seed, local_search_rounds, tol)

    def round_bisection(self, trials=1024, seed=0, local_search_rounds=1000, tol=1e-8, hyperplanes=False):
        """Balanced partitions of a bisection-structured problem read off the current point, on the device
        (lorads_amd.bisection.Bisection, file units): per trial the +-1 rounding's hyperplane signs, the repair to
        sum(sigma) = +-d, and a swap search that keeps the balance; f = sum x^T C x after the repair and after the search, the
        best trial's signs and part sizes per cone, and the dual bound d = b.y + sum_k n_k t_k^2 min(0, lambda_min(S_k)) at Lanczos
        tolerance tol (tol <= 0: NaN).  trials = 0 checks applicability alone (None).  Read-only on the solver's state."""
        return self._rounded("bisection", None, trials, seed, local_search_rounds, tol, hyperplanes)

    def write_bisection(self, path, trials=1024, seed=0, local_search_rounds=1000, tol=1e-8):
        """the bisection file of the command line's --bisectFile (the same C writer: the same bytes)"""
        self._rounded("bisection", path, trials, seed, local_search_rounds, tol)

    def triangle_cuts(self, max_cuts=1000, min_violation=1e-3):
        """Separation of the triangle inequalities of a +-1-structured problem at the current point, on the device
        (lorads_amd.cuts.Cuts): with rho_xy = X_xy / (t_x t_y) all 4 C(n, 3) inequalities of every cone are enumerated (X is never
        formed), the ones violated by more than min_violation counted exactly, and the max_cuts most violated returned, ordered by
        (violation descending, cone, p, q, s, cls ascending).  On a cut-tightened problem (what write_tightened wrote) the
        inequalities that are rows already are neither counted nor returned.  Read-only on the solver's state, deterministic."""
        from .cuts import Cuts, CutsStruct
        return self._separated(CutsStruct, Cuts, "lrd_session_triangle_cuts", "lrd_cuts_free", [min_violation], max_cuts,
                               "triangle inequalities cannot be separated: the problem is not +-1-structured or the %s backend "
                               "cannot separate%s")

    def _separated(self, struct, result, run, free, lead, max_cuts, what_rc2):
        """One separation of the current point: the entry point `run` with the doubles `lead`, max_cuts and the list's address, the
        refusals (what_rc2 as _refused takes it), and `result` of the list, which `free` releases."""
        run, free = getattr(self.lib, run), getattr(self.lib, free)
        run.argtypes = [C.c_void_p] + [C.c_double] * len(lead) + [C.c_int, C.POINTER(C.POINTER(struct))]
        free.argtypes, free.restype = [C.POINTER(struct)], None
        ptr = C.POINTER(struct)()
        rc = run(self.h, *(float(x) for x in lead), int(max_cuts), C.byref(ptr))
        self._refused(rc, what_rc2, "the separation of a sharded deal (world > 1) is not supported")
        _check(rc, run.__name__[len("lrd_session_"):])
        try:
            return result.from_struct(ptr.contents)
        finally:
            free(ptr)

    def _written(self, write, path, struct, lst, argtypes=(), args=()):
        """the return code of the writer `write` for the session, path, the list (an object with to_struct, or None) and `args`"""
        write = getattr(self.lib, write)
        write.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(struct)] + list(argtypes)
        st = lst.to_struct() if lst is not None else None
        return write(self.h, os.fsencode(path), C.byref(st) if st is not None else None, *args)

    def _cuts_why(self):
        self.lib.lrd_cuts_why.restype = C.c_char_p
        return (self.lib.lrd_cuts_why() or b"").decode()

    def present_cuts(self):
        """The triangle cuts a cut-tightened problem holds, read off the problem as it was opened: a list of
        lorads_amd.cuts.PresentCut (cone, p, q, s, cls, row, column; 0-based, in constraint order).  [] without an LP block;
        ValueError with the first reason when the LP block's columns are not all triangle-cut slacks (the device's rule and words)."""
        from .cuts import PresentCut, PresentStruct
        ptr = C.POINTER(PresentStruct)()
        self.lib.lrd_session_present_cuts.argtypes = [C.c_void_p, C.POINTER(C.POINTER(PresentStruct))]
        self.lib.lrd_present_free.argtypes, self.lib.lrd_present_free.restype = [C.POINTER(PresentStruct)], None
        rc = self.lib.lrd_session_present_cuts(self.h, C.byref(ptr))
        if rc == 2:
            raise ValueError(self._cuts_why())
        if rc == 3:
            raise NotImplementedError("the cuts of a sharded deal (world > 1) are not supported")
        _check(rc, "present_cuts")
        try:
            st = ptr.contents
            return [PresentCut(st.cone[e], st.p[e], st.q[e], st.s[e], st.cls[e], st.row[e], st.col[e], st.scale[e]) for e in range(st.n)]
        finally:
            self.lib.lrd_present_free(ptr)

    def write_tightened(self, path, cuts, drop_slack=None, keep=None):
        """The problem as it was read plus one constraint and one slack column per cut, in SDPA sparse format (the command line's
        --cutsFile: the same C writer, the same bytes).  cuts: a lorads_amd.cuts.Cuts or None.  The slacks are a new last LP block, or,
        on a cut-tightened problem, new columns behind its own.  There, drop_slack: a present cut leaves (its row and column with
        it, the others renumbered in order) when its slack in the row's rho units, x_j / scale_j = 1 + sum sign rho at the current
        point, exceeds it (the command line's --cutsDropSlack); keep: the mask itself, one flag per present_cuts() entry.
        Returns how many present cuts left."""
        from .cuts import CutsStruct
        dropped = C.c_int(0)
        if keep is not None:
            if drop_slack is not None:
                raise ValueError("write_tightened: drop_slack and keep exclude each other")
            mask = np.ascontiguousarray(np.asarray(keep, dtype=bool), dtype=np.uint8)
            rc = self._written("lrd_session_write_tightened_keep", path, CutsStruct, cuts, [C.c_void_p, C.c_int],
                               [mask.ctypes.data_as(C.c_void_p), len(mask)])
            dropped.value = int(len(mask) - mask.sum())
        elif drop_slack is not None:
            rc = self._written("lrd_session_write_tightened_drop", path, CutsStruct, cuts, [C.c_double, C.c_double, C.POINTER(C.c_int)],
                               [float(drop_slack), 1e-8, C.byref(dropped)])
        else:
            rc = self._written("lrd_session_write_tightened", path, CutsStruct, cuts)
        if rc == 2:
            why = self._cuts_why()
            raise ValueError("a cut lies outside the problem, names a row no constraint fixes, or the problem has an LP block that "
                             "is not all cut slacks" + (": " + why if why else ""))
        _check(rc, "write_tightened")
        return dropped.value

    def entry_bounds(self, max_cuts=1000, lower=0.0, upper=None, min_violation=1e-3):
        """Separation of the entry bounds lower <= X_pq <= upper (p < q) of every SDP cone at the current point, on the device
        (lorads_amd.bounds.Bounds): all n (n - 1) inequalities of every cone are enumerated (X is never formed), the ones violated by
        more than min_violation counted exactly, and the max_cuts most violated returned, ordered by (violation descending, cone, p,
        q, cls ascending).  lower=None / upper=None: no such bound.  Any problem; read-only on the solver's state, deterministic."""
        from .bounds import Bounds, BoundsStruct
        lead = [-np.inf if lower is None else lower, np.inf if upper is None else upper, min_violation]
        return self._separated(BoundsStruct, Bounds, "lrd_session_entry_bounds", "lrd_bounds_free", lead, max_cuts,
                               "entry bounds cannot be separated: the %s backend has no such slot%.0s")   # (without the backend's reason)

    def write_bounded(self, path, bounds):
        """The problem as it was read plus one constraint and one slack column per bound cut, in SDPA sparse format (the command
        line's --boundsFile: the same C writer, the same bytes).  The slack columns join the problem's LP block, or form a new last
        one.  bounds: a lorads_amd.bounds.Bounds or None."""
        from .bounds import BoundsStruct
        rc = self._written("lrd_session_write_bounded", path, BoundsStruct, bounds)
        if rc == 2:
            raise ValueError("a bound cut lies outside the problem, or the problem has more than one LP block")
        if rc == 3:
            raise NotImplementedError("the bounded problem of a sharded deal (world > 1) is not supported")
        _check(rc, "write_bounded")

    def _spectral_refused(self, rc, what):
        if rc == 2:
            raise NotImplementedError("the attached backend (%s) cannot compute the %s: only the HIP backend does"
                                      % (self.be.name if self.be else "none", what))
        if rc == 3:
            raise NotImplementedError("the %s of a sharded deal (world > 1) is not supported" % what)
        _check(rc, what)

    def spectrum(self, sweeps=False):
        """Per SDP cone the eigenvalues (descending) of F^T F, F = (U + V) / 2 in phase 2 and the phase-1 R otherwise, at the cone's
        own rank: the non-zero eigenvalues of X = F F^T.  Computed on the device (Gram on the matrix cores, cyclic Jacobi); read-only
        on the solver's state.  A list with one array per block (empty for the LP block); sweeps=True: also the Jacobi sweep counts."""
        ranks = [self.block_shape(k)[1] for k in range(self.nblk)]
        lp = self._lp_blocks()
        ranks = [0 if lp[k] else ranks[k] for k in range(self.nblk)]
        eig = np.zeros(max(sum(ranks), 1))
        sw = np.zeros(max(self.nblk, 1), dtype=np.int32)
        self.lib.lrd_session_spectrum.argtypes = [C.c_void_p, _dp, _ip]
        self._spectral_refused(self.lib.lrd_session_spectrum(self.h, eig.ctypes.data_as(_dp), sw.ctypes.data_as(_ip)), "spectrum of the solution")
        out, at = [], 0
        for r in ranks:
            out.append(eig[at:at + r].copy())
            at += r
        return (out, [int(x) for x in sw[:self.nblk]]) if sweeps else out

    def _lp_blocks(self):
        self.lib.lrd_session_block_is_lp.argtypes = [C.c_void_p, C.c_int]
        return [bool(self.lib.lrd_session_block_is_lp(self.h, k)) for k in range(self.nblk)]

    def compress_rank(self, tol=1e-12, max_rank=None, ranks=None):
        """Replace every SDP cone's factor by its top-k spectral factor F Q[:, :k] (R = U = V; mutually orthogonal columns of squared
        norms lambda_1 >= lambda_2 >= ...), k = max(1, min(max_rank, #{j : lambda_j > tol lambda_1})) -- or ranks[k] given per block
        (1 <= ranks[k] <= current rank; the current rank: a pure rotation, X unchanged).  Constraint values, objective and err1 are
        refreshed.  Returns the report as a dict: per block rank before / after, eigenvalues, sweeps, the trace share lost and the
        predicted ||X - X_k||_F / ||X||_F; pobj and err1 before and after."""
        ptr = C.POINTER(SpectralReportStruct)()
        self.lib.lrd_session_compress_ex.argtypes = [C.c_void_p, C.c_double, C.c_int, _ip, C.POINTER(C.POINTER(SpectralReportStruct))]
        self.lib.lrd_spectral_report_free.argtypes = [C.POINTER(SpectralReportStruct)]
        if self._rank_override is not None and \
                self._rank_override != [self.lib.lrd_session_current_rank(self.h, k) for k in range(self.nblk)]:
            # (Backend.resize_rank / Backend.compress_rank went past the host: its record sizes the buffers and feeds the rank rule)
            raise RuntimeError("the ranks were changed through the backend table (%s), the host's record is stale: use "
                               "Backend.compress_rank" % self._rank_override)
        rk = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.int32)
        if rk is not None and len(rk) != self.nblk:
            raise ValueError("ranks: one entry per block")
        rc = self.lib.lrd_session_compress_ex(self.h, float(tol), int(max_rank) if max_rank else 0,
                                              rk.ctypes.data_as(_ip) if rk is not None else None, C.byref(ptr))
        self._spectral_refused(rc, "rank reduction of the solution")
        self._rank_override = None  # (the host's record of the ranks is the current one)
        try:
            r = ptr.contents
            cones = []
            for k in range(r.nblk):
                q = r.cone[k]
                cones.append(dict(n=q.n, is_lp=bool(q.is_lp), rank_before=q.rank_before, rank_after=q.rank_after, sweeps=q.sweeps,
                                  eig=np.array([q.eig[j] for j in range(q.rank_before)]) if q.eig else np.zeros(0),
                                  trace_lost=q.trace_lost, frob_lost=q.frob_lost))
            return dict(src=r.src, tol=r.tol, max_rank=r.cap or None, pobj_before=r.pobj_before, pobj_after=r.pobj_after,
                        err1_before=r.err1_before, err1_after=r.err1_after, cones=cones)
        finally:
            self.lib.lrd_spectral_report_free(ptr)

    def _primal_refused(self, rc, what):
        if rc == 2:
            raise NotImplementedError("the attached backend (%s) cannot query the primal: only the HIP backend does"
                                      % (self.be.name if self.be else "none"))
        if rc == 3:
            raise NotImplementedError("%s of a sharded deal (world > 1) is not supported" % what)
        _check(rc, what)

    def primal_entries(self, blk, rows, cols, ref=None):
        """Entries X[rows[e], cols[e]] of block blk's primal X = F F^T (0-based; F = (U + V) / 2 in phase 2, the phase-1 R otherwise;
        LP block: X = diag(f^2)), computed on the device without forming X; read-only on the solver's state.  Returns (val, stats):
        stats is None without ref, else {sum (val - ref)^2, sum |val - ref|, max |val - ref|, sum ref^2} formed on the device."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        c = np.ascontiguousarray(cols, dtype=np.int32)
        if r.ndim != 1 or r.shape != c.shape:
            raise ValueError("rows and cols: two vectors of one length")
        f = None if ref is None else np.ascontiguousarray(ref, dtype=np.float64)
        if f is not None and f.shape != r.shape:
            raise ValueError("ref: one value per position")
        val = np.zeros(max(len(r), 1))
        st = np.zeros(4) if f is not None else None
        rc = self.lib.lrd_session_primal_entries(self.h, int(blk), len(r), r.ctypes.data_as(_ip), c.ctypes.data_as(_ip),
                                                 val.ctypes.data_as(_dp), f.ctypes.data_as(_dp) if f is not None else None,
                                                 st.ctypes.data_as(_dp) if st is not None else None)
        self._primal_refused(rc, "entries of the primal")
        return val[:len(r)], st

    def primal_apply(self, blk, B, return_t=False):
        """Y = X_blk B for B (n, ncols) or (n,), 1 <= ncols <= 1024, as Y = F (F^T B) on the device's matrix cores; with return_t
        also T = F^T B (rank x ncols; not on the LP block).  Read-only on the solver's state.  The library takes B column-major: a
        C-ordered B is copied first (DESIGN.md section 13 has what that costs at 64 columns)."""
        n, rank = self.block_shape(blk)
        B = np.asarray(B, dtype=np.float64)
        vec = B.ndim == 1
        Bf = np.asfortranarray(B.reshape(n, -1))
        nc = Bf.shape[1]
        Y = np.zeros((n, max(nc, 1)), order="F")
        T = np.zeros((rank, max(nc, 1)), order="F") if return_t else None
        rc = self.lib.lrd_session_primal_apply(self.h, int(blk), nc, Bf.ctypes.data_as(_dp), Y.ctypes.data_as(_dp),
                                               T.ctypes.data_as(_dp) if return_t else None)
        self._primal_refused(rc, "a product with the primal")
        Y = Y[:, 0] if vec else Y
        if return_t:
            return Y, (T[:, 0] if vec else T)
        return Y

    def primal_topk(self, blk, rows, k, cols=None, smallest=False, include_diag=False, skip=None, skip_constrained=False):
        """Per query row p of `rows` the k best columns q of block blk's primal X = F F^T (0-based like primal_entries; F = (U + V) / 2
        in phase 2, the phase-1 R otherwise), searched on the device without forming X: the largest X_pq first (smallest=True: the
        smallest), ties by ascending q.  cols=(lo, hi): the window [lo, hi) of candidate columns (None: all).  The column p itself is
        no candidate unless include_diag.  skip: columns to leave out, a list of integer arrays, one per query, or a (ptr, col) CSR
        pair; skip_constrained: also every column at which a constraint matrix of the cone stores an entry in row p (on a completion
        problem the observed entries).  1 <= k <= 128.  Returns (idx [nq, k] int32, val [nq, k], found [nq]); the slots past found[i]
        hold idx -1 and val 0.0.  Read-only on the solver's state, deterministic."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        if r.ndim != 1:
            raise ValueError("primal_topk: rows is one vector of query rows")
        nq = len(r)
        n = self.block_shape(blk)[0] if 0 <= int(blk) < self.nblk else 0
        lo, hi = (0, n) if cols is None else (int(cols[0]), int(cols[1]))
        sp = sc = None
        if skip is not None:
            if isinstance(skip, tuple) and len(skip) == 2:
                sp = np.ascontiguousarray(skip[0], dtype=np.int64)
                sc = np.ascontiguousarray(skip[1], dtype=np.int32)
            else:
                if len(skip) != nq:
                    raise ValueError("primal_topk: skip holds one list per query, or is a (ptr, col) pair")
                lists = [np.asarray(x, dtype=np.int32).reshape(-1) for x in skip]
                sp = np.zeros(nq + 1, dtype=np.int64)
                sp[1:] = np.cumsum([len(x) for x in lists])
                sc = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), dtype=np.int32)
            if len(sc) == 0:
                sc = np.zeros(1, dtype=np.int32)
        kk = int(k) if 1 <= int(k) <= 128 else 1
        idx = np.full((max(nq, 1), kk), -1, dtype=np.int32)
        val = np.zeros((max(nq, 1), kk))
        found = np.zeros(max(nq, 1), dtype=np.int32)
        self.lib.lrd_session_primal_topk.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     C.POINTER(C.c_int64), _ip, C.c_int, _ip, _dp, _ip]
        rc = self.lib.lrd_session_primal_topk(self.h, int(blk), nq, r.ctypes.data_as(_ip), lo, hi, int(k), int(bool(smallest)),
                                              int(bool(include_diag)), sp.ctypes.data_as(C.POINTER(C.c_int64)) if sp is not None else None,
                                              sc.ctypes.data_as(_ip) if sc is not None else None, int(bool(skip_constrained)),
                                              idx.ctypes.data_as(_ip), val.ctypes.data_as(_dp), found.ctypes.data_as(_ip))
        # (codes 1 and 2 are the slot's own refusals only where the session layer has let the call through: a solver state, the slot,
        # no sharded deal -- otherwise the library's last message belongs to some earlier call)
        self.lib.lrd_session_solver.restype = C.c_void_p
        self.lib.lrd_session_solver.argtypes = [C.c_void_p]
        reached = self.be is not None and self.be.name == "hip-gfx950" and self.be.has_primal_topk() \
            and bool(self.lib.lrd_session_solver(self.h))
        if rc in (1, 2) and reached:
            lib, _ = self._hip()
            lib.lorads_hip_last_error.restype = C.c_char_p
            msg = (lib.lorads_hip_last_error() or b"").decode()
            if msg.startswith("primal_topk: "):
                raise ValueError(msg)
        if rc == 2:
            raise NotImplementedError("the attached backend (%s) cannot search the rows of the primal: only the HIP backend does"
                                      % (self.be.name if self.be else "none"))
        if rc == 3:
            raise NotImplementedError("the top-k search of a sharded deal (world > 1) is not supported")
        _check(rc, "primal_topk")
        return idx[:nq], val[:nq], found[:nq]

    def primal_diag(self, blk):
        """the diagonal of block blk's primal X"""
        idx = np.arange(self.block_shape(blk)[0], dtype=np.int32)
        return self.primal_entries(blk, idx, idx)[0]

    def dual_infeasibility(self):
        """DIMACS error 2 of the current multipliers, data/lorads_solver.c:1007-1037 (-1: slot missing)"""
        v = C.c_double()
        self.lib.lrd_session_dual_infeasibility(self.h, C.byref(v))
        return v.value

    def close(self):
        if self.h:
            self.lib.lrd_session_close(self.h)
            self.h = None
        if getattr(self, "_shmx", None):
            self.lib.lrd_shmx_close.argtypes = [C.c_void_p]
            self.lib.lrd_shmx_close(self._shmx)
            self._shmx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
