"""Exported primal-dual point of a solve (Session.solution) and the plain-text solution file (read_solution).

Problem: min <C, X> s.t. <A_i, X> = b_i, X psd, with C = -F0 and A_i = F_i of the SDPA file (SDPA's own names: Y_sdpa = X,
x_sdpa = -y, X_sdpa = S).  X_k = R_k R_k^T per SDP cone, x_j = r_j^2 on the LP block, S_k = C_k - sum_i y_i A_ik; all values in
the file's units.  The file layout is documented in lorads_amd/csrc/host/solution.c.
"""
import ctypes as C

import numpy as np

CERT_KEYS = ("err1", "err1_inf", "err2", "err3", "err4", "err5", "err6")


class SolutionConeStruct(C.Structure):
    """lrd_solution_cone (csrc/host/lorads_host.h)"""
    _fields_ = [("n", C.c_int), ("rank", C.c_int), ("is_lp", C.c_int),
                ("R", C.POINTER(C.c_double)), ("U", C.POINTER(C.c_double)), ("V", C.POINTER(C.c_double)),
                ("x", C.POINTER(C.c_double)), ("s_nnz", C.c_int64), ("s_row", C.POINTER(C.c_int)),
                ("s_col", C.POINTER(C.c_int)), ("s_val", C.POINTER(C.c_double)), ("lam_min", C.c_double)]


class SolutionStruct(C.Structure):
    """lrd_solution (csrc/host/lorads_host.h)"""
    _fields_ = [("m", C.c_int), ("nblk", C.c_int), ("status", C.c_int), ("src", C.c_int),
                ("scale", C.c_double), ("pobj", C.c_double), ("dobj", C.c_double)] + \
               [(k, C.c_double) for k in CERT_KEYS] + \
               [("xs", C.c_double), ("matvecs", C.c_int), ("y", C.POINTER(C.c_double)),
                ("cone", C.POINTER(SolutionConeStruct))]


def _arr(ptr, n, dtype=np.float64):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n > 0 else np.zeros(0, dtype=dtype)


class Cone:
    """One block: R, U, V (n x rank) of an SDP cone, or x (n) of the LP block"""

    def __init__(self, n, rank, is_lp, R=None, U=None, V=None, x=None, slack=None, lam_min=None):
        self.n, self.rank, self.is_lp = n, rank, bool(is_lp)
        self.R, self.U, self.V, self.x = R, U, V, x
        self._slack = slack
        self.lam_min = lam_min


class Solution:
    """status, pobj, dobj, y, cones[k], certificate (dict), slack(k) -> (row, col, val) lower-triangle triplets"""

    def __init__(self, status, pobj, dobj, y, cones, certificate):
        self.status, self.pobj, self.dobj = status, pobj, dobj
        self.y = y
        self.cones = cones
        self.certificate = certificate

    def slack(self, k):
        """S_k = C_k - sum_i y_i A_ik as (row, col, val) with row >= col (LP block: one (j, j) entry per column)"""
        s = self.cones[k]._slack
        if s is None:
            raise ValueError("a solution read from a file holds no slack: it follows from the problem and y")
        return s

    @classmethod
    def from_struct(cls, st):
        cones = []
        for k in range(st.nblk):
            q = st.cone[k]
            n, r = q.n, q.rank
            mats = [_arr(getattr(q, f), n * r).reshape(r, n).T.copy() for f in ("R", "U", "V")]
            nz = int(q.s_nnz)
            slack = (_arr(q.s_row, nz, np.int32), _arr(q.s_col, nz, np.int32), _arr(q.s_val, nz))
            x = _arr(q.x, n) if q.is_lp else None
            cones.append(Cone(n, r, q.is_lp, *mats, x=x, slack=slack, lam_min=q.lam_min))
        cert = {k: getattr(st, k) for k in CERT_KEYS}
        cert.update(pobj=st.pobj, dobj=st.dobj, xs=st.xs, lam_min=[c.lam_min for c in cones], matvecs=st.matvecs,
                    scale_obj_his=st.scale, source="(U+V)/2" if st.src == 1 else "R")
        return cls(st.status, st.pobj, st.dobj, _arr(st.y, st.m), cones, cert)


def read_solution(path):
    """Parse a solution file (Session.write_solution / lorads --solutionFile) into a Solution (no slack, no U, V)."""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines[0] != "lorads-solution 1":
        raise ValueError("%s: not a lorads solution file" % path)
    pos = 1

    def take():
        nonlocal pos
        pos += 1
        return lines[pos - 1].split()

    head = {}
    for key in ("status", "pobj", "dobj") + CERT_KEYS:
        t = take()
        if t[0] != key:
            raise ValueError("%s: expected %s, found %r" % (path, key, t))
        head[key] = int(t[1]) if key == "status" else float(t[1])
    t = take()
    if t[0] != "y":
        raise ValueError("%s: expected y" % path)
    m = int(t[1])
    y = np.array([float(take()[0]) for _ in range(m)], dtype=np.float64)
    cones = []
    while pos < len(lines) and lines[pos].strip():
        t = take()
        if t[0] == "sdp":
            n, r = int(t[2]), int(t[3])
            R = np.array([[float(v) for v in take()] for _ in range(n)], dtype=np.float64).reshape(n, r)
            cones.append(Cone(n, r, False, R=R))
        elif t[0] == "lp":
            n = int(t[2])
            cones.append(Cone(n, 1, True, x=np.array([float(take()[0]) for _ in range(n)], dtype=np.float64)))
        else:
            raise ValueError("%s: unexpected line %r" % (path, lines[pos - 1]))
    cert = {k: head[k] for k in CERT_KEYS}
    cert.update(pobj=head["pobj"], dobj=head["dobj"])
    return Solution(head["status"], head["pobj"], head["dobj"], y, cones, cert)
