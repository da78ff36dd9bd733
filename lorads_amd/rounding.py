"""Hyperplane rounding of a +-1-structured solve (Session.round_pm1) and the plain-text rounding file (read_rounding).

A context qualifies when it has no LP block and every constraint is a_i X_k[p,p] = b_i with b_i / a_i > 0, one per diagonal
position of every cone (Max-Cut, weighted Max-Cut, +-1 QUBO relaxations and their scaled forms), or is the cut-tightened form of such a problem, whose one LP block holds the slacks of triangle
cuts (Session.write_tightened).  Then x = sigma o t with
t_p = sqrt(b_i / a_i) is feasible for every sigma in {+-1}^n; f = sum_k x_k^T C_k x_k.  For Max-Cut the cut is -f and -bound bounds
the largest cut.  All values in the file's units; DESIGN.md section 11 states the generator and the local search.  The file layout is
documented in lorads_amd/csrc/host/rounding.c.
"""
import ctypes as C

import numpy as np

from ._rounded import FLOAT_KEYS, INT_KEYS, RoundHeadStruct, _arr, head_of, read_head


class RoundingConeStruct(C.Structure):
    """lrd_rounding_cone (csrc/host/lorads_host.h)"""
    _fields_ = [("n", C.c_int), ("rank", C.c_int), ("sigma", C.POINTER(C.c_int8)), ("t", C.POINTER(C.c_double)),
                ("x", C.POINTER(C.c_double)), ("T", C.c_double), ("lam_min", C.c_double), ("G", C.POINTER(C.c_double))]


class RoundingStruct(C.Structure):
    """lrd_rounding (csrc/host/lorads_host.h)"""
    _fields_ = [("head", RoundHeadStruct), ("nblk", C.c_int), ("cone", C.POINTER(RoundingConeStruct)),
                ("nlp", C.c_int), ("lp_neg", C.c_int), ("lp_upper", C.POINTER(C.c_double))]


class RoundingCone:
    """sigma (the best trial's signs), t, x = sigma * t, T = sum t^2, lam_min, G (rank x trials hyperplanes or None)"""

    def __init__(self, n, rank, sigma, t=None, x=None, T=None, lam_min=None, G=None):
        self.n, self.rank = n, rank
        self.sigma, self.t, self.x, self.T, self.lam_min, self.G = sigma, t, x, T, lam_min, G


class Rounding:
    """trials, seed, max_rounds, rounds, src, best, best0, f_best, f_best0, obj, obj0 (per trial, after / before the local
    search), by, bound, gap, scale, tol and cones[k].  On a cut-tightened problem the block of the cuts' slacks is
    an empty cone, and lp_upper (u_j per slack column) and lp_negative (the dual slacks below zero) describe the bound's LP term, as
    the k-cut's do; elsewhere lp_upper is empty."""

    def __init__(self, cones, obj=None, obj0=None, lp_upper=None, lp_negative=0, **scalars):
        self.cones, self.obj, self.obj0 = cones, obj, obj0
        self.lp_upper = np.zeros(0) if lp_upper is None else lp_upper
        self.lp_negative = lp_negative
        for k in INT_KEYS + FLOAT_KEYS:
            setattr(self, k, scalars.get(k))

    @property
    def sign(self):
        """the best trial's signs of all cones, cone after cone"""
        return np.concatenate([c.sigma for c in self.cones]) if self.cones else np.zeros(0, dtype=np.int8)

    @classmethod
    def from_struct(cls, st):
        cones, K = [], st.head.trials
        for k in range(st.nblk):
            q = st.cone[k]
            G = _arr(q.G, q.rank * K).reshape(q.rank, K) if q.G else None
            cones.append(RoundingCone(q.n, q.rank, _arr(q.sigma, q.n, np.int8), _arr(q.t, q.n), _arr(q.x, q.n), q.T, q.lam_min, G))
        obj, obj0, sc = head_of(st, INT_KEYS + FLOAT_KEYS)
        return cls(cones, obj, obj0, _arr(st.lp_upper, st.nlp), st.lp_neg, **sc)


def read_rounding(path):
    """Parse a rounding file (Session.write_rounding / lorads --roundFile) into a Rounding (signs and scalars only)."""
    lines, pos, sc = read_head(path, "lorads-rounding 1", "rounding", INT_KEYS)
    cones = []
    while pos < len(lines) and lines[pos].strip():
        t = lines[pos].split()
        pos += 1
        if t[0] != "cone" or int(t[1]) != len(cones) + 1:
            raise ValueError("%s: unexpected line %r" % (path, lines[pos - 1]))
        n = int(t[2])
        sig = np.array([int(v) for v in lines[pos:pos + n]], dtype=np.int8)
        if len(sig) != n or not np.all(np.abs(sig) == 1):
            raise ValueError("%s: cone %d holds no n signs" % (path, len(cones) + 1))
        pos += n
        cones.append(RoundingCone(n, None, sig))
    return Rounding(cones, **sc)
