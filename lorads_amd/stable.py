"""Stable sets of a theta-structured solve read off its factors (Session.round_stable) and the plain-text file (read_stable).

A problem qualifies when every SDP cone has exactly one trace row a tr(X_k) = b with a > 0 and b > 0 (T_k = b / a), every other
constraint that touches the cone is an edge row X_pq = 0 (one off-diagonal entry, b = 0: the cone's graph), and LP columns occur only
in bound rows 2 a X_pq + c x_j = b -- instances.theta / hamming_theta, block_diag of them, or what Session.write_bounded makes of one.
For a stable set S, X(S) = T 1_S 1_S^T / |S| is feasible and f = <C, X(S)>; for the theta files f = -|S|.  All values in the file's
units; DESIGN.md section 18 states the priorities, the greedy order, the swap search and the dual bound.  The file layout is
documented in lorads_amd/csrc/host/stable.c.
"""
import ctypes as C

import numpy as np

from . import _rounded
from ._rounded import FLOAT_KEYS, RoundHeadStruct, _arr, fill_head, head_of, read_head

INT_KEYS = _rounded.INT_KEYS + ("lp_columns", "lp_negative")


class StableConeStruct(C.Structure):
    """lrd_stable_cone (csrc/host/lorads_host.h)"""
    _fields_ = [("blk", C.c_int), ("n", C.c_int), ("rank", C.c_int), ("size", C.c_int), ("member", C.POINTER(C.c_int)),
                ("sizes", C.POINTER(C.c_int)), ("T", C.c_double), ("lam_min", C.c_double), ("scores", C.POINTER(C.c_double))]


class StableStruct(C.Structure):
    """lrd_stable (csrc/host/lorads_host.h)"""
    _fields_ = [("head", RoundHeadStruct), ("nblk", C.c_int), ("nlp", C.c_int), ("lp_neg", C.c_int), ("lp_upper", C.POINTER(C.c_double)),
                ("cone", C.POINTER(StableConeStruct))]


class StableCone:
    """blk (0-based block of the file), n, rank, member (the best trial's set, 0-based, ascending), trial_sizes (|S| of every trial
    or None), T, lam_min, scores (n x trials priorities in the backend's terms, or None)"""

    def __init__(self, blk, n, rank, member, trial_sizes=None, T=None, lam_min=None, scores=None):
        self.blk, self.n, self.rank, self.member = blk, n, rank, member
        self.trial_sizes, self.T, self.lam_min, self.scores = trial_sizes, T, lam_min, scores


class StableSet:
    """trials, seed, max_rounds, rounds, src, best, best0, f_best, f_best0, obj, obj0 (per trial, after the search / of the greedy
    sets), lp_columns, lp_negative, lp_upper (u_j per LP column), by, bound, gap, scale, tol and cones[k] (the SDP cones);
    members[k], sizes[k] and scores[k] are the cones' sets, their sizes and (when asked for) their priorities"""

    def __init__(self, cones, obj=None, obj0=None, lp_upper=None, **scalars):
        self.cones, self.obj, self.obj0, self.lp_upper = cones, obj, obj0, lp_upper
        for k in INT_KEYS + FLOAT_KEYS:
            setattr(self, k, scalars.get(k))

    @property
    def members(self):
        return [c.member for c in self.cones]

    @property
    def sizes(self):
        return [len(c.member) for c in self.cones]

    @property
    def scores(self):
        return [c.scores for c in self.cones]

    @classmethod
    def from_struct(cls, st):
        cones, K = [], st.head.trials
        for k in range(st.nblk):
            q = st.cone[k]
            sc = _arr(q.scores, K * q.n).reshape(K, q.n).T.copy() if q.scores else None
            cones.append(StableCone(q.blk, q.n, q.rank, _arr(q.member, q.size, np.int64), _arr(q.sizes, K, np.int64), q.T,
                                    q.lam_min, sc))
        obj, obj0, sc = head_of(st, INT_KEYS + FLOAT_KEYS)
        return cls(cones, obj, obj0, _arr(st.lp_upper, st.nlp), **sc)

    def to_struct(self):
        """an lrd_stable that holds what the file holds (for lrd_stable_write); keeps its arrays alive on the struct"""
        st = StableStruct()
        fill_head(st, self, INT_KEYS + FLOAT_KEYS)
        st.nblk = len(self.cones)
        arr = (StableConeStruct * max(1, st.nblk))()
        keep = [arr]
        for k, c in enumerate(self.cones):
            mem = np.ascontiguousarray(c.member, dtype=np.int32)
            keep.append(mem)
            arr[k].blk, arr[k].n, arr[k].rank, arr[k].size = c.blk, c.n, c.rank or 0, len(mem)
            arr[k].member = mem.ctypes.data_as(C.POINTER(C.c_int))
        st.cone = C.cast(arr, C.POINTER(StableConeStruct))
        st._keep = keep
        return st


def read_stable(path):
    """Parse a stable-set file (Session.write_stable / lorads --stableFile) into a StableSet (members and scalars only)."""
    lines, pos, sc = read_head(path, "lorads-stableset 1", "stable-set", INT_KEYS)
    cones = []
    while pos < len(lines) and lines[pos].strip():
        t = lines[pos].split()
        pos += 1
        if len(t) != 4 or t[0] != "cone":
            raise ValueError("%s: unexpected line %r" % (path, lines[pos - 1]))
        blk, n, size = int(t[1]) - 1, int(t[2]), int(t[3])
        mem = np.array([int(v) - 1 for v in lines[pos:pos + size]], dtype=np.int64)
        if len(mem) != size or np.any(mem < 0) or np.any(mem >= n) or np.any(np.diff(mem) <= 0):
            raise ValueError("%s: cone %d holds no %d ascending members below %d" % (path, blk + 1, size, n))
        pos += size
        cones.append(StableCone(blk, n, None, mem))
    return StableSet(cones, **sc)
