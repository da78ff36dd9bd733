"""Entry bounds on the primal X: the small pure-Python side.

Every pair p < q of an SDP cone has two inequalities: class 0, X_pq >= lower with v = lower - X_pq, and class 1, X_pq <= upper with
v = X_pq - upper; v > min_violation is a violation.  The enumeration is the device's (Session.entry_bounds); here: the struct
mirror, the result object and a reader of the list out of a bounded problem file (Session.write_bounded)."""
import ctypes as C

import numpy as np

from .cuts import read_sdpa


class BoundsStruct(C.Structure):
    """lrd_bounds (csrc/host/lorads_host.h)"""
    _fields_ = [("nblk", C.c_int), ("src", C.c_int), ("lower", C.c_double), ("upper", C.c_double), ("min_violation", C.c_double),
                ("max_cuts", C.c_int), ("count", C.POINTER(C.c_int64)), ("kept", C.c_int), ("passes", C.c_int),
                ("cone", C.POINTER(C.c_int)), ("p", C.POINTER(C.c_int)), ("q", C.POINTER(C.c_int)),
                ("cls", C.POINTER(C.c_int8)), ("viol", C.POINTER(C.c_double)), ("bound", C.POINTER(C.c_double))]


class Bounds:
    """count[k]: violated (pair, class) of cone k; cone, p, q, cls, violation, bound: the kept ones, 0-based, ordered by (violation
    descending, cone, p, q, cls ascending), each with the bound it violates; passes: enumeration passes of all cones"""

    def __init__(self, count, cone, p, q, cls, violation, bound, passes=0, src=0, lower=0.0, upper=np.inf, min_violation=0.0,
                 max_cuts=0):
        self.count = np.asarray(count, dtype=np.int64)
        self.cone = np.ascontiguousarray(cone, dtype=np.int32)
        self.p = np.ascontiguousarray(p, dtype=np.int32)
        self.q = np.ascontiguousarray(q, dtype=np.int32)
        self.cls = np.ascontiguousarray(cls, dtype=np.int8)
        self.violation = np.ascontiguousarray(violation, dtype=np.float64)
        self.bound = np.ascontiguousarray(bound, dtype=np.float64)
        self.passes, self.src, self.max_cuts = int(passes), int(src), int(max_cuts)
        self.lower, self.upper, self.min_violation = float(lower), float(upper), float(min_violation)

    def __len__(self):
        return len(self.p)

    def __add__(self, other):
        """the two lists one after the other (rounds of a cutting-plane loop; each cut keeps its own bound)"""
        cat = lambda a: np.concatenate([getattr(self, a), getattr(other, a)])  # noqa: E731
        return Bounds(self.count + other.count, cat("cone"), cat("p"), cat("q"), cat("cls"), cat("violation"), cat("bound"),
                      self.passes + other.passes, other.src, other.lower, other.upper, other.min_violation,
                      self.max_cuts + other.max_cuts)

    @classmethod
    def from_struct(cls, st):
        k = st.kept
        arr = lambda ptr, t: np.array(ptr[:k], dtype=t)  # noqa: E731
        return cls(np.array(st.count[:st.nblk], dtype=np.int64), arr(st.cone, np.int32), arr(st.p, np.int32), arr(st.q, np.int32),
                   arr(st.cls, np.int8), arr(st.viol, np.float64), arr(st.bound, np.float64), st.passes, st.src, st.lower, st.upper,
                   st.min_violation, st.max_cuts)

    def to_struct(self):
        """an lrd_bounds over this object's arrays (which must outlive it)"""
        st = BoundsStruct()
        st.nblk, st.src, st.max_cuts = len(self.count), self.src, self.max_cuts
        st.lower, st.upper, st.min_violation = self.lower, self.upper, self.min_violation
        st.count = self.count.ctypes.data_as(C.POINTER(C.c_int64))
        st.kept, st.passes = len(self), self.passes
        ip = C.POINTER(C.c_int)
        st.cone, st.p, st.q = (a.ctypes.data_as(ip) for a in (self.cone, self.p, self.q))
        st.cls = self.cls.ctypes.data_as(C.POINTER(C.c_int8))
        st.viol = self.violation.ctypes.data_as(C.POINTER(C.c_double))
        st.bound = self.bound.ctypes.data_as(C.POINTER(C.c_double))
        return st


def read_bounded(path, m_original):
    """the list of bound cuts of a bounded problem file: [(cone, p, q, cls, bound)] 0-based in the file's order, one per constraint
    beyond m_original.  A cut holds 0.5 at (p, q) of its cone and -1 (class 0) or +1 (class 1) on the diagonal of an LP block, in a
    column no other constraint uses; its right-hand side is the bound."""
    m, blocks, b, ent = read_sdpa(path)
    per, cols = {}, {}
    for mat, blk, i, j, v in ent:
        if mat > m_original:
            per.setdefault(mat, []).append((blk, i, j, v))
        if blocks[blk - 1] < 0 and mat > 0:
            cols[(blk, i)] = cols.get((blk, i), 0) + 1
    out = []
    for e in range(m_original + 1, m + 1):
        rows = sorted(per.get(e, ()), key=lambda t: blocks[t[0] - 1] < 0)
        ok = len(rows) == 2 and blocks[rows[0][0] - 1] > 0 and blocks[rows[1][0] - 1] < 0
        if ok:
            (k, p, q, a), (lb, i, j, sv) = rows
            ok = a == 0.5 and p < q and i == j and sv in (-1.0, 1.0) and cols[(lb, i)] == 1
        if not ok:
            raise ValueError("constraint %d is not a bound cut" % e)
        out.append((k - 1, p - 1, q - 1, 0 if sv < 0 else 1, float(b[e - 1])))
    return out
