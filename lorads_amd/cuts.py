"""Triangle inequalities of +-1-structured problems: the small pure-Python side.

With rho_xy = X_xy / (t_x t_y) every triple p < q < s of a cone has four inequalities, class c = 0..3:

    SIGNS[c] . (rho_pq, rho_ps, rho_qs) >= -1

and v = -1 - lhs > 0 is a violation.  The enumeration is the device's (Session.triangle_cuts); here: the struct mirror, the
result object and a reader of the cut list out of a tightened problem file (Session.write_tightened)."""
import collections
import ctypes as C
import os

import numpy as np

# coefficients of rho_pq, rho_ps, rho_qs per class
SIGNS = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.int8)


class CutsStruct(C.Structure):
    """lrd_cuts (csrc/host/lorads_host.h)"""
    _fields_ = [("nblk", C.c_int), ("src", C.c_int), ("min_violation", C.c_double), ("max_cuts", C.c_int),
                ("count", C.POINTER(C.c_int64)), ("kept", C.c_int), ("passes", C.c_int),
                ("cone", C.POINTER(C.c_int)), ("p", C.POINTER(C.c_int)), ("q", C.POINTER(C.c_int)), ("s", C.POINTER(C.c_int)),
                ("cls", C.POINTER(C.c_int8)), ("viol", C.POINTER(C.c_double))]


class PresentStruct(C.Structure):
    """lrd_present (csrc/host/lorads_host.h)"""
    _fields_ = [("n", C.c_int), ("lpk", C.c_int)] + [(f, C.POINTER(C.c_int)) for f in ("cone", "p", "q", "s", "cls", "row", "col")] + \
               [("scale", C.POINTER(C.c_double)), ("t", C.POINTER(C.c_double))]


class PresentCut(collections.namedtuple("PresentCut", "cone p q s cls row column scale")):
    """A triangle cut that a cut-tightened problem holds as a row (Session.present_cuts): its triple and class, its constraint and its
    LP column (all 0-based), and scale = -b / c of the row (1 as written).  Compares as the tuple (cone, p, q, s, cls, row, column)."""
    __slots__ = ()

    def __eq__(self, other):
        return tuple(self[:7]) == tuple(other[:7])

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(tuple(self[:7]))


class Cuts:
    """count[k]: violated (triple, class) pairs of cone k; cone, p, q, s, cls, violation: the kept ones, 0-based, ordered by
    (violation descending, cone, p, q, s, cls ascending); passes: enumeration passes of all cones"""

    def __init__(self, count, cone, p, q, s, cls, violation, passes=0, src=0, min_violation=0.0, max_cuts=0):
        self.count = np.asarray(count, dtype=np.int64)
        self.cone = np.ascontiguousarray(cone, dtype=np.int32)
        self.p = np.ascontiguousarray(p, dtype=np.int32)
        self.q = np.ascontiguousarray(q, dtype=np.int32)
        self.s = np.ascontiguousarray(s, dtype=np.int32)
        self.cls = np.ascontiguousarray(cls, dtype=np.int8)
        self.violation = np.ascontiguousarray(violation, dtype=np.float64)
        self.passes, self.src, self.min_violation, self.max_cuts = int(passes), int(src), float(min_violation), int(max_cuts)

    def __len__(self):
        return len(self.p)

    @classmethod
    def from_struct(cls, st):
        k = st.kept
        arr = lambda ptr, t: np.array(ptr[:k], dtype=t)  # noqa: E731
        return cls(np.array(st.count[:st.nblk], dtype=np.int64), arr(st.cone, np.int32), arr(st.p, np.int32), arr(st.q, np.int32),
                   arr(st.s, np.int32), arr(st.cls, np.int8), arr(st.viol, np.float64), st.passes, st.src, st.min_violation,
                   st.max_cuts)

    def to_struct(self):
        """an lrd_cuts over this object's arrays (which must outlive it)"""
        st = CutsStruct()
        st.nblk, st.src, st.min_violation, st.max_cuts = len(self.count), self.src, self.min_violation, self.max_cuts
        st.count = self.count.ctypes.data_as(C.POINTER(C.c_int64))
        st.kept, st.passes = len(self), self.passes
        ip = C.POINTER(C.c_int)
        st.cone, st.p, st.q, st.s = (a.ctypes.data_as(ip) for a in (self.cone, self.p, self.q, self.s))
        st.cls = self.cls.ctypes.data_as(C.POINTER(C.c_int8))
        st.viol = self.violation.ctypes.data_as(C.POINTER(C.c_double))
        return st


def read_sdpa(path):
    """(m, blocks, b, entries) of an SDPA sparse file as this project writes them: entries = [(mat, blk, i, j, value)], 1-based"""
    with open(path) as f:
        lines = [ln for ln in f if ln.strip() and ln[0] not in '*"']
    m, nblk = int(lines[0].split()[0]), int(lines[1].split()[0])
    blocks = [int(x) for x in lines[2].replace(",", " ").split()[:nblk]]
    b = np.array([float(x) for x in lines[3].replace(",", " ").split()[:m]])
    ent = []
    for ln in lines[4:]:
        w = ln.split()
        ent.append((int(w[0]), int(w[1]), int(w[2]), int(w[3]), float(w[4])))
    return m, blocks, b, ent


def read_tightened(path, m_original):
    """the cut list of a tightened problem file: [(cone, p, q, s, cls)] 0-based in the file's order, one per constraint beyond
    m_original.  A cut's three entries sit at (p, q), (p, s), (q, s) of its cone and their signs name its class."""
    m, blocks, b, ent = read_sdpa(path)
    if m == m_original:
        return []
    lp = len(blocks)
    if blocks[-1] != -(m - m_original):
        raise ValueError("the last block is not the LP block of the cuts' slacks")
    per = {}
    for mat, blk, i, j, v in ent:
        if mat > m_original and blk != lp:
            per.setdefault(mat, []).append((blk, i, j, v))
    out = []
    for e in range(m_original + 1, m + 1):
        if b[e - 1] != -1.0 or len(per.get(e, ())) != 3:
            raise ValueError("constraint %d is not a triangle cut" % e)
        rows = sorted(per[e], key=lambda t: (t[1], t[2]))
        (k, p, q, a), (_, p2, s, c), (_, q2, s2, d) = rows
        if not (p == p2 and q == q2 and s == s2 and p < q < s and len({r[0] for r in rows}) == 1):
            raise ValueError("constraint %d is not a triangle cut" % e)
        sg = (np.sign([a, c, d])).astype(np.int8)
        cl = [i for i in range(4) if (SIGNS[i] == sg).all()]
        if len(cl) != 1:
            raise ValueError("constraint %d has the signs of no class" % e)
        out.append((k - 1, p - 1, q - 1, s - 1, cl[0]))
    return out


CutRound = collections.namedtuple("CutRound", "path pObj d f_best gap present added dropped count")


def cut_loop(path, workdir, rounds, max_cuts=1000, min_violation=1e-3, drop_slack=None, trials=1024, seed=0, local_search_rounds=100,
             tol=1e-8, **solve_options):
    """Rounds of solve, round, separate and tighten on a +-1-structured problem file.  Round i opens its file
    (round 0: `path`), solves it (solve_options: Session.set_params), rounds the point (Session.round_pm1), separates the triangle
    inequalities that are not rows yet (Session.triangle_cuts) and writes the next file, workdir/round<i + 1>.dat-s
    (Session.write_tightened with drop_slack), one context at a time.  It stops after `rounds` rounds, or as soon as nothing is
    violated.  Returns (history, f_best, sign): per round a CutRound (the file it solved, pObj, the dual bound d, the round's own
    f_best and gap, the cuts the file held, the cuts added to and dropped from the next, the violated count), and the best +-1 point
    of all rounds.  Every round's d bounds every round's f: the cuts hold at every +-1 point."""
    from .host import Session
    os.makedirs(workdir, exist_ok=True)
    history, best_f, best_sign = [], np.inf, None
    for i in range(int(rounds)):
        s = Session.open(path)
        try:
            s.set_params(**dict(dict(verbose=0), **solve_options))
            s.prepare(1, 0)
            s.attach_hip(lbfgs_len=int(solve_options.get("lbfgsListLength", 2)))
            res = s.solve()
            present = len(s.present_cuts())
            r = s.round_pm1(trials=trials, seed=seed, local_search_rounds=local_search_rounds, tol=tol)
            if r.f_best < best_f:
                best_f, best_sign = r.f_best, r.sign.copy()
            cuts = s.triangle_cuts(max_cuts=max_cuts, min_violation=min_violation)
            count, added, dropped, nxt = int(cuts.count.sum()), 0, 0, None
            if count > 0 and i + 1 < int(rounds):
                nxt = os.path.join(workdir, "round%d.dat-s" % (i + 1))
                dropped = s.write_tightened(nxt, cuts, drop_slack=drop_slack if present else None)
                added = len(cuts)
            history.append(CutRound(path, res["pObj"], r.bound, r.f_best, r.gap, present, added, dropped, count))
        finally:
            s.close()
        if nxt is None:
            break
        path = nxt
    return history, best_f, best_sign
