"""Frieze-Jerrum rounding of a k-cut-structured solve into k parts (Session.round_kcut) and the plain-text file (read_kcut).

A context qualifies when every constraint without an LP entry is a_i X_k[p,p] = b_i with b_i / a_i > 0, one per diagonal position of
every cone (t_p = sqrt(b_i / a_i)), and every constraint with an LP entry is a bound row 2 a X_pq + c x_j = b with one off-diagonal
cone entry and one LP column that occurs nowhere else and has no objective -- a Max-Cut-type problem, or what Session.write_bounded
makes of one.  For labels l_p in {0 .. k-1}, X(l)_pq = t_p t_q where l_p = l_q and -t_p t_q / (k - 1) elsewhere; f = sum <C, X(l)>.
For C = -L/4 (instances.maxcut) the weight of the k-cut is -2 f (k - 1) / k.  All values in the file's units; DESIGN.md section 16
states the generator, the local search and the dual bound.  The file layout is documented in lorads_amd/csrc/host/kcut.c.
"""
import ctypes as C

import numpy as np

from . import _rounded
from ._rounded import FLOAT_KEYS, RoundHeadStruct, _arr, fill_head, head_of, read_head

INT_KEYS = ("parts",) + _rounded.INT_KEYS + ("lp_columns", "lp_negative")


class KCutConeStruct(C.Structure):
    """lrd_kcut_cone (csrc/host/lorads_host.h)"""
    _fields_ = [("blk", C.c_int), ("n", C.c_int), ("rank", C.c_int), ("label", C.POINTER(C.c_uint8)), ("t", C.POINTER(C.c_double)),
                ("size", C.POINTER(C.c_int)), ("T", C.c_double), ("lam_min", C.c_double), ("G", C.POINTER(C.c_double))]


class KCutStruct(C.Structure):
    """lrd_kcut (csrc/host/lorads_host.h)"""
    _fields_ = [("head", RoundHeadStruct), ("nblk", C.c_int), ("parts", C.c_int), ("nlp", C.c_int), ("lp_neg", C.c_int),
                ("lp_upper", C.POINTER(C.c_double)), ("cone", C.POINTER(KCutConeStruct))]


class KCutCone:
    """blk (0-based block of the file), n, rank, label (the best trial's labels), sizes (vertices per part), t, T = sum t^2, lam_min,
    G (parts x rank x trials vectors or None)"""

    def __init__(self, blk, n, rank, label, sizes, t=None, T=None, lam_min=None, G=None):
        self.blk, self.n, self.rank = blk, n, rank
        self.label, self.sizes, self.t, self.T, self.lam_min, self.G = label, sizes, t, T, lam_min, G


class KCut:
    """parts, trials, seed, max_rounds, rounds, src, best, best0, f_best, f_best0, obj, obj0 (per trial, after / before the local
    search), lp_columns, lp_negative, lp_upper (u_j per LP column), by, bound, gap, scale, tol and cones[k] (the SDP cones)"""

    def __init__(self, cones, obj=None, obj0=None, lp_upper=None, **scalars):
        self.cones, self.obj, self.obj0, self.lp_upper = cones, obj, obj0, lp_upper
        for k in INT_KEYS + FLOAT_KEYS:
            setattr(self, k, scalars.get(k))

    @property
    def label(self):
        """the best trial's labels of all SDP cones, cone after cone"""
        return np.concatenate([c.label for c in self.cones]) if self.cones else np.zeros(0, dtype=np.uint8)

    @classmethod
    def from_struct(cls, st):
        cones, K = [], st.head.trials
        for k in range(st.nblk):
            q = st.cone[k]
            G = _arr(q.G, st.parts * q.rank * K).reshape(st.parts, q.rank, K) if q.G else None
            cones.append(KCutCone(q.blk, q.n, q.rank, _arr(q.label, q.n, np.uint8), _arr(q.size, st.parts, np.int64), _arr(q.t, q.n),
                                  q.T, q.lam_min, G))
        obj, obj0, sc = head_of(st, INT_KEYS + FLOAT_KEYS)
        return cls(cones, obj, obj0, _arr(st.lp_upper, st.nlp), **sc)

    def to_struct(self):
        """an lrd_kcut that holds what the file holds (for lrd_kcut_write); keeps its arrays alive on the struct"""
        st = KCutStruct()
        fill_head(st, self, INT_KEYS + FLOAT_KEYS)
        st.nblk = len(self.cones)
        arr = (KCutConeStruct * max(1, st.nblk))()
        keep = [arr]
        for k, c in enumerate(self.cones):
            lab = np.ascontiguousarray(c.label, dtype=np.uint8)
            siz = np.ascontiguousarray(c.sizes, dtype=np.int32)
            keep += [lab, siz]
            arr[k].blk, arr[k].n, arr[k].rank = c.blk, c.n, c.rank or 0
            arr[k].label = lab.ctypes.data_as(C.POINTER(C.c_uint8))
            arr[k].size = siz.ctypes.data_as(C.POINTER(C.c_int))
        st.cone = C.cast(arr, C.POINTER(KCutConeStruct))
        st._keep = keep
        return st


def read_kcut(path):
    """Parse a k-cut file (Session.write_kcut / lorads --kcutFile) into a KCut (labels, part sizes and scalars only)."""
    lines, pos, sc = read_head(path, "lorads-kcut 1", "k-cut", INT_KEYS)
    cones = []
    while pos < len(lines) and lines[pos].strip():
        t = lines[pos].split()
        pos += 1
        if len(t) != 3 or t[0] != "cone":
            raise ValueError("%s: unexpected line %r" % (path, lines[pos - 1]))
        blk, n = int(t[1]) - 1, int(t[2])
        t = lines[pos].split()
        pos += 1
        if not t or t[0] != "sizes" or len(t) != sc["parts"] + 1:
            raise ValueError("%s: cone %d has no line of %d sizes" % (path, blk + 1, sc["parts"]))
        sizes = np.array([int(v) for v in t[1:]], dtype=np.int64)
        lab = np.array([int(v) for v in lines[pos:pos + n]], dtype=np.int64)
        if len(lab) != n or np.any(lab < 0) or np.any(lab >= sc["parts"]) or not np.array_equal(np.bincount(lab, minlength=sc["parts"]), sizes):
            raise ValueError("%s: cone %d holds no n labels that match its sizes" % (path, blk + 1))
        pos += n
        cones.append(KCutCone(blk, n, None, lab.astype(np.uint8), sizes))
    return KCut(cones, **sc)
