"""Balanced partitions of a bisection-structured solve (Session.round_bisection) and the plain-text bisection file (read_bisection).

A context qualifies when it has no LP block and every cone has the +-1 diagonal rows a_i X[p,p] = b_i with one value t of
sqrt(b_i / a_i), and exactly one sum row a <11^T, X> = b over the whole lower triangle with b / (a t^2) = d^2 for an integer
0 <= d <= n, d = n (mod 2) (Min-/Max-Bisection: d = 0; prescribed part sizes (n +- d) / 2 otherwise).  Then x = t sigma with
sum(sigma) = +-d is feasible; f = sum_k x_k^T C_k x_k.  For instances.bisection (C = L / 4) f is the weight of the cut and bound
bounds the smallest balanced cut from below.  All values in the file's units; DESIGN.md section 19 states the repair and the swap
search.  The file layout is documented in lorads_amd/csrc/host/bisect.c.
"""
import ctypes as C

import numpy as np

from ._rounded import FLOAT_KEYS, INT_KEYS, RoundHeadStruct, _arr, head_of, read_head


class BisectionConeStruct(C.Structure):
    """lrd_bisection_cone (csrc/host/lorads_host.h)"""
    _fields_ = [("n", C.c_int), ("rank", C.c_int), ("diff", C.c_int), ("plus", C.c_int), ("minus", C.c_int),
                ("sigma", C.POINTER(C.c_int8)), ("imbalance", C.POINTER(C.c_int)), ("t", C.c_double), ("lam_min", C.c_double),
                ("G", C.POINTER(C.c_double))]


class BisectionStruct(C.Structure):
    """lrd_bisection (csrc/host/lorads_host.h)"""
    _fields_ = [("head", RoundHeadStruct), ("nblk", C.c_int), ("cone", C.POINTER(BisectionConeStruct))]


class BisectionCone:
    """n, rank, diff (d), plus / minus (the part sizes), sigma (the best trial's signs), t, imbalance (per trial, the sum of the
    hyperplane's signs before the repair), lam_min, G (rank x trials hyperplanes or None)"""

    def __init__(self, n, rank, diff, plus, minus, sigma, t=None, imbalance=None, lam_min=None, G=None):
        self.n, self.rank, self.diff, self.plus, self.minus = n, rank, diff, plus, minus
        self.sigma, self.t, self.imbalance, self.lam_min, self.G = sigma, t, imbalance, lam_min, G


class Bisection:
    """trials, seed, max_rounds, rounds, src, best, best0, f_best, f_best0, obj, obj0 (per trial, after the search / after the
    repair), by, bound, gap, scale, tol and cones[k]"""

    def __init__(self, cones, obj=None, obj0=None, **scalars):
        self.cones, self.obj, self.obj0 = cones, obj, obj0
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
            cones.append(BisectionCone(q.n, q.rank, q.diff, q.plus, q.minus, _arr(q.sigma, q.n, np.int8), q.t,
                                       _arr(q.imbalance, K, np.int32), q.lam_min, G))
        obj, obj0, sc = head_of(st, INT_KEYS + FLOAT_KEYS)
        return cls(cones, obj, obj0, **sc)


def read_bisection(path):
    """Parse a bisection file (Session.write_bisection / lorads --bisectFile) into a Bisection (signs, sizes, objectives, scalars)."""
    lines, pos, sc = read_head(path, "lorads-bisection 1", "bisection", INT_KEYS)
    cones = []
    while pos < len(lines) and lines[pos].startswith("cone "):
        t = lines[pos].split()
        pos += 1
        if len(t) != 7 or int(t[1]) != len(cones) + 1:
            raise ValueError("%s: unexpected line %r" % (path, lines[pos - 1]))
        n, d, plus, minus = int(t[2]), int(t[3]), int(t[4]), int(t[5])
        sig = np.array([int(v) for v in lines[pos:pos + n]], dtype=np.int8)
        if len(sig) != n or not np.all(np.abs(sig) == 1):
            raise ValueError("%s: cone %d holds no n signs" % (path, len(cones) + 1))
        if plus != int(np.sum(sig > 0)) or plus + minus != n:
            raise ValueError("%s: the part sizes of cone %d are not its signs'" % (path, len(cones) + 1))
        pos += n
        cones.append(BisectionCone(n, None, d, plus, minus, sig, float(t[6])))
    t = lines[pos].split() if pos < len(lines) else []
    if len(t) != 2 or t[0] != "objectives" or int(t[1]) != sc["trials"]:
        raise ValueError("%s: expected objectives %d, found %r" % (path, sc["trials"], t))
    pos += 1
    both = np.array([[float(v) for v in ln.split()] for ln in lines[pos:pos + sc["trials"]]]).reshape(-1, 2)
    if both.shape[0] != sc["trials"]:
        raise ValueError("%s: holds no %d objectives" % (path, sc["trials"]))
    return Bisection(cones, both[:, 1].copy(), both[:, 0].copy(), **sc)
