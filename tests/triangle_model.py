"""numpy model of the triangle-inequality separation: what lorads_hip_triangle_cuts must return.

Per cone: F (n x r, the factor at the cone's own rank), t (n), rho_xy = (F_x . F_y) / (t_x t_y).  For p < q < s and class c the
violation is v = -1 - SIGNS[c] . (rho_pq, rho_ps, rho_qs).  The total order is (v descending, [cone,] p, q, s, c ascending).

The error bound of one v (derived, not measured): a dot product of r terms in any summation order errs by at most
gamma_r sum |.| <= r 2^-53 |F_x| |F_y| to first order; the square roots, the divisions and the three additions add a few units.  So

    eps(p, q, s) = (r + 6) 2^-53 (n_pq + n_ps + n_qs + 1),   n_xy = |F_x| |F_y| / (t_x t_y)

bounds |v_computed - v_exact| for the device and for the float64 enumeration below alike.  The longdouble evaluation (64-bit
mantissa: its own error is 2^-11 of that) stands for the exact value.

  enumerate_all   every (p, q, s, c, v), by p over the (q, s) upper triangle, in float64 or longdouble (small n)
  Scan            one float64 pass that streams the same enumeration and keeps only what can matter -- pairs within a margin of
                  min_violation, and the running top K -- re-evaluated in longdouble: exact counts at min_violation -+ eps and the
                  exact top of the list at sizes where nothing can be stored
  tightened       the tightened problem as a generator dict (lorads_amd.instances.write_sdpa writes it)
  plant_rows      planted integer factors whose counts have closed forms (plant_counts) and whose kept list is known in advance
                  (first_distinct_triples), at sizes where nothing can be enumerated on the host
"""
from math import comb

import numpy as np

from lorads_amd.cuts import SIGNS

U53 = 2.0 ** -53


def t_of(prob):
    """per cone t_p = sqrt(b_i / a_i) of the constraint a_i X[p,p] = b_i of a generator dict (0 where there is none)"""
    t = [np.zeros(abs(n)) for n in prob["blocks"]]
    b = np.asarray(prob["b"], dtype=np.float64)
    for mat, blk, i, j, v in prob["entries"]:
        if mat > 0 and i == j:
            t[blk - 1][i - 1] = np.sqrt(b[mat - 1] / np.float64(v))
    return t


def rho_matrix(F, t, dtype=np.float64):
    F = np.asarray(F, dtype=dtype)
    t = np.asarray(t, dtype=dtype)
    return (F @ F.T) / np.outer(t, t)


def class_values(a, b, c):
    """the four violations of rho_pq = a, rho_ps = b, rho_qs = c, stacked on a new first axis"""
    return np.stack([-1 - (a + b + c), -1 - (a - b - c), -1 - (-a + b - c), -1 - (-a - b + c)])


def enumerate_all(F, t, dtype=np.float64):
    """(p, q, s, c, v) of all 4 C(n, 3) pairs, by p over the (q, s) upper triangle"""
    rho = rho_matrix(F, t, dtype)
    n = rho.shape[0]
    P, Q, S, Cl, V = [], [], [], [], []
    for p in range(n - 2):
        q, s = np.triu_indices(n - p - 1, 1)
        q, s = q + p + 1, s + p + 1
        v = class_values(rho[p, q], rho[p, s], rho[q, s])
        for c in range(4):
            P.append(np.full(len(q), p)); Q.append(q); S.append(s); Cl.append(np.full(len(q), c)); V.append(v[c])
    if not P:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, np.zeros(0, dtype=dtype)
    return tuple(np.concatenate(x) for x in (P, Q, S, Cl, V))


def order(v, p, q, s, c, cone=None):
    """the permutation into the total order (v descending, cone, p, q, s, c ascending)"""
    keys = [c, s, q, p] + ([cone] if cone is not None else []) + [-np.asarray(v)]
    return np.lexsort(tuple(keys))


def row_norms(F, t):
    return np.sqrt((np.asarray(F, dtype=np.float64) ** 2).sum(1)) / np.asarray(t, dtype=np.float64)


def eps_of(F, t, p, q, s):
    """the per-pair error bound (see the module's text)"""
    nr = row_norms(F, t)
    r = np.asarray(F).shape[1]
    return (r + 6) * U53 * (nr[p] * nr[q] + nr[p] * nr[s] + nr[q] * nr[s] + 1.0)


def exact_values(F, t, p, q, s, c):
    """v of the given pairs in longdouble"""
    F = np.asarray(F, dtype=np.longdouble)
    t = np.asarray(t, dtype=np.longdouble)
    p, q, s, c = (np.asarray(x, dtype=np.int64) for x in (p, q, s, c))
    if len(p) == 0:
        return np.zeros(0, dtype=np.longdouble)
    r = lambda x, y: (F[x] * F[y]).sum(1) / (t[x] * t[y])  # noqa: E731
    v = class_values(r(p, q), r(p, s), r(q, s))
    return v[c, np.arange(len(p))]


class Scan:
    """One streamed float64 enumeration of a cone at (min_violation, K):
      count_hi, count_lo   the number of pairs with exact v > min_violation + eps / > min_violation - eps (eps per pair)
      p, q, s, c, v        the exact list: every pair with exact v > min_violation that can be among the first K, in the total order
                           (v longdouble), complete down to rank K
    A pair whose float64 v is further than `margin` = 4 max eps from a threshold is decided by float64 (both values err by at most
    eps); the others are evaluated in longdouble."""

    def __init__(self, F, t, min_violation, K):
        F = np.asarray(F, dtype=np.float64)
        t = np.asarray(t, dtype=np.float64)
        n, r = F.shape
        nr = row_norms(F, t)
        nmax = float(nr.max()) if n else 0.0
        margin = 4 * (r + 6) * U53 * (3 * nmax * nmax + 1.0)
        rho = rho_matrix(F, t)
        lo_count = min_violation - margin
        sure = 0
        amb = [np.zeros((0, 4), dtype=np.int64)]
        top_idx = [np.zeros((0, 4), dtype=np.int64)]
        top_v = [np.zeros(0)]
        kth = -np.inf
        held = 0
        for p in range(n - 2):
            a = rho[p, p + 1:]
            sub = rho[p + 1:, p + 1:]
            sm = a[None, :] + sub           # rho_ps + rho_qs at [q, s]
            df = a[None, :] - sub           # rho_ps - rho_qs
            am, ap = (-1 - a)[:, None], (-1 + a)[:, None]
            best = np.maximum(am + np.abs(sm), ap + np.abs(df))
            cand = np.triu(best > lo_count, 1)
            qi, si = np.nonzero(cand)
            if len(qi) == 0:
                continue
            v = class_values(a[qi], a[si], sub[qi, si])
            ci, ei = np.nonzero(v > lo_count)
            vv = v[ci, ei]
            idx = np.stack([np.full(len(ei), p), qi[ei] + p + 1, si[ei] + p + 1, ci], 1)
            sure += int(np.count_nonzero(vv > min_violation + margin))
            near = vv <= min_violation + margin
            if near.any():
                amb.append(idx[near])
            if K > 0:
                keep = vv > max(lo_count, kth - margin)
                top_idx.append(idx[keep]); top_v.append(vv[keep])
                held += int(keep.sum())
                if held > 4 * K + 65536:   # prune what has fallen below the running K-th value
                    ti, tv = np.concatenate(top_idx), np.concatenate(top_v)
                    if len(tv) > K:
                        kth = max(kth, float(np.partition(tv, len(tv) - K)[len(tv) - K]))
                    m = tv > max(lo_count, kth - margin)
                    top_idx, top_v, held = [ti[m]], [tv[m]], int(m.sum())
        amb = np.concatenate(amb)
        va = exact_values(F, t, *amb.T)
        ea = eps_of(F, t, amb[:, 0], amb[:, 1], amb[:, 2])
        self.count_hi = sure + int(np.count_nonzero(va > min_violation + ea))
        self.count_lo = sure + int(np.count_nonzero(va > min_violation - ea))
        ti, tv = np.concatenate(top_idx), np.concatenate(top_v)
        if K > 0 and len(tv) > K:
            kth = max(kth, float(np.partition(tv, len(tv) - K)[len(tv) - K]))
            m = tv > max(lo_count, kth - margin)
            ti = ti[m]
        vt = exact_values(F, t, *ti.T)
        m = vt > min_violation
        ti, vt = ti[m], vt[m]
        o = order(vt, ti[:, 0], ti[:, 1], ti[:, 2], ti[:, 3])
        self.p, self.q, self.s, self.c = (ti[o, k] for k in range(4))
        self.v = vt[o]
        self.F, self.t, self.K, self.min_violation = F, t, K, min_violation


def check_against_model(cones, min_violation, max_cuts, counts, cone, p, q, s, c, v, scans=None):
    """The assertions of a device result against the model.  cones = [(F, t)] per cone; counts per cone; the list (cone, p, q, s, c,
    v) is one cone's own (cone all zero) or the session's merged one: at most max_cuts in total, ordered by (v descending, cone, p, q,
    s, c ascending).  Prints every figure before it asserts.  Returns the Scans."""
    cone, p, q, s, c = (np.asarray(x, dtype=np.int64) for x in (cone, p, q, s, c))
    v = np.asarray(v, dtype=np.float64)
    kept = len(p)
    scans = scans or [Scan(F, t, min_violation, max(max_cuts, 1)) for F, t in cones]
    for k, sc in enumerate(scans):
        print("triangle cuts: cone %d, n %d, r %d: count %d, model [%d, %d]" % (k, sc.F.shape[0], sc.F.shape[1], counts[k], sc.count_hi,
                                                                               sc.count_lo))
        assert sc.count_hi <= counts[k] <= sc.count_lo, (k, sc.count_hi, counts[k], sc.count_lo)
    assert kept == min(int(np.sum(counts)), max_cuts), (kept, counts, max_cuts)
    if kept == 0:
        return scans
    nmax = max(F.shape[0] for F, _ in cones)
    key = lambda K_, P, Q, S, C_: (((K_ * nmax + P) * nmax + Q) * nmax + S) * 4 + C_  # noqa: E731
    assert ((0 <= cone) & (cone < len(cones))).all() and ((0 <= c) & (c < 4)).all()
    assert ((0 <= p) & (p < q) & (q < s) & (s < np.array([cones[k][0].shape[0] for k in cone]))).all()
    assert (v > min_violation).all()
    assert (order(v, p, q, s, c, cone) == np.arange(kept)).all(), "the list is not in the total order"
    assert len(np.unique(key(cone, p, q, s, c))) == kept
    ve = np.zeros(kept, dtype=np.longdouble)
    ee = np.zeros(kept)
    for k, (F, t) in enumerate(cones):
        m = cone == k
        ve[m] = exact_values(F, t, p[m], q[m], s[m], c[m])
        ee[m] = eps_of(F, t, p[m], q[m], s[m])
    worst = float(np.max(np.abs(v - ve) / ee))
    print("triangle cuts: kept %d, largest v %.6f, max |v - exact| / eps = %.3f" % (kept, v[0], worst))
    assert (np.abs(v - ve) <= ee).all(), worst
    # the model's merged list, complete down to rank max_cuts
    mc = np.concatenate([np.full(len(sc.v), k) for k, sc in enumerate(scans)])
    mp, mq, ms, mcl = (np.concatenate([getattr(sc, a) for sc in scans]) for a in "pqsc")
    mv = np.concatenate([sc.v for sc in scans])
    me = np.concatenate([eps_of(sc.F, sc.t, sc.p, sc.q, sc.s) for sc in scans])
    o = order(mv, mp, mq, ms, mcl, mc)
    mc, mp, mq, ms, mcl, mv, me = (x[o] for x in (mc, mp, mq, ms, mcl, mv, me))
    tau = mv[kept - 1] if kept <= len(mv) else np.longdouble(min_violation)
    print("triangle cuts: tau %.17g, min (v_listed - tau) / eps = %.3f" % (float(tau), float(np.min((ve - tau) / ee))))
    assert (ve >= tau - ee).all()
    listed = set(key(cone, p, q, s, c).tolist())
    un = np.array([k_ not in listed for k_ in key(mc, mp, mq, ms, mcl).tolist()], dtype=bool)
    if un.any():
        print("triangle cuts: max (v_unlisted - tau) / eps = %.3f" % float(np.max((mv[un] - tau) / me[un])))
        assert (mv[un] <= tau + me[un]).all()
    return scans


PLANT_D = np.array([[1.0, -1.0, 0.0], [0.0, 1.0, -1.0], [-1.0, 0.0, 1.0]])   # norm^2 2 each, every pairwise dot -1


def plant_rows(n, live=None):
    """F (n x 3) with row p = PLANT_D[p % 3] on the last `live` rows (None: all of them) and zero above.  With t = 1 every rho is one of
    2 (the same direction), -1 (two directions) and 0 (a zero row), so every v is a small integer, exact in any order:
      three directions              v = 2 in class 0, -2 in the others
      two rows of one direction     v = 1 in two classes, -1 and -5 in the others
      one direction                 v = 1 in three classes, -7 in class 0
      a zero row                    v <= -1 + |rho of the other two| <= 1"""
    F = PLANT_D[np.arange(n) % 3]
    if live is not None:
        F[:n - live] = 0.0
    return F


def plant_counts(n, live=None):
    """(pairs with v > 1.5, pairs with v > 0.5) of plant_rows(n, live) with t = 1, in closed form: c0 c1 c2 triples of three directions
    give one pair each above 1.5; above 0.5 a triple of live rows with exactly two equal directions gives two more, one of a single
    direction three, and a triple with one zero row and two live rows of one direction (rho = 0, 0, 2) two"""
    live = n if live is None else live
    c = np.bincount(np.arange(n - live, n) % 3, minlength=3).tolist()
    distinct = c[0] * c[1] * c[2]
    all_same = sum(comb(x, 3) for x in c)
    two_same = comb(live, 3) - distinct - all_same
    zero_and_pair = (n - live) * sum(comb(x, 2) for x in c)
    return distinct, distinct + 2 * two_same + 3 * all_same + 2 * zero_and_pair


def first_distinct_triples(rows, want):
    """the first `want` triples p < q < s of the ascending row numbers `rows` with three different p % 3, in (p, q, s) order"""
    out = []
    for i, a in enumerate(rows):
        for j in range(i + 1, len(rows)):
            for c in rows[j + 1:]:
                if len({a % 3, rows[j] % 3, c % 3}) == 3:
                    out.append((a, rows[j], c))
                    if len(out) == want:
                        return out
    return out


def c5_problem():
    """Max-Cut of the 5-cycle with unit weights as a generator dict: SDP value 4.52254, maximum cut 4"""
    ent = [(0, 1, i + 1, i + 1, 0.5) for i in range(5)]
    ent += [(0, 1, min(i, (i + 1) % 5) + 1, max(i, (i + 1) % 5) + 1, -0.25) for i in range(5)]
    ent += [(i + 1, 1, i + 1, i + 1, 1.0) for i in range(5)]
    return dict(m=5, blocks=[5], b=np.ones(5), entries=ent)


def tightened(prob, cuts):
    """the tightened problem of a generator dict: cuts = [(cone, p, q, s, cls)] 0-based.  Constraint m + 1 + e of cut e holds
    sign / (2 t_x t_y) at the three positions of its cone (an off-diagonal entry counts twice in <A, X>), -1 in column e of a new last
    LP block, b = -1.  No cuts: the problem itself."""
    cuts = list(cuts)
    if not cuts:
        return dict(m=prob["m"], blocks=list(prob["blocks"]), b=np.asarray(prob["b"], dtype=np.float64), entries=list(prob["entries"]))
    t = t_of(prob)
    m, nb = prob["m"], len(prob["blocks"])
    ent = list(prob["entries"])
    for e, (k, p, q, s, cl) in enumerate(cuts):
        for w, (x, y) in enumerate(((p, q), (p, s), (q, s))):
            ent.append((m + e + 1, k + 1, x + 1, y + 1, float(np.float64(SIGNS[cl][w]) / (2.0 * (t[k][x] * t[k][y])))))
        ent.append((m + e + 1, nb + 1, e + 1, e + 1, -1.0))
    return dict(m=m + len(cuts), blocks=list(prob["blocks"]) + [-len(cuts)],
                b=np.concatenate([np.asarray(prob["b"], dtype=np.float64), -np.ones(len(cuts))]), entries=ent)
