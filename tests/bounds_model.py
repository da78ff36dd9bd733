"""numpy model of the separation of entry bounds: what lorads_hip_entry_bounds must return.

Per cone: F (n x r, the factor at the cone's own rank), X = F F^T.  For p < q the violations are v = lower - X_pq (class 0) and
v = X_pq - upper (class 1).  The total order is (v descending, [cone,] p, q, class ascending).

The error bound of one v (derived, not measured): a dot product of r terms in any summation order, fused or not, errs by at most
gamma_r sum |.| <= r 2^-53 |F_p| |F_q| to first order, and the subtraction adds half a unit of |X_pq| + |bound|.  So

    eps(p, q) = (r + 2) 2^-53 (|F_p| |F_q| + |bound|)

bounds |v_computed - v_exact|.  The longdouble evaluation (64-bit mantissa: its own error is 2^-11 of that) stands for the exact
value.
"""
import numpy as np

U53 = 2.0 ** -53


def enumerate_all(F, lower, upper, dtype=np.longdouble):
    """(p, q, c, v) of all n (n - 1) (pair, class), by class inside the pair, pairs row by row"""
    F = np.asarray(F, dtype=dtype)
    n = F.shape[0]
    p, q = np.triu_indices(n, 1)
    x = (F[p] * F[q]).sum(1) if n > 1 else np.zeros(0, dtype=dtype)
    lo, up = dtype(lower), dtype(upper)
    with np.errstate(invalid="ignore"):
        v = np.stack([lo - x, x - up], 1).reshape(-1)
    return np.repeat(p, 2), np.repeat(q, 2), np.tile(np.array([0, 1]), len(p)), v


def order(v, p, q, c, cone=None):
    """the permutation into the total order (v descending, cone, p, q, c ascending)"""
    keys = [c, q, p] + ([cone] if cone is not None else []) + [-np.asarray(v)]
    return np.lexsort(tuple(keys))


def eps_of(F, p, q, c, lower, upper):
    """the per-item error bound (see the module's text); an infinite bound's class is off: its v is -inf exactly"""
    F = np.asarray(F, dtype=np.float64)
    nr = np.sqrt((F ** 2).sum(1))
    bound = np.where(np.asarray(c) == 0, lower, upper)
    fin = np.isfinite(bound)
    return np.where(fin, (F.shape[1] + 2) * U53 * (nr[p] * nr[q] + np.abs(np.where(fin, bound, 0.0))), 0.0)


class Scan:
    """One cone at (lower, upper, min_violation): every (pair, class) in longdouble,
      count_hi, count_lo   items with exact v > min_violation + eps / > min_violation - eps
      p, q, c, v           every item with exact v > min_violation, in the total order"""

    def __init__(self, F, lower, upper, min_violation):
        F = np.asarray(F, dtype=np.float64)
        P, Q, Cl, V = enumerate_all(F, lower, upper)
        e = eps_of(F, P, Q, Cl, lower, upper)
        self.count_hi = int(np.count_nonzero(V > min_violation + e))
        self.count_lo = int(np.count_nonzero(V > min_violation - e))
        m = V > min_violation
        o = order(V[m], P[m], Q[m], Cl[m])
        self.p, self.q, self.c, self.v, self.e = P[m][o], Q[m][o], Cl[m][o], V[m][o], e[m][o]
        self.F, self.lower, self.upper, self.min_violation = F, lower, upper, min_violation


def check_against_model(cones, lower, upper, min_violation, max_cuts, counts, cone, p, q, c, v, scans=None):
    """The assertions of a device result against the model.  cones = [F] per SDP cone in the order of `counts`; the list (cone, p, q,
    c, v) is one cone's own (cone all zero) or the session's merged one: at most max_cuts in total, ordered by (v descending, cone, p,
    q, c ascending).  Prints every figure before it asserts.  Returns the Scans."""
    cone, p, q, c = (np.asarray(x, dtype=np.int64) for x in (cone, p, q, c))
    v = np.asarray(v, dtype=np.float64)
    kept = len(p)
    scans = scans or [Scan(F, lower, upper, min_violation) for F in cones]
    for k, sc in enumerate(scans):
        print("entry bounds: cone %d, n %d, r %d: count %d, model [%d, %d]" % (k, sc.F.shape[0], sc.F.shape[1], counts[k], sc.count_hi,
                                                                              sc.count_lo))
        assert sc.count_hi <= counts[k] <= sc.count_lo, (k, sc.count_hi, counts[k], sc.count_lo)
    assert kept == min(int(np.sum(counts)), max_cuts), (kept, counts, max_cuts)
    if kept == 0:
        return scans
    nmax = max(F.shape[0] for F in cones)
    key = lambda K_, P, Q, C_: ((K_ * nmax + P) * nmax + Q) * 2 + C_  # noqa: E731
    assert ((0 <= cone) & (cone < len(cones))).all() and ((0 <= c) & (c < 2)).all()
    assert ((0 <= p) & (p < q) & (q < np.array([cones[k].shape[0] for k in cone]))).all()
    assert (v > min_violation).all()
    assert (order(v, p, q, c, cone) == np.arange(kept)).all(), "the list is not in the total order"
    assert len(np.unique(key(cone, p, q, c))) == kept
    ve = np.zeros(kept, dtype=np.longdouble)
    ee = np.zeros(kept)
    for k, F in enumerate(cones):
        m = cone == k
        Fl = np.asarray(F, dtype=np.longdouble)
        x = (Fl[p[m]] * Fl[q[m]]).sum(1)
        ve[m] = np.where(c[m] == 0, np.longdouble(lower) - x, x - np.longdouble(upper))
        ee[m] = eps_of(F, p[m], q[m], c[m], lower, upper)
    worst = float(np.max(np.abs(v - ve) / ee))
    print("entry bounds: kept %d, largest v %.6f, max |v - exact| / eps = %.3f" % (kept, v[0], worst))
    assert (np.abs(v - ve) <= ee).all(), worst
    # the model's merged list
    mc = np.concatenate([np.full(len(sc.v), k) for k, sc in enumerate(scans)])
    mp, mq, mcl = (np.concatenate([getattr(sc, a) for sc in scans]) for a in "pqc")
    mv = np.concatenate([sc.v for sc in scans])
    me = np.concatenate([sc.e for sc in scans])
    o = order(mv, mp, mq, mcl, mc)
    mc, mp, mq, mcl, mv, me = (x[o] for x in (mc, mp, mq, mcl, mv, me))
    tau = mv[kept - 1] if kept <= len(mv) else np.longdouble(min_violation)
    print("entry bounds: tau %.17g, min (v_listed - tau) / eps = %.3f" % (float(tau), float(np.min((ve - tau) / ee))))
    assert (ve >= tau - ee).all()
    listed = set(key(cone, p, q, c).tolist())
    un = np.array([k_ not in listed for k_ in key(mc, mp, mq, mcl).tolist()], dtype=bool)
    if un.any():
        print("entry bounds: max (v_unlisted - tau) / eps = %.3f" % float(np.max((mv[un] - tau) / me[un])))
        assert (mv[un] <= tau + me[un]).all()
    # where rounding cannot reorder the model's list (neighbours further apart than their two bounds), the lists are equal
    head = min(kept, len(mv))
    nxt = min(head + 1, len(mv))
    gaps = mv[:nxt - 1] - mv[1:nxt]
    if head == kept and bool(np.all(gaps > me[:nxt - 1] + me[1:nxt])):
        assert np.array_equal(key(cone, p, q, c), key(mc, mp, mq, mcl)[:kept]), "the list is not the model's"
    return scans


def bounded(prob, cuts):
    """the bounded problem of a generator dict: cuts = [(cone, p, q, cls, bound)] 0-based.  Constraint m + 1 + e of cut e holds 0.5 at
    (p, q) of its cone (an off-diagonal entry counts twice in <A, X>) and -1 (class 0) or +1 (class 1) in a slack column, b = bound.
    The slack columns are appended to the problem's LP block, or form a new last one.  No cuts: the problem itself."""
    cuts = list(cuts)
    blocks = list(prob["blocks"])
    ent = list(prob["entries"])
    b = np.asarray(prob["b"], dtype=np.float64)
    if not cuts:
        return dict(m=prob["m"], blocks=blocks, b=b, entries=ent)
    lps = [k for k, d in enumerate(blocks) if d < 0]
    assert len(lps) <= 1
    m = prob["m"]
    if lps:
        lp, col0 = lps[0], -blocks[lps[0]]
        blocks[lp] -= len(cuts)
    else:
        lp, col0 = len(blocks), 0
        blocks.append(-len(cuts))
    for e, (k, p, q, cl, bound) in enumerate(cuts):
        ent.append((m + e + 1, k + 1, p + 1, q + 1, 0.5))
        ent.append((m + e + 1, lp + 1, col0 + e + 1, col0 + e + 1, 1.0 if cl else -1.0))
    return dict(m=m + len(cuts), blocks=blocks, b=np.concatenate([b, np.array([c[4] for c in cuts], dtype=np.float64)]), entries=ent)


def antipodal_pairs(d):
    return [(i, (1 << d) - 1 - i) for i in range(1 << (d - 1))]
