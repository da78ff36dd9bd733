"""numpy model of the top-k search per row of the primal: what lorads_hip_primal_topk must return.

F (n x r, the factor at the cone's own rank), X = F F^T.  For query row p the candidates are the columns q of [lo, hi), minus q = p
unless include_diag, minus the query's skip list, minus every q with X_pq NaN.  The total order is (X_pq descending, q ascending);
with `smallest`, (X_pq ascending, q ascending); -0.0 and +0.0 are one value.

The error bound of one X_pq (derived, not measured): a dot product of r terms in any summation order, fused or not, errs by at most
gamma_r sum |.| <= r 2^-53 |F_p| |F_q| to first order; one more unit covers the second-order terms and the float64 norms.  So

    eps(p, q) = (r + 1) 2^-53 |F_p| |F_q|

bounds |X_computed - X_exact|.  The longdouble evaluation (64-bit mantissa: its own error is 2^-11 of that) stands for the exact
value.
"""
import numpy as np

U53 = 2.0 ** -53


def eps_of(F, p, q):
    F = np.asarray(F, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        nr = np.sqrt((F ** 2).sum(1))
        return (F.shape[1] + 1) * U53 * nr[p] * nr[q]


def skip_sets(nq, skip):
    """skip: None, a list of integer sequences (one per query) or a (ptr, col) pair -> a list of sets"""
    if skip is None:
        return [set() for _ in range(nq)]
    if isinstance(skip, tuple):
        ptr, col = skip
        return [set(int(c) for c in col[ptr[i]:ptr[i + 1]]) for i in range(nq)]
    return [set(int(c) for c in s) for s in skip]


def order(x, q, smallest):
    """the permutation of candidates with values x and columns q into the total order"""
    x = np.asarray(x) + 0   # (-0.0 + 0 = +0.0: lexsort would not tell them apart anyway, this says so)
    return np.lexsort((q, x if smallest else -x))


class Query:
    """one query in longdouble: q, x, e of all its candidates in the total order"""

    def __init__(self, F, Fl, p, lo, hi, smallest, include_diag, skip):
        q = np.arange(lo, hi)
        with np.errstate(invalid="ignore", over="ignore"):
            x = (Fl[p][None, :] * Fl[lo:hi]).sum(1) if hi > lo else np.zeros(0, dtype=np.longdouble)
        keep = ~np.isnan(x)
        if not include_diag:
            keep &= q != p
        if skip:
            keep &= ~np.isin(q, np.fromiter(skip, dtype=np.int64, count=len(skip)))
        q, x = q[keep], x[keep]
        o = order(x, q, smallest)
        self.q, self.x = q[o], x[o]
        self.e = eps_of(F, p, self.q)


def model_topk(F, rows, lo, hi, k, smallest=False, include_diag=False, skip=None):
    """(idx [nq, k] int32, val [nq, k] float64 -- the longdouble values rounded --, found [nq]) as the device lays them out"""
    F = np.asarray(F, dtype=np.float64)
    Fl = F.astype(np.longdouble)
    sk = skip_sets(len(rows), skip)
    idx = np.full((len(rows), k), -1, dtype=np.int32)
    val = np.zeros((len(rows), k))
    found = np.zeros(len(rows), dtype=np.int32)
    for i, p in enumerate(rows):
        m = Query(F, Fl, int(p), lo, hi, smallest, include_diag, sk[i])
        f = min(k, len(m.q))
        found[i] = f
        idx[i, :f] = m.q[:f]
        val[i, :f] = m.x[:f].astype(np.float64) + 0.0
    return idx, val, found


def check_against_model(F, rows, lo, hi, k, smallest, include_diag, skip, idx, val, found, what=""):
    """The assertions of a device result against the model; prints the worst figures before it asserts."""
    F = np.asarray(F, dtype=np.float64)
    Fl = F.astype(np.longdouble)
    n = F.shape[0]
    nq = len(rows)
    idx, val, found = np.asarray(idx), np.asarray(val), np.asarray(found)
    assert idx.shape == (nq, k) and val.shape == (nq, k) and found.shape == (nq,), (idx.shape, val.shape, found.shape)
    sk = skip_sets(nq, skip)
    worst_val = worst_in = worst_out = 0.0
    pinned = 0
    for i, p in enumerate(rows):
        p = int(p)
        m = Query(F, Fl, p, lo, hi, smallest, include_diag, sk[i])
        f = int(found[i])
        assert f == min(k, len(m.q)), (what, i, p, f, len(m.q))
        assert (idx[i, f:] == -1).all() and (val[i, f:] == 0.0).all() and not np.signbit(val[i, f:]).any(), (what, i)
        if f == 0:
            continue
        qi, vi = idx[i, :f].astype(np.int64), val[i, :f]
        assert ((lo <= qi) & (qi < hi) & (qi < n)).all(), (what, i, qi)
        assert len(set(qi.tolist())) == f, (what, i, "repeated column")
        assert not (set(qi.tolist()) & sk[i]), (what, i, "a skipped column is listed")
        assert include_diag or p not in qi, (what, i, "the diagonal is listed")
        assert not np.isnan(vi).any(), (what, i)
        with np.errstate(invalid="ignore", over="ignore"):
            exact = (Fl[p][None, :] * Fl[qi]).sum(1)
        e = eps_of(F, p, qi)
        fin = np.isfinite(exact)
        assert np.array_equal(vi[~fin], exact[~fin].astype(np.float64)), (what, i, "infinite values")
        err = np.abs(vi[fin] - exact[fin])
        if err.size:
            worst_val = max(worst_val, float(np.max(err / np.maximum(e[fin], 1e-300))))
        assert (err <= e[fin]).all(), (what, i, p, float(np.max(err / np.maximum(e[fin], 1e-300))))
        # the list is in the total order by its own values
        sgn = -1.0 if smallest else 1.0
        a, b = sgn * vi[:-1], sgn * vi[1:]
        assert ((a > b) | ((a == b) & (qi[:-1] < qi[1:]))).all(), (what, i, "not in the total order")
        # against the model's k-th value
        sx, se = sgn * m.x, m.e
        finm = np.isfinite(sx)
        if len(m.q) > k:
            tau = sx[k - 1]
            if np.isfinite(tau):
                worst_in = max(worst_in, float(np.max(np.where(fin, (tau - sgn * exact) / np.maximum(e, 1e-300), -np.inf))))
                assert (sgn * exact[fin] >= tau - e[fin]).all(), (what, i, "a listed value is below tau - eps")
                un = ~np.isin(m.q, qi) & finm
                if un.any():
                    worst_out = max(worst_out, float(np.max((sx[un] - tau) / np.maximum(se[un], 1e-300))))
                    assert (sx[un] <= tau + se[un]).all(), (what, i, "an unlisted candidate is above tau + eps")
        else:
            assert set(qi.tolist()) == set(m.q.tolist()), (what, i)
        # where the model's neighbouring gaps exceed their two bounds the lists are equal
        upto = min(f + 1, len(m.q))
        with np.errstate(invalid="ignore"):
            gap_ok = (sx[:upto - 1] - sx[1:upto]) > (se[:upto - 1] + se[1:upto])   # [j]: between model positions j and j + 1
        before = np.concatenate([[True], gap_ok[:f - 1]])
        after = np.concatenate([gap_ok, [True]])[:f]
        pin = before & after
        pinned += int(pin.sum())
        assert np.array_equal(qi[pin], m.q[:f][pin]), (what, i, p, "the list is not the model's where the gaps decide")
    print("top-k %s: %d queries, k %d, found %d, pinned %d, max |v - exact| / eps %.3f, max (tau - listed) / eps %.3f, "
          "max (unlisted - tau) / eps %.3f" % (what, nq, k, int(found.sum()), pinned, worst_val, worst_in, worst_out))
