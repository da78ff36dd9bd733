"""The constant behind CG iteration 0's step length on cones of the one-kernel front (csrc/hip/kernels.inc, Cg0Args).

k_wsum forms w_i = sum over the slots s of constraint i of a_s (p_row(s) . V_col(s)); k_spmm_ell forms
Q_p = p_p + sum over the slots s of row p of a_s w_con(s) V_col(s).  Regrouping the slots of p.Q by constraint gives
p.Q = ||p||^2 + ||w||^2, so alpha = rr / (p.Q) is known before the operator kernel runs (p_0 = r_0, rr = ||r_0||^2).
Checked here in numpy on the slot lists of the seeded instances, built the way build.inc builds them."""
import numpy as np
import pytest

from lorads_amd import instances


def _slots(prob):
    """(row, col, con, a) of every slot of block 0's constraints, in the device's convention (build.inc: an entry (p, q, a) of
    constraint i gives slot (p -> q) and, off the diagonal, slot (q -> p), both with coefficient a; rows ascending, each row's
    slots by (neighbour, constraint))."""
    rows, cols, cons, vals = [], [], [], []
    for mat, blk, i, j, v in prob["entries"]:
        if mat == 0 or blk != 1:
            continue
        p, q, k = i - 1, j - 1, mat - 1
        rows.append(p); cols.append(q); cons.append(k); vals.append(v)
        if p != q:
            rows.append(q); cols.append(p); cons.append(k); vals.append(v)
    rows, cols, cons, vals = (np.asarray(x) for x in (rows, cols, cons, vals))
    order = np.lexsort((cons, cols, rows))
    return rows[order], cols[order], cons[order], vals[order].astype(np.float64)


@pytest.mark.parametrize("name,r", [("rand120", 10), ("rand4000", 44)])
def test_pq_is_p_norm_plus_w_norm_on_the_slot_lists(name, r):
    prob = instances.NAMED[name]()
    n, m = prob["blocks"][0], prob["m"]
    rows, cols, cons, a = _slots(prob)
    assert len(a) > 0 and (rows != cols).any()
    rng = np.random.default_rng(7)
    for _ in range(3):
        p = rng.standard_normal((n, r))
        V = rng.standard_normal((n, r))
        contrib = a * np.einsum("ij,ij->i", p[rows], V[cols])      # k_front_cw's per-slot contributions
        w = np.bincount(cons, weights=contrib, minlength=m)           # k_wsum
        Q = p.copy()
        np.add.at(Q, rows, (a * w[cons])[:, None] * V[cols])          # k_spmm_ell, mode OP_CG
        pq = float(np.sum(p * Q))
        rule = float(np.sum(p * p)) + float(np.sum(w * w))
        assert abs(pq - rule) <= 1e-13 * abs(pq), (name, pq, rule)
