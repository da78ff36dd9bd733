"""numpy model of the cut-tightened +-1 structure: what the recogniser, the appending writer, the rounding and
the second separation of a tightened problem must give.

  first_present     the present list of triangle_model.tightened(prob, cuts): cut e is row m + e, column e
  appended          the model's writer of a second tightening: present cuts dropped by a keep mask, the rest renumbered in order, new
                    cuts behind them (a generator dict, as triangle_model.tightened) and the present list of the result
  malformed         the tightened problem with one thing wrong, per case of the recogniser's refusals, and the words the reason must hold
  scaled            a tightened problem with one cut row multiplied by a positive factor
  union_adj         the neighbour lists of the union pattern (C's off-diagonal pattern and the cut positions): what the rounding's
                    local search colours on a tightened context
  packed            the 64-bit packed index ((p n + q) n + s) 4 + class
  dual_bound        d = b.y + sum_k T_k min(0, lambda_min(S_k)) + sum_j u_j min(0, s_j)  (kcut_model's, u_j = 4 scale_j)
"""
import numpy as np

from lorads_amd.cuts import SIGNS
from tests import kcut_model as km
from tests import triangle_model as tm


def first_present(prob, cuts):
    m = prob["m"]
    return [(k, p, q, s, cl, m + e, e) for e, (k, p, q, s, cl) in enumerate(cuts)]


def lp_block(prob):
    """the 1-based number of the LP block of a generator dict"""
    (lp,) = [k + 1 for k, n in enumerate(prob["blocks"]) if n < 0]
    return lp


def appended(prob, present, keep, new):
    """prob: a tightened generator dict whose cuts are `present` [(cone, p, q, s, cls, row, column)]; keep: one flag per present cut;
    new: [(cone, p, q, s, cls)].  Returns (the generator dict of the next problem, its present list)."""
    lp = lp_block(prob)
    keep = np.asarray(keep, dtype=bool)
    drop_rows = {c[5] for c, k in zip(present, keep) if not k}
    drop_cols = {c[6] for c, k in zip(present, keep) if not k}
    m, nl = prob["m"], -prob["blocks"][lp - 1]
    rowmap = np.cumsum([i not in drop_rows for i in range(m)]) - 1
    colmap = np.cumsum([j not in drop_cols for j in range(nl)]) - 1
    m2, nl2 = m - len(drop_rows), nl - len(drop_cols)
    t = tm.t_of(prob)
    ent = []
    for mat, blk, i, j, v in prob["entries"]:
        if mat > 0 and mat - 1 in drop_rows:
            continue
        if blk == lp:
            i, j = int(colmap[i - 1]) + 1, int(colmap[j - 1]) + 1
        ent.append((int(rowmap[mat - 1]) + 1 if mat > 0 else 0, blk, i, j, v))
    for e, (k, p, q, s, cl) in enumerate(new):
        for w, (x, y) in enumerate(((p, q), (p, s), (q, s))):
            ent.append((m2 + e + 1, k + 1, x + 1, y + 1, float(np.float64(SIGNS[cl][w]) / (2.0 * (t[k][x] * t[k][y])))))
        ent.append((m2 + e + 1, lp, nl2 + e + 1, nl2 + e + 1, -1.0))
    blocks = list(prob["blocks"])
    blocks[lp - 1] = -(nl2 + len(new))
    b = np.concatenate([np.asarray(prob["b"], dtype=np.float64)[[i for i in range(m) if i not in drop_rows]], -np.ones(len(new))])
    now = [(c[0], c[1], c[2], c[3], c[4], int(rowmap[c[5]]), int(colmap[c[6]])) for c, k in zip(present, keep) if k]
    now += [(k, p, q, s, cl, m2 + e, nl2 + e) for e, (k, p, q, s, cl) in enumerate(new)]
    return dict(m=m2 + len(new), blocks=blocks, b=b, entries=ent), now


def _copy(prob):
    return dict(m=prob["m"], blocks=list(prob["blocks"]), b=np.array(prob["b"], dtype=np.float64), entries=list(prob["entries"]))


def _cone_entries(prob, row):
    """indices into entries of constraint `row`'s (1-based) cone entries, in (i, j) order, and of its LP entry"""
    lp = lp_block(prob)
    idx = [e for e, x in enumerate(prob["entries"]) if x[0] == row and x[1] != lp]
    idx.sort(key=lambda e: prob["entries"][e][2:4])
    (le,) = [e for e, x in enumerate(prob["entries"]) if x[0] == row and x[1] == lp]
    return idx, le


def scaled(prob, row, factor):
    """constraint `row` (1-based) multiplied by factor > 0"""
    out = _copy(prob)
    out["entries"] = [(mat, blk, i, j, v * factor if mat == row else v) for mat, blk, i, j, v in out["entries"]]
    out["b"][row - 1] *= factor
    return out


def malformed(prob, m0):
    """{case: (generator dict, the words its first reason must hold)} of a tightened problem with at least two cuts whose cut rows
    start at constraint m0 + 1; every case changes one number of the file (the objective case adds the one entry it needs).
    The case 'two_cones' needs a problem with more than one cone and is left out otherwise."""
    lp, row = lp_block(prob), m0 + 1
    nl = -prob["blocks"][lp - 1]
    idx, le = _cone_entries(prob, row)
    out = {}

    def edit(case, needle, e=None, entry=None, fn=None):
        q = _copy(prob)
        if e is not None:
            q["entries"][e] = entry
        if fn is not None:
            fn(q)
        out[case] = (q, needle)

    mat, blk, i, j, v = prob["entries"][idx[0]]
    edit("coefficient", "constraint %d " % row, idx[0], (mat, blk, i, j, v + 1e-6))
    edit("b_sign", "constraint %d " % row, fn=lambda q: q["b"].__setitem__(row - 1, 1.0))
    mat, blk, i, j, v = prob["entries"][idx[2]]   # (q, s) -> (q, s'): no triangle any more
    n = prob["blocks"][blk - 1]
    taken = {prob["entries"][e][2:4] for e in idx}
    j2 = next(x for x in range(n, i, -1) if (i, x) not in taken and x != j)
    edit("no_triangle", "constraint %d " % row, idx[2], (mat, blk, i, j2, v))
    cones = [k + 1 for k, d in enumerate(prob["blocks"]) if d > 0 and k + 1 != blk and d >= j]
    if cones:
        edit("two_cones", "constraint %d " % row, idx[2], (mat, cones[0], i, j, v))
    edit("objective", "LP column 2 ", fn=lambda q: q["entries"].append((0, lp, 2, 2, 1.0)))
    mat, blk, i, j, v = prob["entries"][_cone_entries(prob, row + 1)[1]]   # the second cut's slack moves onto the first's column
    edit("column_twice", "LP column 1 ", _cone_entries(prob, row + 1)[1], (mat, blk, 1, 1, v))
    edit("column_unused", "LP column %d " % (nl + 1), fn=lambda q: q["blocks"].__setitem__(lp - 1, -(nl + 1)))
    return out


def union_adj(adj, cuts, cone):
    """the neighbour lists (ascending) of cone `cone` with the positions (p,q), (p,s), (q,s) of its cuts added to C's `adj`"""
    sets = [set(int(x) for x in a) for a in adj]
    for k, p, q, s, *_ in cuts:
        if k == cone:
            for x, y in ((p, q), (p, s), (q, s)):
                sets[x].add(y)
                sets[y].add(x)
    return [np.array(sorted(a), dtype=np.int64) for a in sets]


def packed(n, p, q, s, cl):
    return ((np.asarray(p, dtype=np.int64) * n + q) * n + s) * 4 + cl


def dual_bound(b, y, T, lam_min, scale, s_lp):
    """the tightened problem's bound: u_j = 4 scale_j (the slack of a triangle row is at most 4 of its rho units)"""
    return km.dual_bound(b, y, T, lam_min, 4.0 * np.asarray(scale, dtype=np.float64), s_lp)
