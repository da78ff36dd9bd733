#!/usr/bin/env python3
"""Synthetic SDPA (.dat-s) instance generators (bench workloads and parity-test inputs).

The reference ships no inputs, so every parity/bench instance is generated
here with a fixed seed and written in SDPA sparse format, the only format the reference reads
(reference: src_semi/io/lorads_file_io.c:21-293).  Conventions of that reader which the
generators rely on:

  * matrix number 0 is F0 and is NEGATED on load (C = -F0, lorads_file_io.c:279-281), so the
    solver minimises <-F0, X>;
  * entries are given once, upper triangle (i <= j), 1-based;
  * entries with |value| < 1e-12 are dropped (lorads_file_io.c:250).

Instances: maxcut (cfg2 / cfg3a), theta (cfg1), randsparse (cfg3b),
blockdiag maxcut (cfg4), matrix completion (cfg5), dense-C.
Each generator returns a dict(m, blocks=[n_k], b, entries=[(mat, blk, i, j, val)]) with 1-based
indices, and `write_sdpa` serialises it.
"""
import argparse
import math
import sys

import numpy as np


def _rand_edges(n, n_edges, rng):
    """n_edges distinct undirected edges (i<j) on n nodes, 0-based, deterministic for a seed."""
    max_e = n * (n - 1) // 2
    if n_edges > max_e:
        raise ValueError("too many edges")
    if n_edges > max_e // 3:
        iu, ju = np.triu_indices(n, 1)
        sel = rng.choice(max_e, size=n_edges, replace=False)
        sel.sort()
        return np.stack([iu[sel], ju[sel]], 1)
    seen = set()
    out = []
    while len(out) < n_edges:
        k = n_edges - len(out)
        a = rng.integers(0, n, size=2 * k + 16)
        b = rng.integers(0, n, size=2 * k + 16)
        for x, y in zip(a.tolist(), b.tolist()):
            if x == y:
                continue
            if x > y:
                x, y = y, x
            key = x * n + y
            if key in seen:
                continue
            seen.add(key)
            out.append((x, y))
            if len(out) == n_edges:
                break
    e = np.array(out, dtype=np.int64)
    order = np.lexsort((e[:, 1], e[:, 0]))
    return e[order]


def maxcut(n, n_edges, seed, weights=None):
    """max <L/4, X> s.t. X_ii = 1.  F0 = L/4 (=> C = -L/4), F_i = e_i e_i^T, b = 1."""
    rng = np.random.default_rng(seed)
    edges = _rand_edges(n, n_edges, rng)
    w = np.ones(len(edges)) if weights is None else weights(rng, len(edges))
    deg = np.zeros(n)
    np.add.at(deg, edges[:, 0], w)
    np.add.at(deg, edges[:, 1], w)
    ent = []
    for i in range(n):
        if deg[i] != 0.0:
            ent.append((0, 1, i + 1, i + 1, deg[i] / 4.0))
    for (i, j), wij in zip(edges.tolist(), w.tolist()):
        ent.append((0, 1, i + 1, j + 1, -wij / 4.0))
    for i in range(n):
        ent.append((i + 1, 1, i + 1, i + 1, 1.0))
    return dict(m=n, blocks=[n], b=np.ones(n), entries=ent)


def kpartite(k, m):
    """the complete k-partite graph on k m vertices (vertex v lies in part v // m) as a maxcut problem with unit weights: every
    edge is cut by the planted partition, k (k - 1) m^2 / 2 of them"""
    n = k * m
    ent = [(0, 1, i + 1, i + 1, (n - m) / 4.0) for i in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            if i // m != j // m:
                ent.append((0, 1, i + 1, j + 1, -0.25))
    for i in range(n):
        ent.append((i + 1, 1, i + 1, i + 1, 1.0))
    return dict(m=n, blocks=[n], b=np.ones(n), entries=ent)


def weighted_maxcut(n, n_edges, seed):
    """Max-Cut with edge weights drawn from [0.5, 2) (not dyadic: f is compared to a relative bound)"""
    return maxcut(n, n_edges, seed, weights=lambda rng, k: rng.uniform(0.5, 2.0, k))


def scaled_pm1(n, n_edges, seed):
    """+-1 QUBO relaxation in a scaled form: min <C, X> s.t. a_i X_ii = b_i with a_i, b_i of mixed signs and b_i / a_i > 0 (so
    X_ii = b_i / a_i, every x = sigma o sqrt(b / a) is feasible); C has off-diagonal entries of both signs and a diagonal."""
    rng = np.random.default_rng(seed)
    edges = _rand_edges(n, n_edges, rng)
    w = rng.uniform(-1.0, 1.0, len(edges))
    ent = []
    for i in range(n):
        ent.append((0, 1, i + 1, i + 1, float(rng.uniform(-0.5, 0.5))))
    for (i, j), wij in zip(edges.tolist(), w.tolist()):
        ent.append((0, 1, i + 1, j + 1, wij))
    sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    a = sgn * rng.uniform(0.5, 2.0, n)
    b = sgn * rng.uniform(0.5, 2.0, n)
    for i in range(n):
        ent.append((i + 1, 1, i + 1, i + 1, float(a[i])))
    return dict(m=n, blocks=[n], b=b, entries=ent)


def dense_maxcut(n, n_edges, seed):
    """Max-Cut on a dense graph: more than 0.1 n (n + 1) / 2 stored entries of C, so the solver keeps C dense"""
    assert n_edges + n > 0.1 * n * (n + 1) / 2
    return maxcut(n, n_edges, seed)


def maxcut_uncovered(n, n_edges, seed):
    """near miss of the +-1 structure: Max-Cut whose last diagonal is fixed by no constraint"""
    p = maxcut(n, n_edges, seed)
    ent = [e for e in p["entries"] if e[0] != n]
    return dict(m=n - 1, blocks=[n], b=np.ones(n - 1), entries=ent)


def maxcut_negative_ratio(n, n_edges, seed):
    """near miss of the +-1 structure: Max-Cut whose first constraint reads X_11 = -1 (b / a < 0)"""
    p = maxcut(n, n_edges, seed)
    b = np.ones(n)
    b[0] = -1.0
    return dict(m=n, blocks=[n], b=b, entries=p["entries"])


def _with_sum_row(prob, diff):
    """prob (one cone, the +-1 diagonal rows) plus the sum row <11^T, X> = diff^2 as its last constraint: every position of the upper
    triangle with the value 1"""
    n, m = prob["blocks"][0], prob["m"]
    ent = list(prob["entries"])
    for i in range(n):
        for j in range(i, n):
            ent.append((m + 1, 1, i + 1, j + 1, 1.0))
    return dict(m=m + 1, blocks=[n], b=np.concatenate([prob["b"], [float(diff * diff)]]), entries=ent)


def bisection_graph(n, edges, w, diff=0, t=1.0, a=1.0):
    """min <L/4, X> s.t. (1/t) X_ii = t, a <11^T, X> = a t^2 diff^2 on the graph with the edges `edges` (0-based pairs i < j, each
    once) of weights `w`, signed or not: the relaxation of the smallest cut with parts of (n + diff) / 2 and (n - diff) / 2 vertices
    (diff = 0: Min-Bisection) in a scaled form, x = t sigma.  F0 = -L/4 (=> C = L/4, x^T C x = t^2 times the cut's weight), the n
    diagonal rows, and the sum row last: every position of the upper triangle with the value a.  diff must have n's parity."""
    if not 0 <= diff <= n or (n - diff) % 2:
        raise ValueError("diff must lie in [0, n] and have n's parity")
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float64)
    deg = np.zeros(n)
    np.add.at(deg, edges[:, 0], w)
    np.add.at(deg, edges[:, 1], w)
    ent = [(0, 1, i + 1, i + 1, -(deg[i] / 4.0)) for i in range(n) if deg[i] != 0.0]
    ent += [(0, 1, i + 1, j + 1, wij / 4.0) for (i, j), wij in zip(edges.tolist(), w.tolist())]
    ent += [(i + 1, 1, i + 1, i + 1, 1.0 / t) for i in range(n)]
    ent += [(n + 1, 1, i + 1, j + 1, float(a)) for i in range(n) for j in range(i, n)]
    return dict(m=n + 1, blocks=[n], b=np.concatenate([np.full(n, float(t)), [float(a * t * t * diff * diff)]]), entries=ent)


def bisection(n, n_edges, seed, diff=0, weights=None):
    """bisection_graph with t = a = 1 on a seeded random graph: min <L/4, X> s.t. X_ii = 1, <11^T, X> = diff^2.  F0 = -L/4 (=> C =
    L/4, x^T C x the cut's weight for x in {+-1}^n), F_i = e_i e_i^T with b = 1, and the sum row last.  diff must have n's parity."""
    if not 0 <= diff <= n or (n - diff) % 2:
        raise ValueError("diff must lie in [0, n] and have n's parity")
    rng = np.random.default_rng(seed)
    edges = _rand_edges(n, n_edges, rng)
    return bisection_graph(n, edges, np.ones(len(edges)) if weights is None else weights(rng, len(edges)), diff)


def clique_pair(m, seed):
    """Min-Bisection of two cliques K_m joined by a perfect matching, the vertex labels shuffled by the seed: the smallest bisection
    separates the cliques and cuts the m matching edges, and the relaxation is tight (n lambda_2(L) / 4 = m for m >= 2)"""
    rng = np.random.default_rng(seed)
    n = 2 * m
    lab = rng.permutation(n)
    edges = [(a, b) for a in range(m) for b in range(a + 1, m)]
    edges += [(m + a, m + b) for a, b in edges]
    edges += [(a, m + a) for a in range(m)]
    ent = [(0, 1, i + 1, i + 1, -m / 4.0) for i in range(n)]  # every vertex has degree m
    for a, b in sorted((min(lab[a], lab[b]), max(lab[a], lab[b])) for a, b in edges):
        ent.append((0, 1, int(a) + 1, int(b) + 1, 0.25))
    for i in range(n):
        ent.append((i + 1, 1, i + 1, i + 1, 1.0))
    return _with_sum_row(dict(m=n, blocks=[n], b=np.ones(n), entries=ent), 0)


def theta(n, n_edges, seed):
    """Lovasz theta: max <J, X> s.t. tr X = 1, X_ij = 0 on edges.  m = n_edges + 1."""
    rng = np.random.default_rng(seed)
    edges = _rand_edges(n, n_edges, rng)
    ent = []
    for i in range(n):
        for j in range(i, n):
            ent.append((0, 1, i + 1, j + 1, 1.0))
    for i in range(n):
        ent.append((1, 1, i + 1, i + 1, 1.0))
    for k, (i, j) in enumerate(edges.tolist()):
        ent.append((k + 2, 1, i + 1, j + 1, 1.0))
    b = np.zeros(n_edges + 1)
    b[0] = 1.0
    return dict(m=n_edges + 1, blocks=[n], b=b, entries=ent)


def hamming_theta(d, max_distance):
    """Lovasz theta of the graph on {0,1}^d with an edge where the Hamming distance is 1 ... max_distance, in the form of theta():
    n = 2^d.  An independent set is a binary code of minimum distance max_distance + 1; theta' (theta with X >= 0 entry-wise,
    Schrijver) is the Delsarte bound: d = 5, max_distance = 2 has theta = 16/3 and theta' = 4."""
    n = 1 << d
    ent = []
    for i in range(n):
        for j in range(i, n):
            ent.append((0, 1, i + 1, j + 1, 1.0))
    for i in range(n):
        ent.append((1, 1, i + 1, i + 1, 1.0))
    k = 2
    for i in range(n):
        for j in range(i + 1, n):
            if bin(i ^ j).count("1") <= max_distance:
                ent.append((k, 1, i + 1, j + 1, 1.0))
                k += 1
    b = np.zeros(k - 1)
    b[0] = 1.0
    return dict(m=k - 1, blocks=[n], b=b, entries=ent)


def randsparse(n, m, seed, c_edges=None, n_diag=2, n_off=8, r0=5, dense_c=False):
    """cfg3b: m random sparse symmetric A_i with n_diag diagonal + n_off off-diagonal entries, values
    N(0,1); b = A(R0 R0^T), R0 ~ N(0,1)/sqrt(n) (n x r0) so the problem is feasible.  The objective
    is C = L/4 + I/4 (graph Laplacian of a random graph plus a multiple of the identity; positive
    definite, so min <C,X> over X >= 0 is bounded -- with C = -L/4 as in max-cut and no diagonal
    constraints the SDP is unbounded and the reference diverges), or a dense PD matrix."""
    rng = np.random.default_rng(seed)
    ent = []
    if dense_c:
        g = rng.standard_normal((n, n))
        cm = g @ g.T / n + np.eye(n)
        for i in range(n):
            for j in range(i, n):
                ent.append((0, 1, i + 1, j + 1, float(-cm[i, j])))
    else:
        ce = 6 * n if c_edges is None else c_edges
        edges = _rand_edges(n, ce, rng)
        deg = np.zeros(n)
        np.add.at(deg, edges[:, 0], 1.0)
        np.add.at(deg, edges[:, 1], 1.0)
        for i in range(n):  # F0 = -C  (the reader negates it back)
            ent.append((0, 1, i + 1, i + 1, -(deg[i] / 4.0 + 0.25)))
        for i, j in edges.tolist():
            ent.append((0, 1, i + 1, j + 1, 0.25))
    R0 = np.random.default_rng(seed + 1).standard_normal((n, r0)) / math.sqrt(n)
    b = np.zeros(m)
    for k in range(m):
        d = rng.choice(n, size=n_diag, replace=False)
        seen = set()
        offs = []
        while len(offs) < n_off:
            i, j = rng.integers(0, n, size=2).tolist()
            if i == j:
                continue
            if i > j:
                i, j = j, i
            if (i, j) in seen:
                continue
            seen.add((i, j))
            offs.append((i, j))
        vals = rng.standard_normal(n_diag + n_off)
        acc = 0.0
        for t, i in enumerate(sorted(d.tolist())):
            ent.append((k + 1, 1, i + 1, i + 1, float(vals[t])))
            acc += vals[t] * float(R0[i] @ R0[i])
        for t, (i, j) in enumerate(sorted(offs)):
            v = float(vals[n_diag + t])
            ent.append((k + 1, 1, i + 1, j + 1, v))
            acc += 2.0 * v * float(R0[i] @ R0[j])
        b[k] = acc
    return dict(m=m, blocks=[n], b=b, entries=ent)


def randsparse_sizes(n, sizes, seed, c_edges, r0=3):
    """randsparse's objective; constraint k has sizes[k] = (n_diag, n_off) entries, values N(0,1)/sqrt(n_diag + n_off) (unscaled,
    a constraint of 256 entries next to one of 1 leaves the CG too ill-conditioned for a float64 model to serve as a yardstick);
    b = A(R0 R0^T) as in randsparse"""
    base = randsparse(n, 0, seed, c_edges=c_edges, r0=r0)
    rng = np.random.default_rng(seed + 7)
    R0 = np.random.default_rng(seed + 1).standard_normal((n, r0)) / math.sqrt(n)
    ent, b = list(base["entries"]), []
    for k, (nd, no) in enumerate(sizes):
        d = sorted(rng.choice(n, size=nd, replace=False).tolist()) if nd else []
        seen = set()
        while len(seen) < no:
            i, j = rng.integers(0, n, size=2).tolist()
            if i != j:
                seen.add((min(i, j), max(i, j)))
        vals = rng.standard_normal(nd + no) / math.sqrt(nd + no)
        acc = 0.0
        for t, i in enumerate(d):
            ent.append((k + 1, 1, i + 1, i + 1, float(vals[t])))
            acc += vals[t] * float(R0[i] @ R0[i])
        for t, (i, j) in enumerate(sorted(seen)):
            v = float(vals[nd + t])
            ent.append((k + 1, 1, i + 1, j + 1, v))
            acc += 2.0 * v * float(R0[i] @ R0[j])
        b.append(acc)
    return dict(m=len(sizes), blocks=[n], b=np.array(b), entries=ent)


# (n_diag, n_off) per constraint: 1 .. 40 entries (k_cw takes 16 / 4 / 2 entries per trip at 8 / 32 / 64 lanes per entry, so the sizes
# 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40 straddle one, two and three trips), and up to 256
SIZES_1_40 = [(1, 0), (0, 1), (2, 0), (1, 1), (0, 3), (2, 3), (1, 6), (0, 8), (2, 7), (0, 15), (1, 15), (0, 17), (2, 29), (0, 32), (1, 32),
              (0, 33), (3, 37)]
SIZES_1_256 = SIZES_1_40 + [(0, 63), (0, 64), (1, 64), (0, 127), (0, 129), (5, 251)]


def prescribed_slack(S):
    """Max-Cut-type instance (X_ii = 1, one constraint per row) whose objective is the off-diagonal part of the symmetric matrix S:
    with the multipliers lambda = -diag(S) the slack C - sum_i lambda_i e_i e_i^T is S itself, entry for entry and without rounding
    (inputs of the dual-side tests whose spectrum is known in closed form).  Off-diagonal zeros of S are not stored."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    assert S.shape == (n, n) and np.array_equal(S, S.T)
    iu, ju = np.nonzero(np.triu(S, 1))
    ent = [(0, 1, int(i) + 1, int(j) + 1, float(-S[i, j])) for i, j in zip(iu, ju)]  # F0 = -C
    for i in range(n):
        ent.append((i + 1, 1, i + 1, i + 1, 1.0))
    return dict(m=n, blocks=[n], b=np.ones(n), entries=ent)


def randsparse_untouched_rows(n, m, seed, rows, **kw):
    """randsparse on n rows of which `rows` (0-based) are touched by no entry of C or of any A_i: the cone's union pattern has
    rows with an empty adjacency"""
    rows = sorted(set(int(r) for r in rows))
    live = [i for i in range(n) if i not in set(rows)]
    base = randsparse(len(live), m, seed, **kw)
    ent = [(mat, blk, live[i - 1] + 1, live[j - 1] + 1, v) for mat, blk, i, j, v in base["entries"]]
    return dict(m=m, blocks=[n], b=base["b"], entries=ent)


def with_dense_constraints(prob, n_dense, seed, r0=2):
    """appends n_dense constraints whose A_i is a DENSE symmetric matrix (every entry non-zero, N(0,1)/n): the reference stores
    such a coefficient packed (sdp_coeff_dense: nnz > 0.1 n(n+1)/2, data/lorads_sdp_data.c:811-828) and runs its dense
    kernels on it (:554-567, :698-732, dense LORADSUVt lorads_alg_common.c:50-67).  b_i = <A_i, R0 R0^T> keeps the problem
    feasible-ish (R0 drawn here; the solver converges to whatever the augmented problem's optimum is)."""
    (n,) = prob["blocks"]
    rng = np.random.default_rng(seed)
    R0 = rng.standard_normal((n, r0)) / math.sqrt(n)
    X0 = R0 @ R0.T
    ent = list(prob["entries"])
    b = list(prob["b"])
    m0 = prob["m"]
    for k in range(n_dense):
        g = rng.standard_normal((n, n)) / n
        a = (g + g.T) / 2
        for i in range(n):
            for j in range(i, n):
                ent.append((m0 + k + 1, 1, i + 1, j + 1, float(a[i, j])))
        b.append(float(np.sum(a * X0)))
    return dict(m=m0 + n_dense, blocks=[n], b=np.array(b), entries=ent)


def with_hub_rows(prob, n_hub, per_hub, seed, r0=2):
    """gives rows 0 .. n_hub-1 `per_hub` more operator slots each, far more than the fixed-width slot list of k_spmm_ell holds, so
    that its adjacency tail runs: per_hub / 2 appended constraints per hub row, each with two off-diagonal entries (p, q1), (p, q2)
    (N(0,1)) -- small constraints, so the one-kernel front stays eligible.  The partner rows q are drawn among rows with at most 6
    slots, so that the other rows keep at most 8.  b_i = <A_i, R0 R0^T>."""
    (n,) = prob["blocks"]
    rng = np.random.default_rng(seed)
    R0 = rng.standard_normal((n, r0)) / math.sqrt(n)
    deg = np.zeros(n, dtype=np.int64)
    for mat, blk, i, j, v in prob["entries"]:
        if mat > 0:
            deg[i - 1] += 1
            deg[j - 1] += i != j
    ent = list(prob["entries"])
    b = list(prob["b"])
    m = prob["m"]
    for h in range(n_hub):
        pool = np.array([q for q in range(n_hub, n) if deg[q] <= 6])
        cols = rng.choice(pool, size=per_hub, replace=False)
        vals = rng.standard_normal(per_hub)
        for t in range(0, per_hub - 1, 2):
            m += 1
            acc = 0.0
            for q, v in sorted(zip(cols[t:t + 2].tolist(), vals[t:t + 2].tolist())):
                ent.append((m, 1, q + 1, h + 1, v))
                acc += 2.0 * v * float(R0[h] @ R0[q])
                deg[q] += 1
            b.append(acc)
    return dict(m=m, blocks=[n], b=np.array(b), entries=ent)


def blockdiag_maxcut(nblk, n_k, edges_k, seed0):
    """cfg4: nblk independent max-cut blocks, block-separable constraints, m = nblk * n_k."""
    ent = []
    for k in range(nblk):
        sub = maxcut(n_k, edges_k, seed0 + k)
        for mat, _, i, j, v in sub["entries"]:
            if mat == 0:
                ent.append((0, k + 1, i, j, v))
            else:
                ent.append((mat + k * n_k, k + 1, i, j, v))
    ent.sort(key=lambda e: (e[0], e[1]))
    return dict(m=nblk * n_k, blocks=[n_k] * nblk, b=np.ones(nblk * n_k), entries=ent)


def block_diag(subs):
    """Independent single-block problems side by side: block-separable constraints (each A_i lives in one
    block), blocks of different size and kind."""
    ent, blocks, bs = [], [], []
    moff = 0
    for k, sub in enumerate(subs):
        assert len(sub["blocks"]) == 1
        for mat, _, i, j, v in sub["entries"]:
            ent.append((0 if mat == 0 else mat + moff, k + 1, i, j, v))
        moff += sub["m"]
        blocks.append(sub["blocks"][0])
        bs.append(np.asarray(sub["b"], dtype=np.float64))
    ent.sort(key=lambda e: (e[0], e[1]))
    return dict(m=moff, blocks=blocks, b=np.concatenate(bs), entries=ent)


def sdp_lp(n, n_edges, n_extra, seed):
    """SDP block + LP block (SDPA: a last block of negative dimension, diagonal entries only).
    max <L/4, X> - c's  s.t.  X_ii + s_i = 1 (one slack column per row: X_ii <= 1), plus n_extra LP columns that
    each sit in two neighbouring rows -- they couple rows, so the column-by-column ADMM update of the LP block has
    real Gauss-Seidel dependencies.  All LP costs positive (bounded)."""
    rng = np.random.default_rng(seed)
    edges = _rand_edges(n, n_edges, rng)
    deg = np.zeros(n)
    np.add.at(deg, edges[:, 0], 1.0)
    np.add.at(deg, edges[:, 1], 1.0)
    d = n + n_extra
    ent = []
    for i in range(n):
        if deg[i] != 0.0:
            ent.append((0, 1, i + 1, i + 1, deg[i] / 4.0))
    for i, j in edges.tolist():
        ent.append((0, 1, i + 1, j + 1, -0.25))
    cost = 0.05 + 0.2 * rng.random(d)
    for i in range(d):
        ent.append((0, 2, i + 1, i + 1, -float(cost[i])))  # F0 = -c  =>  C = -F0 = +c
    for i in range(n):
        ent.append((i + 1, 1, i + 1, i + 1, 1.0))
        ent.append((i + 1, 2, i + 1, i + 1, 1.0))
    for j in range(n_extra):
        r1 = int(rng.integers(0, n - 1))
        ent.append((r1 + 1, 2, n + j + 1, n + j + 1, float(0.3 + 0.5 * rng.random())))
        ent.append((r1 + 2, 2, n + j + 1, n + j + 1, float(0.2 + 0.4 * rng.random())))
    ent.sort(key=lambda e: (e[0], e[1]))
    return dict(m=n, blocks=[n, -d], b=np.ones(n), entries=ent)


def coupled_lp(nblk, n_k, m, n_lp, seed, n_free=0):
    """Coupled SDP cones (every A_i touches every cone) PLUS an LP block whose columns sit in two or three rows each:
    the general path -- cone-by-cone Gauss-Seidel sweep, then the level-scheduled LP column sweep.
    n_free: that many further columns behind them with a cost and no constraint entry (an empty entry range, ||a||^2 = 0); the
    first n_lp columns and everything else stay what they are without them."""
    base = coupled_blocks(nblk, n_k, m, seed, n_diag=1, n_off=2, r0=2, c_edges=2 * n_k)
    rng = np.random.default_rng(seed + 5)
    ent = list(base["entries"])
    b = np.array(base["b"], dtype=np.float64)
    for j in range(n_lp):
        ent.append((0, nblk + 1, j + 1, j + 1, -float(0.1 + 0.3 * rng.random())))  # cost > 0
        rows = rng.choice(m, size=int(rng.integers(2, 4)), replace=False)
        x0 = float(rng.random())  # a feasible point exists with these LP values
        for i in rows.tolist():
            a = float(0.2 + 0.8 * rng.random())
            ent.append((i + 1, nblk + 1, j + 1, j + 1, a))
            b[i] += a * x0
    for j in range(n_lp, n_lp + n_free):
        ent.append((0, nblk + 1, j + 1, j + 1, -float(0.1 + 0.3 * rng.random())))
    ent.sort(key=lambda e: (e[0], e[1]))
    return dict(m=m, blocks=list(base["blocks"]) + [-(n_lp + n_free)], b=b, entries=ent)


def coupled_blocks(nblk, n_k, m, seed, n_diag=2, n_off=4, r0=3, c_edges=None):
    """Block-diagonal SDP whose constraints COUPLE the blocks: every A_i has entries in every
    block (dense-cone branch per block; Gauss-Seidel != Jacobi)."""
    rng = np.random.default_rng(seed)
    ent = []
    b = np.zeros(m)
    for k in range(nblk):
        sub = randsparse(n_k, m, seed + 17 * (k + 1), c_edges=c_edges, n_diag=n_diag, n_off=n_off, r0=r0)
        for mat, _, i, j, v in sub["entries"]:
            ent.append((mat, k + 1, i, j, v))
        b += sub["b"]
    ent.sort(key=lambda e: (e[0], e[1]))
    return dict(m=m, blocks=[n_k] * nblk, b=b, entries=ent)


def matcomp(n1, n2, n_obs, rank, seed):
    """cfg5: matrix completion as an SDP on the (n1+n2) block; A_k = 1/2 (e_i e_j^T + e_j e_i^T)
    picks W_ij of the off-diagonal block, C = I (trace minimisation => F0 = -I)."""
    rng = np.random.default_rng(seed)
    n = n1 + n2
    L = rng.standard_normal((n1, rank))
    Rm = rng.standard_normal((n2, rank))
    seen = set()
    obs = []
    while len(obs) < n_obs:
        k = n_obs - len(obs)
        ii = rng.integers(0, n1, size=k + 16).tolist()
        jj = rng.integers(0, n2, size=k + 16).tolist()
        for i, j in zip(ii, jj):
            if (i, j) in seen:
                continue
            seen.add((i, j))
            obs.append((i, j))
            if len(obs) == n_obs:
                break
    obs.sort()
    ent = [(0, 1, i + 1, i + 1, -1.0) for i in range(n)]
    b = np.zeros(n_obs)
    for k, (i, j) in enumerate(obs):
        ent.append((k + 1, 1, i + 1, n1 + j + 1, 0.5))
        b[k] = float(L[i] @ Rm[j])
    return dict(m=n_obs, blocks=[n], b=b, entries=ent)


def write_sdpa(prob, path):
    with open(path, "w") as f:
        f.write("%d\n%d\n" % (prob["m"], len(prob["blocks"])))
        f.write(" ".join(str(d) for d in prob["blocks"]) + "\n")
        f.write(" ".join(repr(float(x)) for x in prob["b"]) + "\n")
        for mat, blk, i, j, v in prob["entries"]:
            f.write("%d %d %d %d %r\n" % (mat, blk, i, j, float(v)))


# named instances used by tests/golden and the bench
NAMED = {
    # small parity instances (sizes chosen so the reference picks the intended branch)
    "maxcut100": lambda: maxcut(100, 200, 101),            # sparse pattern branch, dense cone
    "theta30": lambda: theta(30, 40, 1),                   # dense C => dense (dsyr2k/dsymm) branch
    "theta50": lambda: theta(50, 103, 1),                  # cfg1 look-alike (m = 104)
    "rand120": lambda: randsparse(120, 40, 2001, c_edges=150, n_diag=2, n_off=3, r0=3),
    "blk4x60": lambda: blockdiag_maxcut(4, 60, 80, 4000),  # sparse-cone branch, separable
    "coupled3x70": lambda: coupled_blocks(3, 70, 30, 3100, n_diag=1, n_off=2, r0=2, c_edges=60),
    "densec40": lambda: randsparse(40, 20, 777, n_diag=1, n_off=2, r0=2, dense_c=True),
    "matcomp60": lambda: matcomp(30, 30, 200, 3, 50),
    # three DENSE constraint matrices next to sparse ones: the reference's dense-coefficient kernels (sdp_coeff_dense)
    "densea40": lambda: with_dense_constraints(randsparse(40, 17, 781, c_edges=60, n_diag=1, n_off=2, r0=2), 3, 782),
    # separable cones of different size and kind, equal rank 9: the lockstep (batched) sweep with row padding
    "mix4": lambda: block_diag([maxcut(60, 90, 61), randsparse(70, 45, 62, c_edges=90, n_diag=2, n_off=3, r0=3),
                                maxcut(66, 100, 63), matcomp(35, 33, 220, 3, 64)]),
    # one-kernel-front cones (LORADS_OP_CW=1) with hub rows 0..2: slot width 8 (<= 0.5 % of the rows over 8 slots) and 16; 810 rows,
    # so that the front's last workgroup holds rows past n (clamped to row 0)
    "hub8": lambda: with_hub_rows(randsparse(810, 200, 2101, c_edges=1600, n_diag=2, n_off=3, r0=3), 3, 40, 2102),
    "hub16": lambda: with_hub_rows(randsparse(810, 400, 2103, c_edges=1600, n_diag=2, n_off=8, r0=3), 3, 60, 2104),
    # ... and one with ten times as many constraints as rows: the constraint values outnumber the operator kernel's threads
    "wide60": lambda: randsparse(60, 600, 2105, c_edges=120, n_diag=1, n_off=2, r0=2),
    # constraints of unequal size (tests/test_unequal_constraints.py): k_cw on the constraint CSR; three trips of k_wsum (mixsz130,
    # mixsz300); a few huge constraints, so the older front under the constraint-wise operator (bigsz200); the constraint-wise
    # operator without a switch (m >= 256: mixsz300, and theta64x300 with a dense C); two such cones next to a Max-Cut cone (mixblk3)
    "mixsz130": lambda: randsparse_sizes(130, SIZES_1_40 * 2, 2201, 260),
    "bigsz200": lambda: randsparse_sizes(200, SIZES_1_256, 2203, 400),
    "mixsz300": lambda: randsparse_sizes(300, (SIZES_1_40 * 16)[:260], 2205, 900),
    "theta64x300": lambda: theta(64, 300, 3),
    "mixblk3": lambda: block_diag([randsparse_sizes(90, SIZES_1_40, 2207, 180),
                                   randsparse_sizes(70, SIZES_1_40[:12] + [(0, 1)] * 6, 2208, 140), maxcut(50, 80, 5)]),
    # Max-Cut cones of unequal size (and therefore unequal rank, data/lorads_solver.c:290-319), separable: one team of workgroups each
    "blkmix5": lambda: block_diag([maxcut(90, 140, 71), maxcut(120, 250, 72), maxcut(150, 400, 73), maxcut(260, 900, 74), maxcut(200, 500, 75)]),
    "densec300": lambda: randsparse(300, 60, 778, n_diag=2, n_off=4, r0=3, dense_c=True),  # dense C -> MFMA C.X path
    "densea300": lambda: with_dense_constraints(randsparse(300, 60, 783, c_edges=900, n_diag=2, n_off=4, r0=3), 4, 784),  # dense A_i -> MFMA path
    "denseac200": lambda: with_dense_constraints(randsparse(200, 40, 785, n_diag=2, n_off=4, r0=3, dense_c=True), 3, 786),  # dense C AND dense A_i
    # SDP cone + LP block (slacks and coupling columns): the LP path (closed-form column sweep)
    "sdplp40": lambda: sdp_lp(40, 90, 12, 4001),
    "sdpslack30": lambda: sdp_lp(30, 60, 0, 4002),
    "coupledlp": lambda: coupled_lp(2, 40, 24, 18, 5100),   # coupled cones + LP columns across rows (general path)         # slacks only: every LP column alone in its row (one level)
    # LP shapes of the ADMM column sweep (tests/test_fixed_count_sweeps.py::test_lp_block): 300 slack columns in one level (the
    # flat kernel on two workgroups); the same with 12 coupling columns, so that level 0 is longer than a workgroup and levels
    # follow it; coupledlp with one more column that has a cost and no constraint entry
    "sdpslack300": lambda: sdp_lp(300, 600, 0, 4003),
    "sdplp300": lambda: sdp_lp(300, 600, 12, 4004),
    "coupledlp_free": lambda: coupled_lp(2, 40, 24, 18, 5100, n_free=1),
    # +-1-structured contexts of the rounding and two near misses
    "wmaxcut150": lambda: weighted_maxcut(150, 400, 151),
    "scaledpm1_120": lambda: scaled_pm1(120, 300, 121),
    "densemaxcut120": lambda: dense_maxcut(120, 2000, 122),
    "kpartite3x10": lambda: kpartite(3, 10),
    "kpartite4x6": lambda: kpartite(4, 6),
    "maxcut_uncovered60": lambda: maxcut_uncovered(60, 120, 123),
    "maxcut_negratio60": lambda: maxcut_negative_ratio(60, 120, 124),
    # bisection-structured contexts of the balanced rounding: the sum row in the sparse structures (n < 32), in
    # the dense store, a prescribed size difference, and the two-clique graphs whose relaxation is tight
    "bisect24": lambda: bisection(24, 80, 241),
    "bisect40d4": lambda: bisection(40, 160, 401, diff=4),
    "cliquepair12": lambda: clique_pair(12, 121),
    "cliquepair16": lambda: clique_pair(16, 161),
    # timing / log-level instances
    "maxcut800": lambda: maxcut(800, 19176, 8001),         # cfg2 G1-like
    "maxcut4000": lambda: maxcut(4000, 24000, 4000),       # cfg3a-mini
    "rand4000": lambda: randsparse(4000, 1000, 20001, c_edges=24000),  # cfg3b-mini
    "matcomp4000": lambda: matcomp(2000, 2000, 16000, 5, 777),   # single-entry constraints at a size the reference solves
    "sdplp2000": lambda: sdp_lp(2000, 8000, 300, 4100),            # SDP cone + 2300 LP columns
    # headline configs
    "maxcut20000": lambda: maxcut(20000, 120000, 20000),   # cfg3a
    "rand20000": lambda: randsparse(20000, 5000, 20001, c_edges=120000),  # cfg3b (headline bench)
    "blk16x4000": lambda: blockdiag_maxcut(16, 4000, 24000, 4000),  # cfg4
    "blk2x4000": lambda: blockdiag_maxcut(2, 4000, 24000, 4000),    # what ONE of eight GPUs holds of cfg4 (two of its sixteen cones)
    "matcomp50000": lambda: matcomp(25000, 25000, 200000, 10, 50000),  # cfg5
    # cfg4's shape with cones of unequal size, n_k in [2000, 6000] (unequal ranks: VERDICT r3 #6)
    "blk16var": lambda: block_diag([maxcut(2000 + 250 * k, 6 * (2000 + 250 * k), 4100 + k) for k in range(16)]),
    # eight cones of the headline's kind (random sparse constraints), unequal sizes => unequal ranks: the lockstep sweep and the
    # single-cone forms of phase 1 on cones that only share a device rank (csrc/hip/build.inc: common_rank)
    "randblk8var": lambda: block_diag([randsparse(1500 + 250 * k, 400 + 60 * k, 5200 + k, c_edges=6 * (1500 + 250 * k)) for k in range(8)]),
}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("name", choices=sorted(NAMED))
    ap.add_argument("out")
    a = ap.parse_args(argv)
    write_sdpa(NAMED[a.name](), a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
