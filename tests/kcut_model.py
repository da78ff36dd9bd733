"""numpy restatement of the rounding into k parts, written from the definition and independent of the device
code: the counter-based generator with the part in the counter, the labels (scores in longdouble), f = sum <C, X(l)> (longdouble),
the applicability check with its reasons, the 1-move local search on the colouring of the stored off-diagonal graph, the bounds
u_j of the LP columns and the dual bound.

Error bounds used by the tests (derived, not measured):
  score   one chain of r products in some order: |s - exact| <= (r + 2) 2^-53 sum_j |R_pj| |g_ja|.  Two scores can swap when they
          differ by at most twice that: such a (row, trial) is "near".
  h_a     a sum of at most deg_p products: |h_a - exact| <= (deg_p + 2) 2^-53 sum_{q in a} |C_pq| t_q =: eh_pa (zero where every
          partial sum is exact: local_search says when).  An argmin over a can differ when a second part reaches the minimum within
          the two bounds; the move test Delta < -tau when |Delta + tau| <= coef t_p (eh_a* + eh_lp) + 4 2^-53 (|Delta| + tau).  Such
          a trial is "flagged".
  f       per row a sum of deg_p + 1 products, 4 waves and 256 strips and the cones added in turn:
          |f - exact| <= (longest row + 256 + cones + 8) 2^-53 sum_p t_p (|C_pp| t_p + sum_q |C_pq| t_q).
"""
import numpy as np

from tests import rounding_model as rm
from tests.admm_model import read_sdpa

U53 = 2.0 ** -53
LD = np.longdouble


def vectors(seed, cone, parts, rank, K):
    """G (parts x rank x K): rounding_model's generator at the counter (cone << 32) | (a << 26) | (t << 10) | j"""
    t = np.arange(K, dtype=np.uint64)[None, None, :]
    j = np.arange(rank, dtype=np.uint64)[None, :, None]
    a = np.arange(parts, dtype=np.uint64)[:, None, None]
    c = (np.uint64(cone) << np.uint64(32)) | (a << np.uint64(26)) | (t << np.uint64(10)) | j
    s = np.uint64(seed)
    with np.errstate(over="ignore"):
        x = rm.sm(s ^ rm.sm(np.uint64(2) * c))
        y = rm.sm(s ^ rm.sm(np.uint64(2) * c + np.uint64(1)))
    u1 = ((x >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (y >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def counter(cone, a, t, j):
    return (cone << 32) | (a << 26) | (t << 10) | j


def vector_int(seed, cone, a, t, j):
    """one value through big-integer splitmix64, written out on its own (the check of the uint64 restatement)"""
    m64 = (1 << 64) - 1

    def sm(x):
        z = (x + 0x9E3779B97F4A7C15) & m64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
        return z ^ (z >> 31)

    c = counter(cone, a, t, j)
    x, y = sm(seed ^ sm((2 * c) & m64)), sm(seed ^ sm((2 * c + 1) & m64))
    u1 = float((x >> 11) + 1) * 2.0 ** -53
    u2 = float(y >> 11) * 2.0 ** -53
    return float(np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2))


class KCutProblem:
    """A problem file seen as the check sees it.  cones: indices of the SDP blocks (file order); per SDP cone C (dense, file units),
    t and adj (the stored off-diagonal graph the colouring uses: C's non-zeros, and on a cone that stores C sparse also the positions
    of the bound rows); rows: the bound rows (constraint, cone, p, q, a, column, c), 0-based; why: None or the first reason the
    problem does not qualify, in the library's words; u: u_j per LP column."""

    def __init__(self, m, b, dims, ent):
        self.m, self.b, self.dims = m, np.asarray(b, dtype=np.float64), list(dims)
        self.lp = [k for k, d in enumerate(dims) if d < 0]
        self.cones = [k for k, d in enumerate(dims) if d > 0]
        self.C = {k: np.zeros((dims[k], dims[k])) for k in self.cones}
        cnz = {k: 0 for k in self.cones}
        self.cobj = {k: np.zeros(-dims[k]) for k in self.lp}
        con = {}
        for mat, blk, i, j, v in ent:
            if abs(v) < 1e-12:
                continue
            k, p, q = blk - 1, min(i, j) - 1, max(i, j) - 1
            if mat == 0:
                if k in self.C:
                    self.C[k][p, q] -= v
                    cnz[k] += 1
                    if p != q:
                        self.C[k][q, p] -= v
                else:
                    self.cobj[k][p] -= v
            else:
                con.setdefault(mat - 1, []).append((k, p, q, v))
        self.t = {k: np.full(dims[k], np.nan) for k in self.cones}
        self.rows, self.u = [], None
        self.why = self._check(con)
        self.ok = self.why is None
        self.adj = {}
        for k in self.cones:
            n = dims[k]
            G = self.C[k] != 0
            if not cnz[k] > 0.1 * (n * (n + 1) // 2):  # (the solver keeps C dense above that: the colouring then sees C alone)
                for _, kk, p, q, _, _, _ in self.rows:
                    if kk == k:
                        G[p, q] = G[q, p] = True
            np.fill_diagonal(G, False)
            self.adj[k] = [np.nonzero(G[p])[0] for p in range(n)]

    def _check(self, con):
        if len(self.lp) > 1:
            return "more than one LP block"
        if not self.cones:
            return "no cone"
        lpk = self.lp[0] if self.lp else -1
        cover = {k: np.zeros(self.dims[k], dtype=np.int64) for k in self.cones}
        use = np.zeros(-self.dims[lpk], dtype=np.int64) if self.lp else np.zeros(0, dtype=np.int64)
        for i in range(self.m):
            E = con.get(i, [])
            lp = [e for e in E if e[0] == lpk]
            sd = [e for e in E if e[0] != lpk]
            if not lp:
                if len(sd) != 1:
                    if not self.lp:   # (the +-1 check counts cone by cone: its message names the cone)
                        per = {}
                        for e in sd:
                            per[e[0]] = per.get(e[0], 0) + 1
                        bad = [k for k in sorted(per) if per[k] != 1]
                        if bad:
                            return "constraint %d has %d entries on cone %d" % (i + 1, per[bad[0]], bad[0] + 1)
                    return "constraint %d has %d stored entries" % (i + 1, len(sd))
                k, p, q, a = sd[0]
                if p != q:
                    return "constraint %d is not on a diagonal" % (i + 1)
                ratio = self.b[i] / a
                if not ratio > 0 or not np.isfinite(ratio):
                    return "constraint %d has b / a = %g (not positive)" % (i + 1, ratio)
                cover[k][p] += 1
                self.t[k][p] = np.sqrt(ratio)
            else:
                if len(lp) != 1:
                    return "constraint %d has %d LP entries" % (i + 1, len(lp))
                if len(sd) != 1:
                    return "constraint %d has an LP entry and %d cone entries" % (i + 1, len(sd))
                k, p, q, a = sd[0]
                if p == q:
                    return "constraint %d has an LP entry and a diagonal entry" % (i + 1)
                use[lp[0][1]] += 1
                self.rows.append((i, k, p, q, a, lp[0][1], lp[0][3]))
        for k in self.cones:
            for p in range(self.dims[k]):
                if cover[k][p] != 1:
                    return "diagonal %d of cone %d is fixed by %d constraints" % (p + 1, k + 1, cover[k][p])
        for j in range(len(use)):
            if use[j] != 1:
                return "LP column %d occurs in %d constraints" % (j + 1, use[j])
            if self.cobj[lpk][j] != 0.0:
                return "LP column %d has an objective coefficient" % (j + 1)
        self.u = np.zeros(len(use))
        for i, k, p, q, a, j, c in self.rows:
            self.u[j] = (abs(self.b[i]) + 2.0 * abs(a) * self.t[k][p] * self.t[k][q]) / abs(c)
        return None

    @classmethod
    def read(cls, path):
        return cls(*read_sdpa(path))

    def T(self, k):
        return float(np.sum(self.t[k] ** 2))


def scores(R, G):
    """P (parts x n x K) in longdouble"""
    Rl = np.asarray(R, dtype=LD)
    return np.stack([Rl @ np.asarray(G[a], dtype=LD) for a in range(G.shape[0])])


def labels(R, G):
    """(labels n x K: the lowest a that attains max_a R_p . g_a; near n x K: the top two scores differ by at most
    2 (r + 2) 2^-53 max_a sum_j |R_pj| |g_ja|)"""
    P = scores(R, G)
    lab = np.argmax(P, axis=0).astype(np.uint8)
    top = np.sort(P, axis=0)
    mag = np.max(np.stack([np.abs(R) @ np.abs(G[a]) for a in range(G.shape[0])]), axis=0)
    near = (top[-1] - top[-2]).astype(np.float64) <= 2.0 * (R.shape[1] + 2) * U53 * mag
    return lab, near


def point(t, lab, k):
    """X(l) (dense) of one labeling"""
    same = lab[:, None] == lab[None, :]
    return np.outer(t, t) * np.where(same, 1.0, -1.0 / (k - 1))


def objective(C, t, lab, k, dtype=LD):
    """f_t = <C, X(l_t)> for every column of lab (n x K)"""
    Cl, tl = np.asarray(C, dtype=dtype), np.asarray(t, dtype=dtype)
    Coff = Cl - np.diag(np.diag(Cl))
    diag = np.sum(np.diag(Cl) * tl * tl)
    allp = tl @ Coff @ tl
    same = np.zeros(lab.shape[1], dtype=dtype)
    for a in range(k):
        Z = np.where(lab == a, tl[:, None], dtype(0))
        same = same + np.einsum("pt,pt->t", Z, Coff @ Z)
    return diag + same - (allp - same) / dtype(k - 1)


def f_bound(Cs, ts, adjs):
    """the bound on |f_device - f_exact| of the module's text, for lists of cones"""
    longest = max(max((len(a) for a in adj), default=0) for adj in adjs) + 1
    mag = sum(float(np.sum(t * (np.abs(C) @ t))) for C, t in zip(Cs, ts))
    return (longest + 256 + len(Cs) + 8) * U53 * mag


def local_search(C, t, adj, lab, k, max_rounds, record=None):
    """The 1-move local search on every trial (columns of lab): rounds over the colour classes of `adj` in increasing order; p moves to
    a* = the lowest a attaining min_a h_a where Delta = coef t_p (h_a* - h_lp) < -tau_p.  Returns (labels, rounds, flagged per trial).
    A trial is flagged when a decision of its run could fall the other way within the error of h: eh_pa = (deg_p + 2) 2^-53
    sum_{q in a} |C_pq| t_q bounds the error of h_a in any summation order; it is zero for an empty part, and zero for a row whose
    products C_pq t_q are all multiples of 2^-30 with sum |C_pq| t_q < 2^20 (every partial sum is then exact in 53 bits, whatever
    the order).  The argmin is ambiguous when a second part can reach the minimum within the two bounds and one of them is not zero
    (equal exact values give the lowest a on both sides); the move test when |Delta + tau| <= coef t_p (eh_a* + eh_lp) +
    4 2^-53 (|Delta| + tau).  record: a list that receives (p, trial, Delta) of every accepted move."""
    lab = lab.copy()
    n, K = lab.shape
    col = rm.colouring(adj)
    Coff = C - np.diag(np.diag(C))
    Cabs = np.abs(Coff)
    coef = 2.0 * k / (k - 1)
    asum = Cabs @ t
    tau = 2.0 ** -40 * coef * t * asum
    deg = np.array([len(a) for a in adj], dtype=np.float64)
    prod = Coff * t[None, :] * 2.0 ** 30
    exact = np.all(prod == np.round(prod), axis=1) & (asum < 2.0 ** 20)
    unit = np.where(exact, 0.0, (deg + 2) * U53)
    classes = [np.nonzero(col == c)[0] for c in range(int(col.max()) + 1 if n else 0)]
    flagged = np.zeros(K, dtype=bool)
    rounds = 0
    for _ in range(max_rounds):
        rounds += 1
        moved = False
        for rows in classes:
            Z = [np.where(lab == a, t[:, None], 0.0) for a in range(k)]
            h = np.stack([Coff[rows] @ z for z in Z])                                   # parts x rows x K
            eh = np.stack([Cabs[rows] @ z for z in Z]) * unit[rows][None, :, None]
            amin = np.argmin(h, axis=0)
            cur = lab[rows][None].astype(np.int64)
            hmin, ehmin = h.min(axis=0), np.take_along_axis(eh, amin[None], axis=0)[0]
            hcur, ehcur = np.take_along_axis(h, cur, axis=0)[0], np.take_along_axis(eh, cur, axis=0)[0]
            cand = h - eh <= (h + eh).min(axis=0)[None]
            ambiguous = (cand.sum(axis=0) > 1) & (np.where(cand, eh, 0.0).max(axis=0) > 0)
            delta = coef * t[rows, None] * (hmin - hcur)
            err = coef * t[rows, None] * (ehmin + ehcur) + 4 * U53 * (np.abs(delta) + tau[rows, None])
            mv = delta < -tau[rows, None]
            close = (np.abs(delta + tau[rows, None]) <= err) & (err > 0)   # (err = 0: Delta = tau = 0 exactly on both sides)
            flagged |= np.any(close | (ambiguous & (amin != cur[0])), axis=0)
            if mv.any():
                moved = True
                if record is not None:
                    for i, tr in zip(*np.nonzero(mv)):
                        record.append((int(rows[i]), int(tr), float(delta[i, tr])))
                lab[rows] = np.where(mv, amin, lab[rows]).astype(lab.dtype)
        if not moved:
            break
    return lab, rounds, flagged


def move_deltas(C, t, lab, k):
    """(Delta n x K of the best move of every vertex, tau n): the 1-move-optimality test"""
    Coff = C - np.diag(np.diag(C))
    coef = 2.0 * k / (k - 1)
    h = np.stack([Coff @ np.where(lab == a, t[:, None], 0.0) for a in range(k)])
    hcur = np.take_along_axis(h, lab[None].astype(np.int64), axis=0)[0]
    return coef * t[:, None] * (h.min(axis=0) - hcur), 2.0 ** -40 * coef * t * (np.abs(Coff) @ t)


def dual_bound(b, y, T, lam_min, u=(), s=()):
    """d = b.y + sum_k T_k min(0, lambda_min(S_k)) + sum_j u_j min(0, s_j)"""
    return (float(np.dot(b, y)) + sum(Tk * min(0.0, lk) for Tk, lk in zip(T, lam_min)) +
            sum(uj * min(0.0, sj) for uj, sj in zip(u, s)))
