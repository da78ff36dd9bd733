"""numpy restatement of the stable-set rounding, written from the definition and independent of the device code.

Structure ("theta-structured").  At most one LP block, at least one SDP cone.  A constraint with an entry in the LP block is a bound
row 2 a X_pq + c x_j = b: one off-diagonal cone entry, one LP column, neither coefficient zero (kcut_model's rule and words); every LP
column sits in exactly one of them and has no objective.  Every other constraint lives in one cone and is either the cone's trace row
-- a on every one of its n diagonal positions and nowhere else, a > 0, b > 0: T = b / a, exactly one per cone -- or an edge row: one
off-diagonal entry (p, q), b = 0.  The edge rows are the cone's graph G.  C is arbitrary.  `why` is the first reason in the library's
words, constraints walked in their order.

Definition, per cone with factor F (n x r; R, or (U + V) / 2 formed per component) and directions G (r x K, rounding_model.hyperplanes
of the cone: the +-1 rounding's layout and counters, so trial t's direction is that rounding's hyperplane t; column 0 is generated and
not used):
  priority   pi_p0 = |F_p|^2 = X_pp;  pi_pt = F_p . g_t for t >= 1.
  order      q comes before p when pi_q > pi_p, or pi_q = pi_p and q < p.
  greedy     the lexicographically first maximal stable set in that order: walk the vertices in the order, take a vertex when none of
             its neighbours is taken.  The device's parallel fixed point (an undecided vertex joins when every neighbour that comes
             before it is out, then an undecided vertex with a neighbour that is in leaves; at most n + 1 rounds) gives the same set:
             fixed_point restates it.
  search     at most max_rounds rounds.  tau(u) = neighbours of u in S.  For v in S, L_v = {u not in S, u ~ v, tau(u) = 1} ascending;
             v is improvable when L_v holds a non-adjacent pair, its pair the lexicographically first (u, w), u < w.  The improvable v
             of least index leaves, its pair joins, then the greedy runs on the vertices with tau = 0 in the trial's order.  The round
             that finds no improvable v is the last; it is counted.  `rounds` of a call is the largest count over trials and cones.
  value      X(S) = T 1_S 1_S^T / |S|;  f = <C, X(S)> = (T / |S|) sum_{p, q in S} C_pq, in the file's units (theta files: -|S|).
  best       obj[t] = sum over the cones of f(t); best = the least obj[t], the least t on ties; obj0 / best0 for the greedy sets.
  bound      d = b.y + sum_k T_k min(0, lambda_min(S_k)) + sum_j u_j min(0, s_j), u_j = (|2 a| T / 2 + |b|) / |c| of the column's bound
             row (x_j = (b - 2 a X_pq) / c and |X_pq| <= (X_pp + X_qq) / 2 <= T / 2):  d <= optimum <= f, theta files |S| <= alpha <= -d.

Error bounds used by the tests (derived, not measured):
  score   one chain of r products in some order: |pi - exact| <= (r + 2) 2^-53 sum_j |F_pj| |g_jt|; trial 0 the same with F_pj^2.
          (The average (U + V) / 2 is formed exactly as the model forms it, so F is the same bits on both sides.)
  f       a member's row: at most min(longest stored row, |S|) additions of stored C_pq; a thread adds at most ceil(n / 256) rows; a
          tree of 8 levels over the 256 threads; T / |S| and its product: 2; the cones added in turn; C on the device is scale x C
          rounded once and f is divided by scale once: 2 more.  With L = min(longest row, |S|):
          |f - exact| <= sum over the cones of (L + ceil(n / 256) + 8 + 4 + cones) 2^-53 (T / |S|) sum_{p, q in S} |C_pq|.
"""
import numpy as np

from tests import rounding_model as rm
from tests.admm_model import read_sdpa
from tests.kcut_model import dual_bound  # noqa: F401  (the same formula: the LP term with this module's u)

U53 = 2.0 ** -53
LD = np.longdouble


def directions(seed, cone, rank, K):
    """G (rank x K) of one cone: the +-1 rounding's hyperplanes"""
    return rm.hyperplanes(seed, cone, rank, K)


class StableProblem:
    """A problem file seen as the check sees it.  cones / lp: indices of the SDP / LP blocks (file order); per SDP cone C (dense, file
    units), T, adj (neighbour arrays, ascending) and edges (p < q); rows: the bound rows (constraint, cone, p, q, a, column, c),
    0-based; why: None or the first reason the problem does not qualify; u: u_j per LP column."""

    def __init__(self, m, b, dims, ent):
        self.m, self.b, self.dims = m, np.asarray(b, dtype=np.float64), list(dims)
        self.lp = [k for k, d in enumerate(dims) if d < 0]
        self.cones = [k for k, d in enumerate(dims) if d > 0]
        self.C = {k: np.zeros((dims[k], dims[k])) for k in self.cones}
        self.cobj = {k: np.zeros(-dims[k]) for k in self.lp}
        con = {}
        for mat, blk, i, j, v in ent:
            if abs(v) < 1e-12:
                continue
            k, p, q = blk - 1, min(i, j) - 1, max(i, j) - 1
            if mat == 0:
                if k in self.C:
                    self.C[k][p, q] -= v
                    if p != q:
                        self.C[k][q, p] -= v
                else:
                    self.cobj[k][p] -= v
            else:
                con.setdefault(mat - 1, []).append((k, p, q, v))
        self.T, self.edges, self.rows, self.u = {}, {k: set() for k in self.cones}, [], np.zeros(0)
        self.why = self._check(con)
        self.ok = self.why is None
        self.adj = {}
        for k in self.cones:
            nb = [[] for _ in range(dims[k])]
            for p, q in sorted(self.edges[k]):
                nb[p].append(q)
                nb[q].append(p)
            self.adj[k] = [np.array(sorted(x), dtype=np.int64) for x in nb]

    def _check(self, con):
        if len(self.lp) > 1:
            return "more than one LP block"
        if not self.cones:
            return "no cone"
        lpk = self.lp[0] if self.lp else -1
        use = np.zeros(-self.dims[lpk], dtype=np.int64) if self.lp else np.zeros(0, dtype=np.int64)
        trace = {}
        for i in range(self.m):
            E = con.get(i, [])
            lp = [e for e in E if e[0] == lpk]
            sd = [e for e in E if e[0] != lpk]
            if lp:
                if len(lp) != 1:
                    return "constraint %d has %d LP entries" % (i + 1, len(lp))
                if len(sd) != 1:
                    return "constraint %d has an LP entry and %d cone entries" % (i + 1, len(sd))
                k, p, q, a = sd[0]
                if p == q:
                    return "constraint %d has an LP entry and a diagonal entry" % (i + 1)
                use[lp[0][1]] += 1
                self.rows.append((i, k, p, q, a, lp[0][1], lp[0][3]))
                continue
            if not sd:
                return "constraint %d has no stored entry" % (i + 1)
            k = sd[0][0]
            if any(e[0] != k for e in sd):
                return "constraint %d touches more than one cone" % (i + 1)
            diag = all(e[1] == e[2] for e in sd)
            if len(sd) == 1 and not diag:
                if self.b[i] != 0.0:
                    return "constraint %d is an edge row with b = %g (not 0)" % (i + 1, self.b[i])
                self.edges[k].add((sd[0][1], sd[0][2]))
                continue
            a = sd[0][3]
            if not diag or any(e[3] != a for e in sd) or len(sd) != self.dims[k]:
                return "constraint %d is neither a trace row nor an edge row of cone %d" % (i + 1, k + 1)
            if not a > 0 or not self.b[i] > 0 or not np.isfinite(self.b[i] / a):
                return "constraint %d is a trace row with a = %g, b = %g (not both positive)" % (i + 1, a, self.b[i])
            if k in trace:
                return "cone %d has two trace rows (constraints %d and %d)" % (k + 1, trace[k] + 1, i + 1)
            trace[k] = i
            self.T[k] = self.b[i] / a
        for k in self.cones:
            if k not in trace:
                return "cone %d has no trace row" % (k + 1)
        for j in range(len(use)):
            if use[j] != 1:
                return "LP column %d occurs in %d constraints" % (j + 1, use[j])
            if self.cobj[lpk][j] != 0.0:
                return "LP column %d has an objective coefficient" % (j + 1)
        self.u = np.zeros(len(use))
        for i, k, p, q, a, j, c in self.rows:
            self.u[j] = (abs(2.0 * a) * self.T[k] / 2.0 + abs(self.b[i])) / abs(c)
        return None

    @classmethod
    def read(cls, path):
        return cls(*read_sdpa(path))


def priorities(F, G):
    """pi (n x K) in longdouble: column 0 |F_p|^2, column t F_p . g_t"""
    Fl = np.asarray(F, dtype=LD)
    P = Fl @ np.asarray(G, dtype=LD)
    P[:, 0] = np.sum(Fl * Fl, axis=1)
    return P


def priority_bound(F, G):
    """(n x K) the bound on |pi_device - pi_exact| of the module's text"""
    Fa = np.abs(np.asarray(F, dtype=np.float64))
    B = Fa @ np.abs(G)
    B[:, 0] = np.sum(Fa * Fa, axis=1)
    return (F.shape[1] + 2) * U53 * B


def order(pi):
    """the vertices in the trial's order: priority descending, index ascending"""
    return sorted(range(len(pi)), key=lambda p: (-pi[p], p))


def greedy(adj, pi, member=None, cand=None):
    """the sequential greedy: member (bool n, the set so far; None: empty) completed over the candidates (None: all) in the order"""
    n = len(adj)
    S = np.zeros(n, dtype=bool) if member is None else member.copy()
    ok = np.ones(n, dtype=bool) if cand is None else cand
    for p in order(pi):
        if ok[p] and not S[p] and not S[adj[p]].any():
            S[p] = True
    return S


def fixed_point(adj, pi):
    """the device's parallel fixed point from the empty set, restated: (set, rounds)"""
    n = len(adj)
    UND, IN, OUT = 0, 1, 2
    s = np.zeros(n, dtype=np.int8)
    rounds = 0
    while (s == UND).any():
        rounds += 1
        assert rounds <= n + 1
        old = s.copy()
        for p in np.nonzero(old == UND)[0]:
            if all(old[q] == OUT or not (pi[q] > pi[p] or (pi[q] == pi[p] and q < p)) for q in adj[p]):
                s[p] = IN
        mid = s.copy()
        for p in np.nonzero(mid == UND)[0]:
            if any(mid[q] == IN for q in adj[p]):
                s[p] = OUT
    return s == IN, rounds


def swap_search(adj, pi, S, max_rounds):
    """the (1, 2)-swap search: (set, rounds run, the final round included)"""
    S = S.copy()
    n = len(adj)
    nbr = [set(int(q) for q in a) for a in adj]
    rounds = 0
    for _ in range(max_rounds):
        rounds += 1
        tau = np.array([int(S[adj[u]].sum()) for u in range(n)])
        found = None
        for v in np.nonzero(S)[0]:
            L = [int(u) for u in adj[v] if not S[u] and tau[u] == 1]
            for i, u in enumerate(L):
                for w in L[i + 1:]:
                    if w not in nbr[u]:
                        found = (int(v), u, w)
                        break
                if found:
                    break
            if found:
                break
        if not found:
            break
        v, u, w = found
        S[v] = False
        S[u] = S[w] = True
        free = np.array([not S[p] and not S[adj[p]].any() for p in range(n)])
        S = greedy(adj, pi, S, free)
    return S, rounds


def run_trial(adj, pi, max_rounds):
    """(greedy set, set after the search, rounds)"""
    S0 = greedy(adj, pi)
    S1, r = swap_search(adj, pi, S0, max_rounds) if max_rounds > 0 else (S0, 0)
    return S0, S1, r


def value(C, T, S):
    """(f in longdouble, (T / |S|) sum |C_pq| over S x S)"""
    idx = np.nonzero(S)[0]
    if len(idx) == 0:
        return LD(0), 0.0
    sub = np.asarray(C, dtype=LD)[np.ix_(idx, idx)]
    w = LD(T) / LD(len(idx))
    return w * sub.sum(), float(w * np.abs(sub).sum())


def f_bound(C, T, S, ncones):
    """the bound on |f_device - f_exact| of the module's text for one cone"""
    idx = np.nonzero(S)[0]
    n = len(S)
    longest = int((np.asarray(C) != 0).sum(axis=1).max()) if n else 0
    L = min(longest, len(idx))
    return (L + -(-n // 256) + 8 + 4 + ncones) * U53 * value(C, T, S)[1]


def is_stable(adj, S):
    return not any(S[p] and S[adj[p]].any() for p in range(len(adj)))


def is_maximal(adj, S):
    return all(S[p] or S[adj[p]].any() for p in range(len(adj)))


def alpha(adj):
    """the stability number by branching on a vertex of largest degree"""
    n = len(adj)
    nb = [0] * n
    for p in range(n):
        for q in adj[p]:
            nb[p] |= 1 << int(q)

    def rec(mask):
        if mask == 0:
            return 0
        best_p, best_d = -1, -1
        m = mask
        while m:
            p = (m & -m).bit_length() - 1
            m &= m - 1
            d = bin(nb[p] & mask).count("1")
            if d > best_d:
                best_p, best_d = p, d
        if best_d <= 1:   # isolated vertices and disjoint edges
            seen, cnt, m = 0, 0, mask
            while m:
                p = (m & -m).bit_length() - 1
                m &= m - 1
                if not (seen >> p) & 1:
                    cnt += 1
                    seen |= nb[p] & mask
            return cnt
        p = best_p
        return max(1 + rec(mask & ~(1 << p) & ~nb[p]), rec(mask & ~(1 << p)))

    return rec((1 << n) - 1)
