"""numpy restatement of the hyperplane rounding, written from the definition and independent of the device
code: the counter-based generator in uint64 arithmetic, the signs, f = x^T C x, the greedy colouring, the 1-flip local search and
the dual bound."""
import numpy as np

from tests.admm_model import read_sdpa

M64 = (1 << 64) - 1
GOLD = np.uint64(0x9E3779B97F4A7C15)


def sm_int(x):
    """splitmix64 of a Python integer: the output of the generator whose state was x before its step (big-integer arithmetic)"""
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sm(x):
    """splitmix64 of a uint64 array (wrapping numpy arithmetic)"""
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=np.uint64) + GOLD
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniforms(seed, cone, trials, rank):
    """(u1, u2) of every (column j, trial t), shape rank x len(trials)"""
    t = np.asarray(trials, dtype=np.uint64)[None, :]
    j = np.arange(rank, dtype=np.uint64)[:, None]
    c = (np.uint64(cone) << np.uint64(32)) | (t << np.uint64(10)) | j
    s = np.uint64(seed)
    with np.errstate(over="ignore"):
        a = sm(s ^ sm(np.uint64(2) * c))
        b = sm(s ^ sm(np.uint64(2) * c + np.uint64(1)))
    u1 = ((a >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (b >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return u1, u2


def hyperplanes(seed, cone, rank, K):
    """G (rank x K) of one cone: g = sqrt(-2 ln u1) cos(2 pi u2)"""
    u1, u2 = uniforms(seed, cone, np.arange(K), rank)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def hyperplane_int(seed, cone, t, j):
    """one value through big-integer splitmix64 (the check of the uint64 restatement)"""
    c = (cone << 32) | (t << 10) | j
    a = sm_int(seed ^ sm_int(2 * c))
    b = sm_int(seed ^ sm_int(2 * c + 1))
    u1 = float((a >> 11) + 1) * 2.0 ** -53
    u2 = float(b >> 11) * 2.0 ** -53
    return float(np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2))


class Pm1Problem:
    """per cone: C (dense n x n, file units), t, and the off-diagonal neighbour lists (ascending); b"""

    def __init__(self, m, b, dims, ent):
        self.m, self.b, self.dims = m, np.asarray(b, dtype=np.float64), list(dims)
        self.C = [np.zeros((n, n)) for n in dims]
        self.t = [np.full(n, np.nan) for n in dims]
        a = {}
        for mat, blk, i, j, v in ent:
            if abs(v) < 1e-12:
                continue
            k, p, q = blk - 1, min(i, j) - 1, max(i, j) - 1
            if mat == 0:
                self.C[k][p, q] -= v
                if p != q:
                    self.C[k][q, p] -= v
            else:
                a.setdefault(mat - 1, []).append((k, p, q, v))
        self.ok = all(n > 0 for n in dims) and len(a) == m
        for i, lst in a.items():
            if len(lst) != 1 or lst[0][1] != lst[0][2] or not self.b[i] / lst[0][3] > 0:
                self.ok = False
                continue
            k, p, _, v = lst[0]
            if not np.isnan(self.t[k][p]):
                self.ok = False
            self.t[k][p] = np.sqrt(self.b[i] / v)
        self.ok = self.ok and all(not np.isnan(t).any() for t in self.t)
        self.adj = [[np.nonzero((C[p] != 0) & (np.arange(len(C)) != p))[0] for p in range(len(C))] for C in self.C]

    @classmethod
    def read(cls, path):
        return cls(*read_sdpa(path))

    def T(self, k):
        return float(np.sum(self.t[k] ** 2))


def signs(R, G):
    """sigma (n x K): +1 where R_p . g_t >= 0 (and the projections, for the near-zero exclusion)"""
    P = R @ G
    return np.where(P >= 0, 1, -1).astype(np.int8), P


def objective(C, t, sigma):
    """f_t = x_t^T C x_t for every column of sigma (x = sigma o t)"""
    X = sigma * t[:, None]
    return np.einsum("pt,pt->t", X, C @ X)


def colouring(adj):
    """greedy colouring in increasing vertex order: a vertex takes the smallest colour none of its lower-numbered neighbours holds"""
    col = np.zeros(len(adj), dtype=np.int64)
    for p in range(len(adj)):
        used = {int(col[q]) for q in adj[p] if q < p}
        c = 0
        while c in used:
            c += 1
        col[p] = c
    return col


def local_search(C, t, adj, sigma, max_rounds):
    """the 1-flip local search on every trial (columns of sigma): rounds over the colour classes in increasing order, flip p where
    Delta_p = -4 x_p h_p < -tau_p, tau_p = 2^-40 4 t_p sum_{q != p} |C_pq| t_q; stop after a round without a flip or after max_rounds.
    Returns (sigma, rounds run)."""
    sigma = sigma.copy()
    col = colouring(adj)
    Coff = C - np.diag(np.diag(C))
    tau = 2.0 ** -40 * 4.0 * t * (np.abs(Coff) @ t)
    classes = [np.nonzero(col == c)[0] for c in range(int(col.max()) + 1 if len(col) else 0)]
    rounds = 0
    for _ in range(max_rounds):
        rounds += 1
        flipped = False
        for rows in classes:
            X = sigma * t[:, None]
            h = Coff[rows] @ X
            delta = -4.0 * X[rows] * h
            fl = delta < -tau[rows, None]
            if fl.any():
                flipped = True
                sigma[rows] = np.where(fl, -sigma[rows], sigma[rows])
        if not flipped:
            break
    return sigma, rounds


def deltas(C, t, sigma):
    """Delta_p (n x K) and tau_p (n) of every vertex: the 1-opt test"""
    Coff = C - np.diag(np.diag(C))
    X = sigma * t[:, None]
    return -4.0 * X * (Coff @ X), 2.0 ** -40 * 4.0 * t * (np.abs(Coff) @ t)


def dual_bound(b, y, T, lam_min):
    """d = b.y + sum_k T_k min(0, lambda_min(S_k))"""
    return float(np.dot(b, y)) + sum(Tk * min(0.0, lk) for Tk, lk in zip(T, lam_min))
