"""numpy restatement of the bisection rounding, written from the definition and independent of the device
code: the structure check on the file's entries, the repair to sum(sigma) = +-d, the swap search, f = x^T C x, and a brute force
over all balanced sign vectors.  The hyperplanes and their signs are tests/rounding_model.py's."""
import itertools

import numpy as np

from tests.admm_model import read_sdpa


class BisectProblem:
    """per cone: C (dense n x n, file units), t and d; b; ok / why (the structure check)"""

    def __init__(self, m, b, dims, ent):
        self.m, self.b, self.dims = m, np.asarray(b, dtype=np.float64), list(dims)
        self.C = [np.zeros((abs(n), abs(n))) for n in dims]
        self.t = [float("nan")] * len(dims)
        self.d = [-1] * len(dims)
        rows = {}
        for mat, blk, i, j, v in ent:
            if abs(v) < 1e-12:
                continue
            k, p, q = blk - 1, min(i, j) - 1, max(i, j) - 1
            if mat == 0:
                self.C[k][p, q] -= v
                if p != q:
                    self.C[k][q, p] -= v
            else:
                rows.setdefault(mat - 1, []).append((k, p, q, v))
        self.why = self._check(rows)
        self.ok = self.why == ""

    def _check(self, rows):
        if any(n <= 0 for n in self.dims):
            return "LP block or empty cone"
        tp = [np.full(n, np.nan) for n in self.dims]
        sums = [[] for _ in self.dims]
        for i in range(self.m):
            lst = rows.get(i, [])
            if not lst:
                return "constraint %d has no stored entry" % (i + 1)
            k = lst[0][0]
            n = self.dims[k]
            if any(e[0] != k for e in lst):
                return "constraint %d touches more than one cone" % (i + 1)
            if len(lst) == 1 and not (n == 1 and not np.isnan(tp[k][0])):
                _, p, q, a = lst[0]
                if p != q:
                    return "constraint %d is not on a diagonal" % (i + 1)
                if not self.b[i] / a > 0 or not np.isfinite(self.b[i] / a):
                    return "constraint %d has b / a not positive" % (i + 1)
                if not np.isnan(tp[k][p]):
                    return "diagonal %d of cone %d is fixed twice" % (p + 1, k + 1)
                tp[k][p] = np.sqrt(self.b[i] / a)
                continue
            pos = {(p, q) for _, p, q, _ in lst}
            a = lst[0][3]
            if len(lst) != n * (n + 1) // 2 or len(pos) != len(lst) or any(e[3] != a for e in lst):
                return "constraint %d is neither a diagonal row nor a sum row" % (i + 1)
            sums[k].append((i, a))
        for k, n in enumerate(self.dims):
            if np.isnan(tp[k]).any():
                return "a diagonal of cone %d is not fixed" % (k + 1)
            if np.any(tp[k] != tp[k][0]):
                return "cone %d has unequal diagonal values" % (k + 1)
            if len(sums[k]) != 1:
                return "cone %d has %d sum rows" % (k + 1, len(sums[k]))
            i, a = sums[k][0]
            q = self.b[i] / (a * tp[k][0] ** 2)
            d = int(np.floor(np.sqrt(q) + 0.5)) if q >= 0 else -1
            if d < 0 or not abs(q - d * d) <= 1e-9 * max(1.0, q) or d > n or (d - n) % 2:
                return "the sum row of cone %d has b / (a t^2) = %r" % (k + 1, float(q))
            self.t[k], self.d[k] = float(tp[k][0]), d
        return ""

    @classmethod
    def read(cls, path):
        return cls(*read_sdpa(path))

    @classmethod
    def from_instance(cls, prob):
        return cls(prob["m"], prob["b"], prob["blocks"], prob["entries"])

    def T(self, k):
        return self.dims[k] * self.t[k] ** 2


def _off(C):
    return C - np.diag(np.diag(C))


def objective(C, t, sigma):
    """f = x^T C x as sum_p x_p (h_p + C_pp x_p), x = t sigma"""
    x = t * sigma.astype(np.float64)
    return float(np.sum(x * (_off(C) @ x + np.diag(C) * x)))


def _argmin(vals, mask):
    """the index of the least value under the mask, the lowest index on ties (-1: the mask is empty)"""
    idx = np.nonzero(mask)[0]
    return int(idx[np.argmin(vals[idx])]) if len(idx) else -1


def repair(C, t, d, sigma, log=None):
    """|D - target| / 2 flips, target = +d where D >= 0 else -d: each flips the vertex of least Delta_p = -4 x_p h_p on the side in
    excess, the lowest index on ties.  Returns (sigma, D)."""
    sigma = sigma.astype(np.int64).copy()
    Coff = _off(C)
    D = int(sigma.sum())
    target = d if D >= 0 else -d
    side = 1 if D > target else -1
    for _ in range(abs(D - target) // 2):
        x = t * sigma
        delta = -4.0 * x * (Coff @ x)
        p = _argmin(delta, sigma == side)
        if log is not None:
            log.append(("flip", p, float(delta[p])))
        sigma[p] = -sigma[p]
    return sigma, D


def tau(C, t):
    return 4.0 * t * t * np.abs(_off(C)).sum(axis=1)


def swap_round(C, t, sigma):
    """the pair a round looks at: (p, q, Delta) of order A unless Delta_B < Delta_A, or None where a side is empty"""
    Coff = _off(C)
    x = t * sigma
    delta = -4.0 * x * (Coff @ x)
    best = None
    for plus in (1, -1):
        p = _argmin(delta, sigma == plus)
        if p < 0 or not np.any(sigma == -plus):
            continue
        v = delta + 8.0 * Coff[p] * x[p] * x
        q = _argmin(v, sigma == -plus)
        dl = float(delta[p] + v[q])
        if best is None or dl < best[2]:
            best = (p, q, dl)
    return best


def swap_search(C, t, sigma, max_rounds, log=None):
    """at most max_rounds rounds; a round swaps its pair where Delta < -2^-40 (tau_p + tau_q); the round that does not swap is the
    last and is counted.  Returns (sigma, rounds)."""
    sigma = sigma.astype(np.int64).copy()
    tv = tau(C, t)
    rounds = 0
    while rounds < max_rounds:
        rounds += 1
        pick = swap_round(C, t, sigma)
        if pick is None:
            break
        p, q, dl = pick
        if not dl < -2.0 ** -40 * (tv[p] + tv[q]):
            break
        if log is not None:
            log.append(("swap", p, q, dl))
        sigma[p], sigma[q] = -sigma[p], -sigma[q]
    return sigma, rounds


def run(C, t, d, sigma0, max_rounds, log=None):
    """one trial of one cone: dict(imbalance, sigma0 (after the repair), f0, sigma, f, rounds)"""
    s0, D = repair(C, t, d, sigma0, log)
    s1, rounds = swap_search(C, t, s0, max_rounds, log)
    return dict(imbalance=D, sigma0=s0, f0=objective(C, t, s0), sigma=s1, f=objective(C, t, s1), rounds=rounds)


def brute_force(C, t, d):
    """min of x^T C x over all sigma with sum(sigma) = +-d"""
    n = len(C)
    best = np.inf
    for npos in sorted({(n + d) // 2, (n - d) // 2}):
        for plus in itertools.combinations(range(n), npos):
            s = -np.ones(n, dtype=np.int64)
            s[list(plus)] = 1
            best = min(best, objective(C, t, s))
    return best
