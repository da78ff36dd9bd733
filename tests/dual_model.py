"""Model of the dual side of the device path: the slack S_k = C_k - sum_i lambda_i A_ik, its smallest eigenvalue by the thick-restart
Lanczos process of csrc/hip/lanczos.inc, and the sums of the DIMACS certificate of csrc/hip/solution.inc.  For the comparisons of
tests/test_dual_edges.py (the device) and tests/test_dual_model.py (the model against independent arithmetic).

Plain numpy in np.longdouble (80-bit on x86 hosts) or np.float64 (to measure a case's conditioning by the spread between the two),
independent of the HIP library and of the oracle.  Written from the algorithm's description:

    start vector    v_i = 2 u_i - 1, u_i the top 53 bits of the 64-bit LCG s <- 6364136223846793005 s + 1442695040888963407
                    (s_0 = 0x9E3779B97F4A7C15), normalised -- in float64: the vector is an input of the process
    step j          w = S v_j;  h1 = V_j^T w, w -= V_j h1;  h2 = V_j^T w, w -= V_j h2  (classical Gram-Schmidt, twice, against the
                    whole basis);  alpha_j = h1_j + h2_j, beta_j = ||w||, tnorm = max(tnorm, |alpha_j|, beta_j) over the whole solve;
                    breakdown when not (beta_j > 1e-13 max(tnorm, 1e-300)): the Ritz values of the j + 1 steps are exact
    after a sweep   T = the projected matrix (after a restart: diag(theta_0..keep-1) with the arrow beta Y[mm - 1, i] in row and
                    column `keep`, tridiagonal behind), (theta, Y) its eigenpairs, res = |beta Y[mm - 1, 0]|;
                    stop on a breakdown, on res <= tol max(eps^(2/3), |theta_0|), at the restart budget, or when mm < 2
    thick restart   keep = min(8, mm - 1) lowest Ritz vectors, then the residual direction v_mm

The coefficients alpha, beta cross to float64 where the device reads them back (T, theta and Y are float64 on the host), the basis
stays in the model's precision.  No summation order of any device kernel is mirrored."""
import numpy as np

from tests.admm_model import read_sdpa

LD = np.longdouble
EPS = 2.220446049250313e-16
EPS23 = EPS ** (2.0 / 3.0)
KEEP_MAX = 8


def _problem(prob_or_path):
    if isinstance(prob_or_path, dict):
        p = prob_or_path
        return p["m"], np.asarray(p["b"], dtype=np.float64), list(p["blocks"]), p["entries"]
    m, b, dims, ent = read_sdpa(prob_or_path)
    return m, np.asarray(b, dtype=np.float64), dims, ent


def problem(prob_or_path):
    """the instance as a dict with its entries as arrays (entries below 1e-12 dropped, as the reader drops them): parse once, pass
    the dict to slack / certificate / dual_infeasibility"""
    if isinstance(prob_or_path, dict) and "_arr" in prob_or_path:
        return prob_or_path
    m, b, dims, ent = _problem(prob_or_path)
    e = np.array([t for t in ent if abs(t[4]) >= 1e-12], dtype=np.float64).reshape(-1, 5)
    arr = dict(mat=e[:, 0].astype(np.int64), blk=e[:, 1].astype(np.int64) - 1, i=e[:, 2].astype(np.int64) - 1,
               j=e[:, 3].astype(np.int64) - 1, v=e[:, 4].copy())
    return dict(m=m, b=b, blocks=dims, entries=ent, _arr=arr)


class Slack:
    """S of one cone: lower-triangle entries (row >= col, duplicates summed) with, per entry, `mag` = |C_e| + sum_i |lam_i a_i| --
    the scale of the entry's rounding.  An LP block holds its diagonal.  dense() is the full symmetric matrix, matvec(x) = S x."""

    def __init__(self, n, is_lp, row, col, val, mag, dtype):
        self.n, self.is_lp, self.dtype = n, is_lp, dtype
        self.row, self.col, self.val, self.mag = row, col, val, mag   # sorted by (row, col)
        off = self.row != self.col
        r = np.concatenate([self.row, self.col[off]])
        c = np.concatenate([self.col, self.row[off]])
        v = np.concatenate([self.val, self.val[off]])
        o = np.lexsort((c, r))
        self._r, self._c, self._v = r[o], c[o], v[o]
        self._starts = np.flatnonzero(np.diff(self._r, prepend=-1)) if len(r) else np.zeros(0, dtype=np.int64)
        self._rows = self._r[self._starts] if len(r) else np.zeros(0, dtype=np.int64)

    def dense(self):
        S = np.zeros((self.n, self.n), dtype=self.dtype)
        S[self._r, self._c] = self._v
        return S

    def diagonal(self):
        d = np.zeros(self.n, dtype=self.dtype)
        on = self.row == self.col
        d[self.row[on]] = self.val[on]
        return d

    def matvec(self, x):
        y = np.zeros(self.n, dtype=self.dtype)
        if len(self._r):
            y[self._rows] = np.add.reduceat(self._v * x[self._c], self._starts)
        return y


def slack(prob_or_path, lam, dtype=LD):
    """[Slack of cone k] for the multipliers lam, in the sign convention of common.slack_matrices: C = -F0, so an entry v of matrix 0
    gives -v and an entry v of matrix i gives -lam_i v (added in the file's order).  An LP entry is keyed by its row."""
    p = problem(prob_or_path)
    a, dims = p["_arr"], p["blocks"]
    lam = np.asarray(lam, dtype=np.float64).astype(dtype)
    v = a["v"].astype(dtype)
    isa = a["mat"] > 0
    w = -v
    w[isa] = -lam[a["mat"][isa] - 1] * v[isa]
    out = []
    for k, n in enumerate(dims):
        sel = np.flatnonzero(a["blk"] == k)
        i, j = a["i"][sel], a["j"][sel]
        r, c = (i, i) if n < 0 else (np.maximum(i, j), np.minimum(i, j))
        key, inv = np.unique(r * abs(n) + c, return_inverse=True)
        val, mag = np.zeros(len(key), dtype=dtype), np.zeros(len(key), dtype=np.float64)
        np.add.at(val, inv, w[sel])
        np.add.at(mag, inv, np.abs(w[sel]).astype(np.float64))
        out.append(Slack(abs(n), n < 0, key // abs(n), key % abs(n), val, mag, dtype))
    return out


def start_vector(n):
    """the fixed pseudo-random unit start vector (float64, every operation in the order it is written)"""
    s = 0x9E3779B97F4A7C15
    v = np.empty(n, dtype=np.float64)
    nr = 0.0
    for i in range(n):
        s = (s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        x = (float(s >> 11) / 9007199254740992.0) * 2.0 - 1.0
        v[i] = x
        nr += x * x
    return v * (1.0 / np.sqrt(nr))


class LanczosResult:
    def __init__(self, theta, matvecs, restarts, breakdown, res, m):
        self.theta, self.matvecs, self.restarts, self.breakdown, self.res, self.m = theta, matvecs, restarts, breakdown, res, m

    def __repr__(self):
        return "LanczosResult(theta=%r, matvecs=%d, restarts=%d, breakdown=%s, res=%.3e)" % (
            self.theta, self.matvecs, self.restarts, self.breakdown, self.res)


def lanczos(S, tol=1e-2, ncv=40, max_restarts=600, dtype=LD):
    """smallest Ritz value of S (a Slack, or a dense symmetric array) by the process of the module's header.  tol may be a
    sequence: the tolerance enters the stopping test alone, so one run serves them all and returns {tol: result}."""
    if not np.isscalar(tol):
        return _lanczos(S, sorted(set(float(t) for t in tol), reverse=True), ncv, max_restarts, dtype)
    return _lanczos(S, [float(tol)], ncv, max_restarts, dtype)[float(tol)]


def _lanczos(S, tols, ncv, max_restarts, dtype):
    if isinstance(S, Slack):
        n = S.n
        if S.dtype != dtype:
            raise ValueError("the slack was assembled in another precision")
        mv = S.matvec
    else:
        A = np.asarray(S).astype(dtype)
        n = A.shape[0]
        mv = lambda x: A @ x  # noqa: E731
    m = max(1, min(ncv, n))
    V = np.zeros((m + 1, n), dtype=dtype)
    V[0] = start_vector(n).astype(dtype)
    T = np.zeros((m, m), dtype=np.float64)
    k, nmv, tnorm = 0, 0, 0.0
    restart, done = 0, {}
    while True:
        mm, breakdown, beta = m, False, 0.0
        for j in range(k, m):
            w = mv(V[j])
            B = V[:j + 1]
            h1 = B @ w
            w = w - h1 @ B
            h2 = B @ w
            w = w - h2 @ B
            alpha = float(h1[j] + h2[j])
            beta = float(np.sqrt(max(dtype(0), w @ w)))
            nmv += 1
            T[j, j] = alpha
            tnorm = max(tnorm, abs(alpha), beta)
            if not np.isfinite(alpha) or not np.isfinite(beta):
                raise FloatingPointError("non-finite Lanczos coefficient")
            if not (beta > 1e-13 * max(tnorm, 1e-300)):
                mm, breakdown = j + 1, True
                break
            V[j + 1] = w * (dtype(1) / dtype(beta))
            if j + 1 < m:
                T[j, j + 1] = T[j + 1, j] = beta
        theta, Y = np.linalg.eigh(T[:mm, :mm])
        res = 0.0 if breakdown else abs(beta * Y[mm - 1, 0])
        for tol in tols:
            if tol not in done and (breakdown or res <= tol * max(EPS23, abs(theta[0])) or restart >= max_restarts or mm < 2):
                done[tol] = LanczosResult(float(theta[0]), nmv, restart, breakdown, res, m)
        if len(done) == len(tols):
            return done
        keep = min(KEEP_MAX, mm - 1)
        Vn = Y[:, :keep].T.astype(dtype) @ V[:mm]
        last = V[mm].copy()
        V[:keep] = Vn
        V[keep] = last
        T[:] = 0.0
        for i in range(keep):
            T[i, i] = theta[i]
            T[i, keep] = T[keep, i] = beta * Y[mm - 1, i]
        k = keep
        restart += 1


def dual_infeasibility(prob_or_path, lam, tol=1e-2, ncv=40, max_restarts=600, dtype=LD):
    """what lorads_hip_dual_infeasibility returns: (sum, per-block lambda_min (0 for an LP block), S x products, per-block result,
    the LP columns' shares |min(s_j, 0)| per LP block)"""
    tot, mins, nmv, results, lp = dtype(0), [], 0, [], {}
    for k, S in enumerate(slack(prob_or_path, lam, dtype)):
        if S.is_lp:
            share = np.abs(np.minimum(S.diagonal(), 0))
            lp[k] = share
            tot += share.sum()
            mins.append(0.0)
            results.append(None)
        else:
            r = lanczos(S, tol, ncv, max_restarts, dtype)
            tot += abs(min(r.theta, 0.0))
            mins.append(r.theta)
            nmv += r.matvecs
            results.append(r)
    return float(tot), mins, nmv, results, lp


def certificate(prob_or_path, R_per_cone, x_lp, lam, dtype=LD):
    """The certificate's sums at X_k = R_k R_k^T (SDP cones; R_per_cone[k], None on an LP block) and X = diag(x_lp[k]) (LP blocks;
    a dict or list indexed by block), each with the sum of the absolute values of its terms (`*_abs`): cx = <C, X>, sx = <S, X>,
    res = A(X) - b (with res_abs per constraint, |b_i| included), nrm2sq = ||res||_2^2, nrm2, ninf, binf = ||b||_inf,
    bl = b . lam, lp_min = {block: min_j s_j}."""
    p = problem(prob_or_path)
    m, b, dims, a = p["m"], p["b"], p["blocks"], p["_arr"]
    lam64 = np.asarray(lam, dtype=np.float64)
    lamd = lam64.astype(dtype)
    bd = b.astype(dtype)
    F = []
    for k, n in enumerate(dims):
        F.append(np.asarray(x_lp[k], dtype=np.float64).astype(dtype) if n < 0 else np.asarray(R_per_cone[k], dtype=np.float64).astype(dtype))
    mat, blk, ii, jj, vv = a["mat"], a["blk"], a["i"], a["j"], a["v"].astype(dtype)
    d = np.zeros(len(vv), dtype=dtype)  # <E_ij + E_ji (i != j) | E_ii, X>
    for k, n in enumerate(dims):
        sel = np.flatnonzero(blk == k)
        if not len(sel):
            continue
        if n < 0:
            d[sel] = F[k][ii[sel]]
        else:
            d[sel] = (F[k][ii[sel]] * F[k][jj[sel]]).sum(axis=1) * np.where(ii[sel] == jj[sel], 1.0, 2.0).astype(dtype)
    isc, isa = mat == 0, mat > 0
    tc = -vv[isc] * d[isc]
    ta = vv[isa] * d[isa]
    ax = np.zeros(m, dtype=dtype)
    ax_abs = np.zeros(m, dtype=dtype)
    np.add.at(ax, mat[isa] - 1, ta)
    np.add.at(ax_abs, mat[isa] - 1, np.abs(ta))
    ts = -lamd[mat[isa] - 1] * ta
    res = ax - bd
    out = dict(cx=tc.sum(), cx_abs=np.abs(tc).sum(), sx=tc.sum() + ts.sum(), sx_abs=np.abs(tc).sum() + np.abs(ts).sum(),
               res=res, res_abs=ax_abs + np.abs(bd), nrm2sq=(res * res).sum(), bl=(bd * lamd).sum(), bl_abs=np.abs(bd * lamd).sum(),
               ninf=np.abs(res).max() if m else dtype(0), binf=float(np.abs(b).max()) if m else 0.0)
    out["nrm2"] = np.sqrt(out["nrm2sq"])
    out["lp_min"] = {k: Sk.diagonal().min() for k, Sk in enumerate(slack(p, lam64, dtype)) if Sk.is_lp} if min(dims) < 0 else {}
    return out
