"""Extended-precision model of the ADMM sweep, for fixed-count comparisons of the device (tests/test_fixed_count_sweeps.py) and of
the CPU oracle (tests/test_admm_model_vs_oracle.py).

Plain numpy in np.longdouble (80-bit on x86 hosts), independent of the HIP library and of the oracle.  The operator is written in its
textbook form, not in any kernel's form:

    A_i(U V^T)  = <A_i, sym(U V^T)>, from the entries of A_i (an off-diagonal entry counts twice)
    CG operator = x + sum_i <A_i, sym(x V^T)> A_i V

and the sweep follows the reference step for step: the right-hand side of LORADSUpdateSDPVarOne (lorads_admm.c:428-480), CGSolve
(lorads_cgs.c:81-240, as oracle/lorads_oracle.c:453-492 restates it: start from the current factor, restart with the true residual
when k % 20 == 0 -- k = 0 included --, stop on ||r||_2 / ||b||_1 < tol or at maxit), cones in sequence with U then V and the running
constraint sum, the LP block column by column in closed form (lorads_admm.c:595-629), the dual update and the evaluation of the fused
step (pObj, dObj, DIMACS error 1).  The data are what the host hands to the operator table: C = -F0, entries below 1e-12 dropped,
lower triangle, LP entries keyed by their row.  No summation order of any device kernel is mirrored."""
import re

import numpy as np

LD = np.longdouble


def read_sdpa(path):
    """(m, b, dims, entries) of a .dat-s file; entries: list of (mat, blk, i, j, v), 1-based as in the file"""
    with open(path) as f:
        lines = [ln for ln in f if ln.strip() and ln.lstrip()[0] not in "*\""]
    tok = lambda s: [t for t in re.split(r"[\s,{}()]+", s) if t]  # noqa: E731
    m = int(tok(lines[0])[0])
    nblk = int(tok(lines[1])[0])
    dims = [int(x) for x in tok(lines[2])[:nblk]]
    pos, b = 3, []
    while len(b) < m:
        b += [float(x) for x in tok(lines[pos])]
        pos += 1
    ent = []
    for ln in lines[pos:]:
        t = tok(ln)
        if len(t) >= 5:
            ent.append((int(t[0]), int(t[1]), int(t[2]), int(t[3]), float(t[4])))
    return m, b, dims, ent


class _Cone:
    """one cone: C and the A_i as lower-triangular entry lists, duplicates summed"""

    def __init__(self, n, is_lp, cent, aent, dtype):
        self.n, self.is_lp = n, is_lp
        self.c_row, self.c_col, self.c_val = self._arrays(cent, dtype)
        con = sorted(aent)
        self.a_con = np.array([k[0] for k in con], dtype=np.int64)
        self.a_row = np.array([k[1] for k in con], dtype=np.int64)
        self.a_col = np.array([k[2] for k in con], dtype=np.int64)
        self.a_val = np.array([aent[k] for k in con], dtype=dtype)
        self.cons = np.unique(self.a_con)

    @staticmethod
    def _arrays(d, dtype):
        keys = sorted(d)
        return (np.array([k[0] for k in keys], dtype=np.int64), np.array([k[1] for k in keys], dtype=np.int64),
                np.array([d[k] for k in keys], dtype=dtype))


class AdmmModel:
    """State: U[k], V[k] (n x r), lam, csum (sum over cones of A(U V^T)), cv[k] (cone k's share of csum).
    dtype: np.longdouble (the model) or np.float64 (to measure a case's conditioning by the spread between the two)."""

    def __init__(self, m, b, dims, entries, dtype=LD):
        self.dtype = dtype
        self.m = m
        self.b = np.asarray(b, dtype=np.float64).astype(dtype)
        self.bnrm1 = sum(abs(float(x)) for x in b)
        cents = [dict() for _ in dims]
        aents = [dict() for _ in dims]
        for mat, blk, i, j, v in entries:
            if abs(v) < 1e-12:
                continue
            k = blk - 1
            r, c = i - 1, j - 1
            if dims[k] < 0:
                c = r  # (the reference keys LP entries by their row index only)
            r, c = max(r, c), min(r, c)
            if mat == 0:
                cents[k][(r, c)] = cents[k].get((r, c), 0.0) + (-v)  # C = -F0
            else:
                key = (mat - 1, r, c)
                aents[k][key] = aents[k].get(key, 0.0) + v
        self.cones = [_Cone(abs(n), n < 0, cents[k], aents[k], dtype) for k, n in enumerate(dims)]
        self.nb = len(self.cones)
        self.U = [None] * self.nb
        self.V = [None] * self.nb
        self.lam = np.zeros(m, dtype=dtype)
        self.csum = np.zeros(m, dtype=dtype)
        self.cv = [np.zeros(m, dtype=dtype) for _ in range(self.nb)]

    @classmethod
    def from_file(cls, path, dtype=LD):
        return cls(*read_sdpa(path), dtype=dtype)

    # ---- the operator in textbook form
    def _pair_dots(self, X, Y, rows, cols):
        """sym(X Y^T) at (row, col) times 2 off the diagonal: X_row . Y_col + X_col . Y_row  (X_row . Y_row on it)"""
        d = np.sum(X[rows] * Y[cols], axis=1)
        off = rows != cols
        d[off] += np.sum(X[cols[off]] * Y[rows[off]], axis=1)
        return d

    def cone_auv(self, k, X, Y):
        """m-vector of <A_i, sym(X Y^T)> over the constraints of cone k"""
        cn = self.cones[k]
        out = np.zeros(self.m, dtype=self.dtype)
        if len(cn.a_val):
            np.add.at(out, cn.a_con, cn.a_val * self._pair_dots(X, Y, cn.a_row, cn.a_col))
        return out

    def auv(self, X, Y):
        """sum over the cones of A(sym(X_k Y_k^T)); X, Y: lists per cone"""
        out = np.zeros(self.m, dtype=self.dtype)
        for k in range(self.nb):
            out += self.cone_auv(k, X[k], Y[k])
        return out

    def _apply_sym(self, rows, cols, coef, Y, out):
        """out += S Y with S = sum_e coef_e (E_row,col + E_col,row) (E_row,row on the diagonal)"""
        np.add.at(out, rows, coef[:, None] * Y[cols])
        off = rows != cols
        np.add.at(out, cols[off], coef[off][:, None] * Y[rows[off]])

    def cg_operator(self, k, x, F):
        """x + sum_i <A_i, sym(x F^T)> A_i F"""
        cn = self.cones[k]
        w = self.cone_auv(k, x, F)
        out = np.array(x, dtype=self.dtype, copy=True)
        self._apply_sym(cn.a_row, cn.a_col, cn.a_val * w[cn.a_con], F, out)
        return out

    # ---- one factor update (LORADSUpdateSDPVarOne) and CGSolve
    def rhs(self, k, F, rho):
        cn = self.cones[k]
        M1 = rho * (self.csum - self.cv[k] - self.b) - self.lam
        SF = np.zeros_like(F)
        self._apply_sym(cn.c_row, cn.c_col, cn.c_val, F, SF)
        self._apply_sym(cn.a_row, cn.a_col, cn.a_val * M1[cn.a_con], F, SF)
        return -(SF - rho * F) / rho

    def cg(self, k, F, x, b, tol, maxit):
        """CGSolve from x (updated in place).  Returns (iterations, residual history): history[0] is the initial ||r||/||b||_1,
        history[j] the value after iteration j (before a restart replaces the residual)."""
        bn = np.sum(np.abs(b))
        r = b - self.cg_operator(k, x, F)
        rel = np.sqrt(np.sum(r * r)) / bn
        hist = [float(rel)]
        if rel < tol:
            return 0, hist
        p = r.copy()
        it = 0
        for kk in range(maxit):
            it += 1
            Q = self.cg_operator(k, p, F)
            rr = np.sum(r * r)
            alpha = rr / np.sum(p * Q)
            x += alpha * p
            r = r - alpha * Q
            rel = np.sqrt(np.sum(r * r)) / bn
            hist.append(float(rel))
            if rel < tol:
                break
            if kk % 20 == 0:  # restart with the true residual; the direction below is then 2 r (beta = 1, p = r)
                r = b - self.cg_operator(k, x, F)
                p = r.copy()
                rr = np.sum(r * r)
            rrn = np.sum(r * r)
            p = (rrn / rr) * p + r
        return it, hist

    # ---- the LP block: closed form per column (lorads_admm.c:595-629) with the bookkeeping of lorads_alg_common.c:236-246
    def _lp_sweep(self, k, rho):
        cn = self.cones[k]
        U, V = self.U[k], self.V[k]
        cidx = {int(rw): t for t, rw in enumerate(cn.c_row)}
        xs = self.lp_x[k]
        for col in range(cn.n):
            sel = np.nonzero(cn.a_row == col)[0]
            g, a = cn.a_con[sel], cn.a_val[sel]
            nrm2sq = np.sum(a * a)
            for upd, fixed in ((U, V), (V, U)):
                old = xs[col]  # the product behind the column's stored constraint values (u v, or r^2 after an evaluation)
                w = cn.c_val[cidx[col]] if col in cidx else self.dtype(0)
                w = w + np.sum(a * (rho * (self.csum[g] - self.b[g] - a * old) - self.lam[g]))
                f = fixed[col, 0]
                upd[col, 0] = -(w * f - rho * f) / rho / (1 + nrm2sq * f * f)
                xs[col] = new = U[col, 0] * V[col, 0]
                self.csum[g] += a * (new - old)
                self.cv[k][g] += a * (new - old)

    # ---- state
    def set_state(self, U, V, lam):
        self.U = [np.asarray(u, dtype=np.float64).astype(self.dtype) for u in U]
        self.V = [np.asarray(v, dtype=np.float64).astype(self.dtype) for v in V]
        self.lam = np.asarray(lam, dtype=np.float64).astype(self.dtype)
        self.init_constr()

    def init_constr(self):
        self.lp_x = [u[:, 0] * v[:, 0] if cn.is_lp else None for cn, u, v in zip(self.cones, self.U, self.V)]
        self.cv = [self.cone_auv(k, self.U[k], self.V[k]) for k in range(self.nb)]
        self.csum = np.sum(self.cv, axis=0) if self.nb else np.zeros(self.m, dtype=self.dtype)

    def scale_obj(self, s):
        """objScale_dualvar (data/lorads_solver.c:1040-1052): C and the multipliers times s; factors and constraint sums stay"""
        s = self.dtype(s)
        for cn in self.cones:
            cn.c_val = cn.c_val * s
        self.lam = self.lam * s

    def sweep(self, rho, tol, maxit):
        """admm_update_var: returns (CG iterations over all solves, [(cone, half, iterations, history), ...])"""
        rho = self.dtype(rho)
        tot, log = 0, []
        for k, cn in enumerate(self.cones):
            if cn.is_lp:
                self._lp_sweep(k, rho)
                continue
            for half in range(2):
                x, F = (self.U[k], self.V[k]) if half == 0 else (self.V[k], self.U[k])
                it, hist = self.cg(k, F, x, self.rhs(k, F, rho), tol, maxit)
                tot += it
                log.append((k, half, it, hist))
                self.csum -= self.cv[k]
                self.cv[k] = self.cone_auv(k, self.U[k], self.V[k])
                self.csum += self.cv[k]
        return tot, log

    def update_dual(self, rho):
        self.lam = self.lam + self.dtype(rho) * (self.b - self.csum)

    def evaluate(self):
        """cal_obj(UV) + cal_dual_obj + update_dimacs(UV): (pObj, dObj, err1); leaves csum = A(R R^T), R = (U + V) / 2"""
        R = [(u + v) / 2 for u, v in zip(self.U, self.V)]
        pobj = self.dtype(0)
        for k, cn in enumerate(self.cones):
            if len(cn.c_val):
                pobj += np.sum(cn.c_val * self._pair_dots(R[k], R[k], cn.c_row, cn.c_col))
        dobj = np.sum(self.b * self.lam)
        self.lp_x = [r[:, 0] * r[:, 0] if cn.is_lp else None for cn, r in zip(self.cones, R)]
        self.cv = [self.cone_auv(k, R[k], R[k]) for k in range(self.nb)]
        self.csum = np.sum(self.cv, axis=0)
        vio = self.b - self.csum
        err1 = np.sqrt(np.sum(vio * vio)) / (1 + self.dtype(self.bnrm1))
        return pobj, dobj, err1

    def step(self, rho, tol, maxit):
        """admm_step: (CG iterations, pObj, dObj, err1, solve log)"""
        its, log = self.sweep(rho, tol, maxit)
        p, d, e = self.evaluate()
        return its, p, d, e, log


def stopping_tol(model, rho, js, maxit, ratio=1.5, margin=1.05, probe_maxit=None):
    """A tolerance that stops some solve of the next sweep after exactly j iterations, for the first j of `js` that has one: the
    geometric mean of that solve's smallest residual before iteration j and its residual after iteration j, taken only where they
    differ by >= `ratio` (CG residuals need not decrease).  Checked on a copy of the model over the whole sweep: no solve may have a
    residual within a factor `margin` of it before it stops (rounding cannot then move a stop), and no solve may pass on its initial
    residual.  probe_maxit: the model's sweeps run at most that many iterations per solve, whatever `maxit` is, and EVERY solve must
    stop by the tolerance before them -- the tolerance then holds for any iteration limit from probe_maxit on (a limit of thousands,
    which no solve may come near).  Returns (tol, j, index of that solve in the sweep), or None when no such tolerance exists."""
    import copy
    run = maxit if probe_maxit is None else min(maxit, probe_maxit)
    probe = copy.deepcopy(model)
    _, log = probe.sweep(rho, 0.0, run)
    for j in js:
        for idx, (_, _, _, hist) in enumerate(log):
            if len(hist) <= j or min(hist[:j]) < ratio * hist[j]:
                continue
            tol = float(np.sqrt(min(hist[:j]) * hist[j]))
            probe = copy.deepcopy(model)
            _, log2 = probe.sweep(rho, tol, run)
            if len(log2) > idx and log2[idx][2] == j and all(
                    h[0] >= tol and not any(tol / margin < x < tol * margin for x in h) for _, _, _, h in log2) and (
                    probe_maxit is None or all(h[-1] < tol for _, _, _, h in log2)):
                return tol, j, idx
    return None
