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
lower triangle, LP entries keyed by their row.  No summation order of any device kernel is mirrored.

A sweep's count is the reference's too: a solve that passes on its initial residual adds its cone's stale count (DESIGN.md section 5,
Q7; run_stage).  stopping_tol finds tolerances at which no solve does that, pattern_tol tolerances at which chosen solves do, and
solved_state the factors from which they do (tests/test_immediate_exits.py)."""
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
    """State: U[k], V[k] (n x r), lam, csum (sum over cones of A(U V^T)), cv[k] (cone k's share of csum), cg_last[k] (the count of
    cone k's latest solve that iterated: what a solve that passes on its initial residual adds to a sweep's total, see sweep).
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
        self.cg_last = [0] * self.nb  # (CGSolverCreate / CGSolverClear: iter = 0, lorads_cgs.c:27,54)

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

    def as_dtype(self, dtype):
        """a copy of the model and its state in another number format (data, factors, multipliers and constraint sums rounded)"""
        import copy
        other = copy.deepcopy(self)
        other.dtype = dtype
        for cn in other.cones:
            cn.c_val, cn.a_val = cn.c_val.astype(dtype), cn.a_val.astype(dtype)
        conv = lambda xs: [None if x is None else x.astype(dtype) for x in xs]  # noqa: E731
        other.U, other.V, other.cv, other.lp_x = conv(other.U), conv(other.V), conv(other.cv), conv(other.lp_x)
        other.b, other.lam, other.csum = other.b.astype(dtype), other.lam.astype(dtype), other.csum.astype(dtype)
        return other

    def init_constr(self):
        self.lp_x =[u[:, 0] * v[:, 0] if cn.is_lp else None for cn, u, v in zip(self.cones, self.U, self.V)]
        self.cv = [self.cone_auv(k, self.U[k], self.V[k]) for k in range(self.nb)]
        self.csum = np.sum(self.cv, axis=0) if self.nb else np.zeros(self.m, dtype=self.dtype)

    def scale_obj(self, s):
        """objScale_dualvar (data/lorads_solver.c:1040-1052): C and the multipliers times s; factors and constraint sums stay"""
        s = self.dtype(s)
        for cn in self.cones:
            cn.c_val = cn.c_val * s
        self.lam = self.lam * s

    def stages(self):
        """the sweep's stages in order: (cone, half) per CG solve, (cone, None) for the LP block"""
        out = []
        for k, cn in enumerate(self.cones):
            out += [(k, None)] if cn.is_lp else [(k, 0), (k, 1)]
        return out

    def run_stage(self, k, half, rho, tol, maxit):
        """one stage of the sweep.  A solve returns (iterations, history, count added to the sweep's total); the LP block None.

        The count is the reference's, not the solve's: every cone has one CGLinsys whose `iter` CGSolve sets to 0 only behind
        the test of the initial residual (lorads_cgs.c:157-160 return before line 173), and LORADSUpdateSDPVarOne adds that field
        to cgIter after every solve (lorads_admm.c:477,532).  A solve that passes on its initial residual therefore adds the count
        of the cone's latest solve that iterated -- of its U- or its V-solve, whichever came last; 0 before the first -- and leaves
        it as it is.  The LP columns are closed forms without a CGLinsys (lorads_admm.c:595-629) and add nothing."""
        rho = self.dtype(rho)
        if half is None:
            self._lp_sweep(k, rho)
            return None
        x, F = (self.U[k], self.V[k]) if half == 0 else (self.V[k], self.U[k])
        it, hist = self.cg(k, F, x, self.rhs(k, F, rho), tol, maxit)
        if not passed_at_once(it, hist, tol):
            self.cg_last[k] = it
        self.csum -= self.cv[k]
        self.cv[k] = self.cone_auv(k, self.U[k], self.V[k])
        self.csum += self.cv[k]
        return it, hist, self.cg_last[k]

    def sweep(self, rho, tol, maxit):
        """admm_update_var: returns (the reference's CG count of the sweep, [(cone, half, iterations, history), ...]).  The log
        holds what each solve did (0 iterations for one that passed on its initial residual); the count is cgIter's increment,
        which for such a solve is the cone's stale count (see run_stage)."""
        tot, log = 0, []
        for k, half in self.stages():
            res = self.run_stage(k, half, rho, tol, maxit)
            if res is not None:
                tot += res[2]
                log.append((k, half, res[0], res[1]))
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


def passed_at_once(it, hist, tol):
    """did the solve with this count and residual history leave on its initial residual (CGSolve's first exit)?"""
    return it == 0 and hist[0] < tol


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


RUN = "run"


def _pattern_shown(model, rho, tol, maxit, pattern, stop, margin, clear):
    """the per-solve counts of the model's next sweep at `tol` if it shows the pattern with the margins of pattern_tol, else None"""
    import copy
    _, log = copy.deepcopy(model).sweep(rho, tol, maxit)
    _, log64 = model.as_dtype(np.float64).sweep(rho, tol, maxit)
    if len(log) != len(pattern) or [e[2] for e in log64] != [e[2] for e in log]:
        return None
    for want, (_, _, it, h), (_, _, _, h64) in zip(pattern, log, log64):
        gone = passed_at_once(it, h, tol)
        if any(tol / margin < x < tol * margin for x in h + h64) or (gone and not h[0] + clear * abs(h64[0] - h[0]) < tol / margin):
            return None
        if want is None:
            continue
        if (want == 0) != gone or (want != 0 and it < 1) or (want not in (0, RUN) and not (it == want and h[-1] < tol)):
            return None
    if stop is not None and not any(w == RUN and it == stop and h[-1] < tol for w, (_, _, it, h) in zip(pattern, log)):
        return None
    return tuple(e[2] for e in log)


def pattern_tol(model, rho, maxit, pattern, stop=None, margin=1.05, clear=100.0, top=1.0, budget=120):
    """A tolerance below `top` at which the model's next sweep shows a wanted pattern of immediate exits, or None.

    pattern: one entry per CG solve of the sweep, in sweep order (cone by cone, U then V; the LP block has none): 0 -- the solve
    passes on its initial residual and does nothing; RUN -- it iterates at least once; an integer j >= 1 -- the tolerance stops it
    after exactly j iterations; None -- whatever the model says.  stop: some solve marked RUN is stopped by the tolerance after
    exactly that many iterations.

    Conditions, all decided by the model alone (the same kind as stopping_tol's): the sweep at the returned tolerance shows exactly
    that pattern; no residual of any history lies within the factor `margin` of the tolerance; the model in float64 -- the format
    the device forms its residuals in -- runs the same counts with the same margin; and every solve that passes still passes, by
    that margin, with `clear` times the distance between the two formats' initial residuals added to its own.  Where a solve starts
    at its solution (solved_state) its residual is rounding alone -- some 1e-18 ||b||_1 in the model, 1e-16 in float64 and on the
    device, which sums in another order again -- and the condition reads: the float64 residual is below tol / `clear`.  Where the
    residual is a property of the state (a V-solve that passes at 0.06 under a tolerance of 0.1 while a U-solve iterates), the
    two formats agree to 1e-16 and the margin decides, as for every other residual.  Returns (tol, counts per solve).

    The search walks the sweep solve by solve and keeps the interval of tolerances that is still open: a solve's residual history
    (at tolerance 0, from the state the earlier solves leave) splits it into "passes at once", "stops after j" for every j, and
    "runs to maxit"; each admissible part is followed depth first, at most `budget` solves in all."""
    import copy
    stages = model.stages()
    left = [budget]

    def walk(mdl, si, pi, lo, hi, have):
        while si < len(stages) and stages[si][1] is None:
            mdl.run_stage(stages[si][0], None, rho, 0.0, maxit)
            si += 1
        if si == len(stages):
            if stop is not None and not have:
                return None
            tol = float(np.sqrt(lo * hi)) if lo > 0 else hi / 2
            counts = _pattern_shown(model, rho, tol, maxit, pattern, stop, margin, clear)
            return None if counts is None else (tol, counts)
        if left[0] <= 0:
            return None
        left[0] -= 1
        k, half = stages[si]
        want = pattern[pi]
        _, h, _ = copy.deepcopy(mdl).run_stage(k, half, rho, 0.0, maxit)
        parts = []  # (iterations to run: None = passes at once, lo, hi, stops at the wanted `stop`)
        if want in (0, None):
            parts.append((None, max(lo, h[0] * margin), hi, False))
        if want != 0:
            for j in range(1, len(h)):
                if want in (RUN, None, j):
                    parts.append((j, max(lo, h[j] * margin), min(hi, min(h[:j]) / margin), want == RUN and j == stop))
            if want in (RUN, None) and len(h) > 1:
                parts.append((len(h) - 1, lo, min(hi, min(h) / margin), False))
        parts = [p for p in parts if p[1] < p[2]]
        parts.sort(key=lambda p: not (p[3] and not have))  # (stable: the wanted stop first while none is taken)
        for j, plo, phi, st in parts:
            nxt = copy.deepcopy(mdl)
            nxt.run_stage(k, half, rho, np.inf if j is None else 0.0, j or 0)
            found = walk(nxt, si + 1, pi + 1, plo, phi, have or st)
            if found:
                return found
        return None

    return walk(copy.deepcopy(model), 0, 0, 0.0, float(top), False)


def solved_state(model, rho, cones=None, half=0, iters=200):
    """(U, V) in float64 with the chosen cones' U (half 0; 1: V) replaced by the converged solve for the other factor as the model
    holds it: the model's cg at tolerance 0 over `iters` iterations, cone by cone in sweep order (a later cone's right-hand side
    sees the constraint values of an earlier cone's solution), rounded to float64.  cones: None = every cone with a CG.  In a sweep
    from the returned state such a solve starts at its solution (initial residual near 1e-16 ||b||_1 in double) as long as no
    earlier solve of the sweep has moved what its right-hand side reads; the model decides that (pattern_tol)."""
    import copy
    probe = copy.deepcopy(model)
    for k, h in probe.stages():
        if h is not None and h == half and (cones is None or k in cones):
            probe.run_stage(k, half, rho, 0.0, iters)
    U = [np.asarray(u, dtype=np.float64) for u in probe.U]
    V = [np.asarray(v, dtype=np.float64) for v in probe.V]
    assert all(np.all(np.isfinite(x)) for x in U + V)
    return U, V


def lp_levels(model, k):
    """column counts per level of LP block k's level schedule, from the model's data: level(j) = 1 + the largest level among the
    earlier columns that share a constraint row with j (columns of one level do not see each other; a column without an entry
    is in level 0)"""
    cn = model.cones[k]
    row_lvl, sizes = {}, []
    for col in range(cn.n):
        rows = [int(g) for g in cn.a_con[cn.a_row == col]]
        lvl = max([row_lvl.get(g, 0) for g in rows], default=0)
        for g in rows:
            row_lvl[g] = lvl + 1
        sizes += [0] * (lvl + 1 - len(sizes))
        sizes[lvl] += 1
    return sizes
