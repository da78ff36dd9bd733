"""Extended-precision model of phase 1 (the ALM warm start's inner iteration: gradient, L-BFGS direction, line-search sums, step,
history update), for comparisons over consecutive iterations of the device (tests/test_fixed_count_alm.py) and of the CPU oracle
(tests/test_alm_model_vs_oracle.py).

Plain numpy in np.longdouble, independent of the HIP library and of the oracle.  The data and the textbook operator are those of
tests/admm_model.py (AdmmModel: A_i(X Y^T) = <A_i, sym(X Y^T)> from the entries of A_i; the LP block as a diagonal cone of rank 1,
include/lorads_hip.h: lorads_hip_block.is_lp).  The steps follow the reference's inner loop (lorads_alm.c:1066-1131) slot for slot,
as include/lorads_hip.h cites them.  The history is a plain list of (s, y, beta), newest last: no ring and no head index, and no
summation order of any kernel is mirrored."""
import numpy as np

from tests.admm_model import LD, AdmmModel

QUANTITIES = ("p1", "p2", "a", "b", "c", "d", "D", "q1", "q2", "R", "Grad", "lagNormSq", "err1", "csum")


class AlmModel(AdmmModel):
    """State per context: R[k], Grad[k], D[k] (n x r per cone), lam, csum, q1, q2 and hist = [(s, y, beta), ...] over the
    concatenation of the cones, newest last.  dtype: np.longdouble (the model) or np.float64 (the same schedule in double: the spread
    between the two measures a case's conditioning)."""

    def __init__(self, m, b, dims, entries, dtype=LD, hist_len=2):
        super().__init__(m, b, dims, entries, dtype=dtype)
        self.L = int(hist_len)
        self.hist = []
        self.R = [None] * self.nb
        self.Grad = [None] * self.nb
        self.D = [None] * self.nb
        self.q1 = np.zeros(m, dtype=dtype)
        self.q2 = np.zeros(m, dtype=dtype)
        self.p1 = self.p2 = dtype(0)
        self.p1_mag = self.p2_mag = dtype(0)

    @classmethod
    def from_file(cls, path, dtype=LD, hist_len=2):
        from tests.admm_model import read_sdpa
        return cls(*read_sdpa(path), dtype=dtype, hist_len=hist_len)

    # ---- flat views (the L-BFGS vectors run over all cones, lorads_alm.c:230-260)
    def _flat(self, mats):
        return np.concatenate([x.ravel() for x in mats])

    def _unflat(self, v):
        out, pos = [], 0
        for r in self.R:
            out.append(v[pos:pos + r.size].reshape(r.shape).copy())
            pos += r.size
        return out

    # ---- state
    def set_r_state(self, R, lam):
        self.R = [np.asarray(r, dtype=np.float64).astype(self.dtype) for r in R]
        self.lam = np.asarray(lam, dtype=np.float64).astype(self.dtype)
        self.hist = []
        self.init_constr()

    def init_constr(self):
        """InitConstrValAll + InitConstrValSum (lorads_alg_common.c:78-84,134-142) on (R, R): csum = sum_k A_k(R_k R_k^T)"""
        self.csum = self.auv(self.R, self.R)

    def cal_grad(self, rho):
        """ALMCalGrad (lorads_alm.c:9-54): M1 = -lam - rho b + rho csum, Grad_k = 2 (C_k + sum_i M1_i A_ik) R_k; sum_k ||Grad_k||^2"""
        rho = self.dtype(rho)
        M1 = -self.lam - rho * self.b + rho * self.csum
        tot = self.dtype(0)
        for k, cn in enumerate(self.cones):
            S = np.zeros_like(self.R[k])
            self._apply_sym(cn.c_row, cn.c_col, cn.c_val, self.R[k], S)
            self._apply_sym(cn.a_row, cn.a_col, cn.a_val * M1[cn.a_con], self.R[k], S)
            self.Grad[k] = 2 * S
            tot += np.sum(self.Grad[k] * self.Grad[k])
        return tot

    def direction(self, inner):
        """LBFGSDirection + LBFGSDirectionUseGrad (lorads_alm.c:230-391,469-489): the two-loop recursion over the newest
        nn = inner if inner <= L - 1 else L pairs, then D = -Grad where <D, Grad> >= 0.
        Returns (cos(D, Grad) before the fallback, fallback taken)."""
        g = self._flat(self.Grad)
        if inner == 0:
            q = g.copy()
        else:
            nn = inner if inner <= self.L - 1 else self.L
            assert len(self.hist) >= nn, "the history holds fewer pairs than the reference's rule reads"
            pairs = self.hist[-nn:]
            q = g.copy()
            alpha = [None] * nn
            for t in range(nn - 1, -1, -1):  # newest -> oldest
                s, y, beta = pairs[t]
                alpha[t] = beta * np.sum(s * q)
                q = q - alpha[t] * y
            for t in range(nn):  # oldest -> newest
                s, y, beta = pairs[t]
                q = q + (alpha[t] - beta * np.sum(y * q)) * s
        d = -q
        ip = np.sum(d * g)
        cos = float(ip / np.sqrt(np.sum(d * d) * np.sum(g * g)))
        taken = bool(ip >= 0)
        if taken:
            d = -g
        self.D = self._unflat(d)
        return cos, taken

    def _obj_pair(self, X, Y):
        """(<C, sym(X Y^T)>, the sum of the magnitudes of its terms) over the cones"""
        v = mag = self.dtype(0)
        for k, cn in enumerate(self.cones):
            if len(cn.c_val):
                t = cn.c_val * self._pair_dots(X[k], Y[k], cn.c_row, cn.c_col)
                v += np.sum(t)
                mag += np.sum(np.abs(t))
        return v, mag

    def q12p12(self):
        """ALMCalq12p12 (lorads_alm.c:540-560): q1 = 2 A(sym(R D^T)), q2 = A(D D^T), p1 = 2 <C, sym(R D^T)>, p2 = <C, D D^T>"""
        self.q1 = 2 * self.auv(self.R, self.D)
        self.q2 = self.auv(self.D, self.D)
        p1, m1 = self._obj_pair(self.R, self.D)
        self.p1, self.p1_mag = 2 * p1, 2 * m1
        self.p2, self.p2_mag = self._obj_pair(self.D, self.D)
        return self.p1, self.p2

    def linesearch_coeffs(self, rho):
        """the m-vector half of ALMLineSearch (lorads_alm.c:161-172, oracle/lorads_oracle.c:314-340): q0 = b - csum + lam / rho,
        a = rho ||q2||^2 / 2, b = rho q1.q2, c = p2 - rho q0.q2 + rho ||q1||^2 / 2, d = p1 - rho q0.q1.
        Returns ((a, b, c, d), the sum of the magnitudes of each one's terms): c and d cancel."""
        rho = self.dtype(rho)
        q0 = self.b - self.csum + self.lam / rho
        q1, q2 = self.q1, self.q2
        coef = (rho * np.sum(q2 * q2) / 2, rho * np.sum(q1 * q2), self.p2 - rho * np.sum(q0 * q2) + rho * np.sum(q1 * q1) / 2,
                self.p1 - rho * np.sum(q0 * q1))
        mags = (rho * np.sum(q2 * q2) / 2, rho * np.sum(np.abs(q1 * q2)),
                self.p2_mag + rho * np.sum(np.abs(q0 * q2)) + rho * np.sum(q1 * q1) / 2, self.p1_mag + rho * np.sum(np.abs(q0 * q1)))
        return coef, mags

    def step(self, tau, rho):
        """setAsNegGrad, ALMupdateVar + the constraint sums' recurrence, ALMCalGrad, setlbfgsHisTwo, updateDimacsALM
        (lorads_alm.c:583-598, 619-648 and 1122-1124, 9-54, 657-678; lorads_alg_common.c:250-290).
        Returns (lagNormSq, err1).  csum_rec keeps the constraint sums by recurrence (what the gradient saw); csum is left as
        update_dimacs leaves it, A(R R^T) formed anew."""
        tau = self.dtype(tau)
        ynew = -self._flat(self.Grad)
        self.R = [r + tau * d for r, d in zip(self.R, self.D)]
        self.csum = self.csum + tau * self.q1 + tau * tau * self.q2
        self.csum_rec = self.csum
        lag = self.cal_grad(rho)
        s = tau * self._flat(self.D)
        y = ynew + self._flat(self.Grad)
        self.hist.append((s, y, 1 / np.sum(y * s)))
        self.hist = self.hist[-self.L:]
        self.csum = self.auv(self.R, self.R)
        vio = self.b - self.csum
        err1 = np.sqrt(np.sum(vio * vio)) / (1 + self.dtype(self.bnrm1))
        return lag, err1

    def pair_cos(self):
        """cos(y, s) of the newest stored pair"""
        s, y, _ = self.hist[-1]
        return float(np.sum(y * s) / np.sqrt(np.sum(y * y) * np.sum(s * s)))


def descent_tau(coef, frac=0.5):
    """A step that stores a pair with y.s < 0: y.s = tau^2 (4 a tau^2 + 3 b tau + 2 c), negative inside the roots of the quadratic
    (real when 9 b^2 > 32 a c, e.g. c < 0).  Returns frac times the larger root, or None."""
    a, b, c, _ = [float(x) for x in coef]
    disc = 9 * b * b - 32 * a * c
    if disc <= 0 or a <= 0:
        return None
    hi = (-3 * b + np.sqrt(disc)) / (8 * a)
    return frac * hi if hi > 0 else None


def run_schedule(path, R, lam, rho, iters, hist_len, tau_of, dtype=LD, taus=None):
    """`iters` consecutive inner iterations from (R, lam) without any resync.  tau_of(i, coef) gives the step of iteration i from the
    model's coefficients (floats); `taus` replays a recorded schedule instead.  Returns a list of records, one per iteration:
    the QUANTITIES after the iteration's front (p1 .. q2 of iteration i) and after its step (R .. csum), the term magnitudes of
    p1, p2, a, b, c, d, tau, cos(D, Grad) before the fallback, whether it was taken and cos(y, s) of the pair the step stored;
    record 0 also holds lagNormSq of the starting point (lag0)."""
    mdl = AlmModel.from_file(path, dtype=dtype, hist_len=hist_len)
    mdl.set_r_state(R, lam)
    lag0 = mdl.cal_grad(rho)
    recs = []
    for i in range(iters):
        cos, taken = mdl.direction(i)
        p1, p2 = mdl.q12p12()
        coef, mags = mdl.linesearch_coeffs(rho)
        tau = taus[i] if taus is not None else tau_of(i, [float(x) for x in coef])
        rec = dict(p1=p1, p2=p2, a=coef[0], b=coef[1], c=coef[2], d=coef[3], D=[x.copy() for x in mdl.D], q1=mdl.q1.copy(),
                   q2=mdl.q2.copy(), mags=dict(p1=mdl.p1_mag, p2=mdl.p2_mag, a=mags[0], b=mags[1], c=mags[2], d=mags[3]),
                   tau=float(tau), cos_dg=cos, fallback=taken, grad_before=[g.copy() for g in mdl.Grad])
        lag, err1 = mdl.step(tau, rho)
        rec.update(R=[x.copy() for x in mdl.R], Grad=[x.copy() for x in mdl.Grad], lagNormSq=lag, err1=err1, csum=mdl.csum.copy(),
                   csum_rec=mdl.csum_rec.copy(), cos_ys=mdl.pair_cos())
        if i == 0:
            rec["lag0"] = lag0
        recs.append(rec)
    return recs, mdl


def _rel(got, want, scale=None):
    got = np.asarray(got, dtype=LD).ravel()
    want = np.asarray(want, dtype=LD).ravel()
    sc = float(np.max(np.abs(want))) if scale is None else float(scale)
    return float(np.max(np.abs(got - want))) / max(sc, 1e-300) if want.size else 0.0


def record_errors(got, want):
    """worst rel-to-scale difference of a record `got` (any subset of the QUANTITIES) from the model's record `want`, by group:
    coefficients (p1, p2, a .. d: to the magnitudes of their terms), factors (D, R, Grad: to the matrix's largest entry), vectors
    (q1, q2, csum: to the vector's largest entry), scalars (lagNormSq, err1: to themselves)"""
    out = dict(coefficients=0.0, factors=0.0, vectors=0.0, scalars=0.0)
    for key in ("p1", "p2", "a", "b", "c", "d"):
        if key in got:
            out["coefficients"] = max(out["coefficients"], _rel(got[key], want[key], want["mags"][key]))
    for key in ("D", "R", "Grad"):
        if key in got:
            for g, w in zip(got[key], want[key]):
                out["factors"] = max(out["factors"], _rel(g, w))
    for key in ("q1", "q2", "csum"):
        if key in got:
            out["vectors"] = max(out["vectors"], _rel(got[key], want[key]))
    for key in ("lagNormSq", "err1", "lag0"):
        if key in got:
            out["scalars"] = max(out["scalars"], _rel(got[key], want[key]))
    return out


def conditioning(recs_ld, recs_64):
    """e64(i): the worst rel-to-scale difference over all compared quantities at iteration i between the float64 and the longdouble
    run of the model on the same tau schedule"""
    return [max(record_errors(r64, rld).values()) for rld, r64 in zip(recs_ld, recs_64)]


BOUND_FACTOR, BOUND_FLOOR, BOUND_CEILING, E64_CUT, MIN_COS = 32.0, 1e-14, 1e-11, 3e-13, 0.05


def plan(path, R, lam, rho, iters, hist_len, tau_of, min_iters=4):
    """The model's side of a case: the longdouble records, the iterations to compare (those before the first with e64 > 3e-13), the
    bound max(32 max e64, 1e-14) <= 1e-11 and the checks that no compared iteration sits near a branch point
    (|cos(D, Grad)| >= 0.05 before the fallback, |cos(y, s)| >= 0.05 for every stored pair).
    Returns (records cut to the compared iterations, e64 per iteration, bound, the model after the schedule: its operator)."""
    recs, mdl = run_schedule(path, R, lam, rho, iters, hist_len, tau_of)
    taus = [r["tau"] for r in recs]
    recs64, _ = run_schedule(path, R, lam, rho, iters, hist_len, None, dtype=np.float64, taus=taus)
    e64 = conditioning(recs, recs64)
    n = next((i for i, e in enumerate(e64) if e > E64_CUT), len(e64))
    assert n >= min(min_iters, iters), ("the case's conditioning leaves fewer iterations than it must compare", n, e64)
    for i, r in enumerate(recs[:n]):
        assert i == 0 or abs(r["cos_dg"]) >= MIN_COS, ("iteration near the fallback's branch point", i, r["cos_dg"])
        assert abs(r["cos_ys"]) >= MIN_COS, ("stored pair near y.s = 0", i, r["cos_ys"])
    bound = min(max(BOUND_FACTOR * max(e64[:n]), BOUND_FLOOR), BOUND_CEILING)
    return recs[:n], e64, bound, mdl
