"""The extended-precision ADMM model (tests/admm_model.py) against the CPU oracle, which is itself pinned to the compiled reference
(tests/test_oracle_vs_reference.py): this proves the model's conventions -- data transformations, right-hand side, CG restarts and
stopping rule, the LP columns, the dual update, the step's scalars -- before the device is held to it
(tests/test_fixed_count_sweeps.py).  Fixed-count sweeps leave no iteration count or tolerance to absorb an error.

The second half does the same for solves that pass on their initial residual (CGSolve's first exit) and for the count the
reference returns for them, before tests/test_immediate_exits.py holds the device to it."""
import os

import numpy as np
import pytest

from lorads_amd import host
from tests import common
from tests.admm_model import RUN, AdmmModel, lp_levels, passed_at_once, pattern_tol, solved_state, stopping_tol
from tests.test_hip_parity import TRACE_NAMES


RHO = 1.5
BOUND = 1e-13
# the two cones of the dense branch (dense objective) past the k = 20 restart, where the CG amplifies rounding most: the float64
# oracle sits 7.5e-13 (theta30, factors) and 3.4e-13 (densec40, constraint sums) from the longdouble model; 1e-13 everywhere else
BOUNDS = {"theta30": 2e-12, "densec40": 1e-12}


@pytest.mark.parametrize("name", TRACE_NAMES)
def test_fixed_count_sweeps_of_the_model_equal_the_oracle(oracle_lib, name):
    path = common.instance_path(name)
    BOUND = BOUNDS.get(name, globals()["BOUND"])
    s = common.oracle_session(path)
    try:
        model = AdmmModel.from_file(path)
        U, V, lam = common.random_uv_state(s, 11)
        common.load_uv_state(s.be, U, V, lam)
        model.set_state(U, V, lam)
        assert common.rel_to_scale(s.be.get_vec(host.VEC_CONSTR_SUM), model.csum) <= BOUND
        worst = 0.0
        # K = 1, 2, 22 with tol 0 (22 runs past the k = 20 restart: iteration 22 starts from it), the second as a fused step,
        # then one sweep stopped by a tolerance
        sched = [("sweep", 1, 0.0), ("step", 2, 0.0), ("sweep", 22, 0.0)]
        for i, (kind, maxit, tol) in enumerate(sched + [("step", 25, None)]):
            if tol is None:
                found = stopping_tol(model, RHO, (3, 4, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 1), maxit) or \
                    stopping_tol(model, RHO, (3, 4, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 1), maxit, ratio=1.25)
                assert found is not None, "no tolerance that stops a solve at a clear iteration"
                tol = found[0]
            if kind == "sweep":
                its = s.be.admm_update_var(RHO, tol, maxit)
                mits, _ = model.sweep(RHO, tol, maxit)
            else:
                its, p, d, e = s.be.admm_step(RHO, tol, maxit) if s.be.has_admm_step else (
                    s.be.admm_update_var(RHO, tol, maxit), s.be.cal_obj(host.PAIR_UV), s.be.cal_dual_obj(),
                    s.be.update_dimacs(host.PAIR_UV))
                mits, mp, md, me, _ = model.step(RHO, tol, maxit)
                # (dObj = b . lambda relative to ||b||_1 max |lambda_i|: lambda is held to its own scale)
                dscale = float(np.sum(np.abs(model.b)) * np.max(np.abs(model.lam)))
                for lbl, x, y, sc in (("pObj", p, mp, 1.0), ("dObj", d, md, dscale), ("err1", e, me, 0.0)):
                    err = abs(x - float(y)) / max(abs(float(y)), sc, 1e-300)
                    worst = max(worst, err)
                    assert err <= BOUND, (name, i, lbl, x, float(y), err)
            assert its == mits, (name, i, its, mits)
            for k in range(s.nblk):
                for lbl, which, want in (("U", host.MAT_U, model.U[k]), ("V", host.MAT_V, model.V[k])):
                    err = common.rel_to_scale(s.be.get_mat(which, k), want)
                    worst = max(worst, err)
                    assert err <= BOUND, (name, i, lbl, k, err)
            err = common.rel_to_scale(s.be.get_vec(host.VEC_CONSTR_SUM), model.csum)
            worst = max(worst, err)
            assert err <= BOUND, (name, i, "constraint sums", err)
            s.be.update_dual_var(RHO)
            model.update_dual(RHO)
            err = common.rel_to_scale(s.be.get_vec(host.VEC_LAMBDA), model.lam)
            worst = max(worst, err)
            assert err <= BOUND, (name, i, "lambda", err)
        print(name, "worst rel-to-scale error, oracle vs model: %.2e" % worst)
    finally:
        s.close()


# ---- solves that pass on their initial residual: the model's counts (the cone's stale count, Q7), the tolerances its search finds
# and its solved states against the oracle, on every golden instance and on the three LP shapes of test_lp_block
NEW_LP = ["sdpslack300", "sdplp300", "coupledlp_free"]
STOPS = (3, 4, 5, 6, 2, 7, 8, 1)


def _path(name):
    return common.instance_path(name) if os.path.exists(common.instance_path(name)) else common.generated_instance(name)


class _Pair:
    """an oracle session and the model in the same seeded state; run() takes both through one sweep or step and compares"""

    def __init__(self, name):
        self.name, self.bound, self.worst = name, BOUNDS.get(name, BOUND), 0.0
        self.s = common.oracle_session(_path(name))
        self.model = AdmmModel.from_file(_path(name))
        self.U, self.V, self.lam = common.random_uv_state(self.s, 11)
        self.load(self.U, self.V)
        self.ncg = sum(1 for cn in self.model.cones if not cn.is_lp)

    def load(self, U, V):
        common.load_uv_state(self.s.be, U, V, self.lam)
        self.model.set_state(U, V, self.lam)

    def _err(self, what, got, want):
        err = common.rel_to_scale(got, want)
        self.worst = max(self.worst, err)
        assert err <= self.bound, (self.name, what, err)

    def factors(self):
        be = self.s.be
        return [be.get_mat(host.MAT_U, k) for k in range(self.s.nblk)], [be.get_mat(host.MAT_V, k) for k in range(self.s.nblk)]

    def run(self, kind, maxit, tol, tag):
        """returns (the model's per-solve counts, the count both returned)"""
        be, model = self.s.be, self.model
        before = self.factors()
        if kind == "sweep":
            its = be.admm_update_var(RHO, tol, maxit)
            mits, log = model.sweep(RHO, tol, maxit)
        else:
            its, p, d, e = be.admm_step(RHO, tol, maxit) if be.has_admm_step else (
                be.admm_update_var(RHO, tol, maxit), be.cal_obj(host.PAIR_UV), be.cal_dual_obj(), be.update_dimacs(host.PAIR_UV))
            mits, mp, md, me, log = model.step(RHO, tol, maxit)
            dscale = float(np.sum(np.abs(model.b)) * np.max(np.abs(model.lam)))
            for lbl, x, y, sc in (("pObj", p, mp, 1.0), ("dObj", d, md, dscale), ("err1", e, me, 0.0)):
                err = abs(x - float(y)) / max(abs(float(y)), sc, 1e-300)
                self.worst = max(self.worst, err)
                assert err <= self.bound, (self.name, tag, lbl, x, float(y), err)
        counts = tuple(e[2] for e in log)
        assert its == mits, (self.name, tag, "CG count", its, mits, counts)
        after = self.factors()
        for k, half, it, hist in log:  # a solve that passed has touched nothing
            if passed_at_once(it, hist, tol):
                assert np.array_equal(after[half][k], before[half][k]), (self.name, tag, "a solve that passed moved its factor", k, half)
        for k in range(self.s.nblk):
            self._err((tag, "U", k), after[0][k], model.U[k])
            self._err((tag, "V", k), after[1][k], model.V[k])
        self._err((tag, "constraint sums"), be.get_vec(host.VEC_CONSTR_SUM), model.csum)
        be.update_dual_var(RHO)
        model.update_dual(RHO)
        self._err((tag, "lambda"), be.get_vec(host.VEC_LAMBDA), model.lam)
        return counts, its

    def close(self):
        print(self.name, "worst rel-to-scale error, oracle vs model: %.2e" % self.worst)
        self.s.close()


def _independent(model, k):
    """cone k's constraints touch no earlier cone: nothing that runs before its U-solve moves that solve's right-hand side"""
    return not any(np.intersect1d(model.cones[k].cons, model.cones[j].cons).size for j in range(k))


def u_runs_v_passes(model, maxit=30):
    """(tolerance, counts) at which every U-solve of the model's next sweep iterates and every V-solve passes at once, or -- where
    no tolerance does that for all cones together -- at which some cone's two solves do"""
    ncg = sum(1 for cn in model.cones if not cn.is_lp)
    found = pattern_tol(model, RHO, maxit, [RUN, 0] * ncg)
    for k in range(ncg if not found else 0):
        pat = [None] * (2 * ncg)
        pat[2 * k], pat[2 * k + 1] = RUN, 0
        found = found or pattern_tol(model, RHO, maxit, pat)
    return found


@pytest.fixture(params=TRACE_NAMES + NEW_LP)
def pair(request, oracle_lib):
    p = _Pair(request.param)
    yield p
    p.close()


def test_all_pass_sweeps_add_the_stale_counts(pair):
    """a: a fixed sweep of 3 iterations per solve, then a sweep and a step at tolerance 0.5: every solve passes, nothing but the LP
    columns moves, and both return the cone's stale count (3) once per solve"""
    counts, its = pair.run("sweep", 3, 0.0, "fixed")
    assert counts == (3,) * (2 * pair.ncg) and its == 6 * pair.ncg
    for kind in ("sweep", "step"):
        lp_before = [f[-1].copy() for f in pair.factors()]
        counts, its = pair.run(kind, 30, 0.5, "all pass, " + kind)
        assert counts == (0,) * (2 * pair.ncg), (pair.name, kind, counts)
        assert its == 6 * pair.ncg, (pair.name, kind, its)
        if pair.model.cones[-1].is_lp:  # no CG, no count -- and its columns are updated all the same
            assert all(np.all(f[-1] != b) for f, b in zip(pair.factors(), lp_before)), pair.name


def test_solved_u_passes_and_v_stops_where_the_model_says(pair):
    """b: U holds the converged U-solve for the loaded V (cone by cone); the sweep runs at a tolerance of the model's search at
    which those U-solves pass (their residual is rounding) and some V-solve is stopped after a clear j iterations"""
    model = pair.model
    pair.load(*solved_state(model, RHO))
    pattern = []
    for k in range(pair.ncg):
        pattern += [0 if _independent(model, k) else None, RUN]
    found = None
    for j in STOPS:
        found = found or pattern_tol(model, RHO, 30, pattern, stop=j)
    assert found, (pair.name, "no tolerance at which the solved U passes and a V-solve stops at a clear iteration")
    counts, its = pair.run("sweep", 30, found[0], "solved U")
    print(pair.name, "solved U, tol %.3e:" % found[0], counts)
    assert counts == found[1] and counts[0] == 0 and max(counts) >= 1
    assert its == sum(counts)  # (a fresh session: the U-solves that pass add the stale count 0, and every V-solve iterates)


def test_u_runs_v_passes_and_the_next_all_pass_sweep_adds_it_twice(pair):
    """c: the tolerance of the model's search at which U-solves iterate and the V-solves behind them pass at once (for all cones
    where one tolerance does it, else for one cone), then d: an all-pass sweep, which adds every cone's latest count twice more"""
    model = pair.model
    found = u_runs_v_passes(model)
    for _ in range(0 if found else 2):  # (a fixed sweep first where the seeded state offers no such tolerance)
        pair.run("sweep", 1, 0.0, "fixed")
        found = found or u_runs_v_passes(model)
    assert found, (pair.name, "no tolerance at which a U-solve iterates and its V-solve passes")
    counts, its = pair.run("sweep", 30, found[0], "U runs, V passes")
    print(pair.name, "U runs, V passes, tol %.3e:" % found[0], counts)
    assert counts == found[1] and any(counts[2 * k] >= 1 and counts[2 * k + 1] == 0 for k in range(pair.ncg))
    stale = list(model.cg_last)
    assert any(stale) and len(stale) == pair.s.nblk
    counts, its = pair.run("sweep", 30, 0.5, "all pass")
    assert counts == (0,) * (2 * pair.ncg), (pair.name, counts)
    assert its == 2 * sum(stale), (pair.name, its, stale)


@pytest.mark.parametrize("name", ["sdplp40", "sdpslack30", "coupledlp"] + NEW_LP)
def test_lp_shapes(name):
    """which path of the LP column sweep an instance takes, from the model's data: one level (the flat kernel), a level longer
    than a workgroup of 256, a column without a constraint entry"""
    model = AdmmModel.from_file(_path(name))
    cn = model.cones[-1]
    assert cn.is_lp and not any(c.is_lp for c in model.cones[:-1])
    levels = lp_levels(model, model.nb - 1)
    assert sum(levels) == cn.n
    want = dict(sdplp40=(52, 4, 40), sdpslack30=(30, 1, 30), coupledlp=(18, 8, 3), sdpslack300=(300, 1, 300), sdplp300=(312, 3, 300),
                coupledlp_free=(19, 8, 4))[name]
    assert (cn.n, len(levels), max(levels)) == want, (name, cn.n, levels)
    empty = [col for col in range(cn.n) if not np.any(cn.a_row == col)]
    assert empty == ([18] if name == "coupledlp_free" else []), (name, empty)
    if empty:
        assert 18 in cn.c_row  # (the column has a cost)
