"""The extended-precision ADMM model (tests/admm_model.py) against the CPU oracle, which is itself pinned to the compiled reference
(tests/test_oracle_vs_reference.py): this proves the model's conventions -- data transformations, right-hand side, CG restarts and
stopping rule, the LP columns, the dual update, the step's scalars -- before the device is held to it
(tests/test_fixed_count_sweeps.py).  Fixed-count sweeps leave no iteration count or tolerance to absorb an error."""
import numpy as np
import pytest

from lorads_amd import host
from tests import common
from tests.admm_model import AdmmModel, stopping_tol
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
