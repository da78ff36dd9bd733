"""The extended-precision phase-1 model (tests/alm_model.py) against the CPU oracle, which is itself pinned to the compiled reference
(tests/test_oracle_vs_reference.py): consecutive inner iterations without any resync, slot by slot, at history lengths 1, 2, 3 and 5.
This proves the model's conventions -- the gradient's weights, the count of history pairs the direction reads, the order of the two
loops, the fallback, the line search's coefficients, the history update -- before the device is held to it
(tests/test_fixed_count_alm.py).  Both sides take the same tau, from the host's scalar code on the MODEL's coefficients.

Bound: max(32 max_i e64(i), 1e-14), never above 1e-11, over the iterations before the first with e64 > 3e-13, where e64(i) is the
spread between the model in float64 and in longdouble on the same tau schedule (alm_model.plan): nothing is taken from the oracle."""
import numpy as np
import pytest

from lorads_amd import host
from tests import common
from tests.alm_model import LD, AlmModel, _rel, descent_tau, plan, record_errors
from tests.test_hip_parity import TRACE_NAMES

RHO, SEED, LAM_SCALE, ITERS = 0.7, 5, 0.1, 10
NAMES = TRACE_NAMES + ["theta50"]


def _tau(i, coef):
    return common.linesearch_tau(coef)[0]


def _mats(be, which, nb):
    return [be.get_mat(which, k) for k in range(nb)]


def oracle_records(s, recs, rho):
    """the seven slots on a table, with the records' taus; yields (iteration, the table's record)"""
    be, nb = s.be, s.nblk
    lag0 = be.alm_cal_grad(rho)
    for i, want in enumerate(recs):
        be.lbfgs_direction(i)
        got = dict(D=_mats(be, host.MAT_U, nb))
        p1, p2 = be.alm_q12p12()
        coef = be.alm_linesearch_coeffs(rho, p1, p2)
        got.update(p1=p1, p2=p2, a=coef[0], b=coef[1], c=coef[2], d=coef[3], q1=be.get_vec(host.VEC_Q1), q2=be.get_vec(host.VEC_Q2))
        be.set_y_as_neg_grad()
        be.alm_update_var(want["tau"])
        csum_rec = be.get_vec(host.VEC_CONSTR_SUM)
        lag = be.alm_cal_grad(rho)
        be.set_lbfgs_his_two(want["tau"])
        err1 = be.update_dimacs(host.PAIR_RR)
        got.update(R=_mats(be, host.MAT_R, nb), Grad=_mats(be, host.MAT_GRAD, nb), lagNormSq=lag, err1=err1,
                   csum=be.get_vec(host.VEC_CONSTR_SUM))
        if i == 0:
            got["lag0"] = lag0
        yield i, got, csum_rec


@pytest.mark.parametrize("hist", [1, 2, 3, 5])
@pytest.mark.parametrize("name", NAMES)
def test_consecutive_inner_iterations_of_the_model_equal_the_oracle(oracle_lib, name, hist):
    path = common.instance_path(name)
    s = common.oracle_session(path, lbfgs_len=hist)
    try:
        R, lam = common.random_r_state(s, SEED, LAM_SCALE)
        recs, e64, bound, _ = plan(path, R, lam, RHO, ITERS, hist, _tau, min_iters=4)
        # (the well-conditioned cases run past the first wrap of the longest ring)
        assert len(recs) >= hist + 3 or name not in ("rand120", "mix4"), (name, hist, e64)
        common.load_r_state(s.be, R, lam)
        worst = dict(coefficients=0.0, factors=0.0, vectors=0.0, scalars=0.0)
        for i, got, csum_rec in oracle_records(s, recs, RHO):
            err = record_errors(got, recs[i])
            err["vectors"] = max(err["vectors"], common.rel_to_scale(csum_rec, recs[i]["csum_rec"].astype(np.float64)))
            for k, v in err.items():
                worst[k] = max(worst[k], v)
                assert v <= bound, (name, hist, "iteration", i, k, v, "bound", bound, "e64", e64)
            # the model's invariants: the constraint sums by recurrence are A(R R^T), and D descends
            assert _rel(recs[i]["csum_rec"], recs[i]["csum"]) <= 1e-16, (name, i)
            dg = sum(float(np.sum(d * g)) for d, g in zip(recs[i]["D"], recs[i]["grad_before"]))
            assert dg < 0, (name, hist, i, dg)
        print(name, "history", hist, "iterations", len(recs), "e64 %.1e" % max(e64[:len(recs)]), "bound %.1e" % bound,
              "worst", {k: "%.1e" % v for k, v in worst.items()})
    finally:
        s.close()


@pytest.mark.parametrize("hist", [1, 2])
def test_the_fallback_is_taken_by_model_and_oracle(oracle_lib, hist):
    """A step inside the roots of 4 a tau^2 + 3 b tau + 2 c stores a pair with y.s < 0 (alm_model.descent_tau): the two-loop matrix
    is then indefinite and the next direction ascends, so both sides must take D = -Grad at iteration 1."""
    path = common.instance_path("maxcut100")
    s = common.oracle_session(path, lbfgs_len=hist, timesLogRank=0.1)  # (a rank below 10: resize_rank only grows)
    try:
        assert s.block_shape(0)[1] <= 10
        s.be.resize_rank([10])
        R, lam = common.random_r_state(s, SEED, 3.0)
        tau_of = lambda i, coef: descent_tau(coef) if i == 0 else _tau(i, coef)  # noqa: E731
        recs, e64, bound, _ = plan(path, R, lam, 0.02, 6, hist, tau_of)
        assert recs[0]["cos_ys"] <= -0.1 and recs[1]["fallback"] and recs[1]["cos_dg"] >= 0.1, (recs[0]["cos_ys"], recs[1]["cos_dg"])
        common.load_r_state(s.be, R, lam)
        got_grad = None
        for i, got, _ in oracle_records(s, recs, 0.02):
            err = record_errors(got, recs[i])
            assert max(err.values()) <= bound, (hist, i, err, bound)
            if recs[i]["fallback"]:
                assert all(np.array_equal(d, -g) for d, g in zip(got["D"], got_grad)), (hist, i)
            got_grad = got["Grad"]
        print("fallback, history", hist, "cos(y, s) %.2f" % recs[0]["cos_ys"], "cos(D, Grad)", ["%.2f" % r["cos_dg"] for r in recs],
              "taken", [r["fallback"] for r in recs], "e64 %.1e" % max(e64[:len(recs)]))
    finally:
        s.close()


def test_two_loop_recursion_equals_the_dense_inverse_hessian_product():
    """60 unknowns (sdpslack30 at rank 1: a cone of 30 rows and 30 LP columns): q of the two-loop recursion against H g with the BFGS
    inverse-Hessian matrix written out, H_0 = I, H <- (I - beta s y^T) H (I - beta y s^T) + beta s s^T over the pairs it reads,
    oldest first, at every nn up to L.  Both sides are longdouble; the matrix form loses cond(H) eps to its products, so the
    bound is 1e-12 (a pair too few, the loops in the wrong order or a wrong beta give errors of order 1e-2 and more)."""
    path = common.instance_path("sdpslack30")
    rng = np.random.default_rng(3)
    for L in (1, 2, 3, 5):
        mdl = AlmModel.from_file(path, hist_len=L)
        shapes = [(cn.n, 1) for cn in mdl.cones]
        R = [rng.standard_normal(sh) / np.sqrt(sh[0]) for sh in shapes]
        size = sum(a * b for a, b in shapes)
        assert size <= 60, size
        mdl.set_r_state(R, 0.1 * rng.standard_normal(mdl.m))
        mdl.cal_grad(RHO)
        for inner in range(L + 3):
            mdl.direction(inner)
            g = mdl._flat(mdl.Grad)
            nn = 0 if inner == 0 else (inner if inner <= L - 1 else L)
            H = np.eye(g.size, dtype=LD)
            for sv, yv, beta in (mdl.hist[-nn:] if nn else []):
                V = np.eye(g.size, dtype=LD) - beta * np.outer(yv, sv)
                H = V.T @ H @ V + beta * np.outer(sv, sv)
            want = -(H @ g)
            if float(np.sum(want * g)) >= 0:
                want = -g
            assert _rel(mdl._flat(mdl.D), want) <= 1e-12, (L, inner, _rel(mdl._flat(mdl.D), want))
            mdl.q12p12()
            coef, _ = mdl.linesearch_coeffs(RHO)
            mdl.step(_tau(inner, [float(x) for x in coef]), RHO)
