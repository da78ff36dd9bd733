"""The dual-side model (tests/dual_model.py) against independent arithmetic, on the CPU: its Lanczos process against
numpy.linalg.eigvalsh over the cases the device is held to (tests/dual_cases.py), its certificate against numpy_certificate of
tests/test_solution.py, its dual infeasibility against the oracle's slot, and the table of cases on which the float64 and the
extended-precision model disagree about the number of S x products."""
from types import SimpleNamespace

import numpy as np
import pytest

from lorads_amd import host, instances
from tests import common
from tests import dual_cases as dc
from tests import dual_model as dm
from tests.test_solution import numpy_certificate

NAMED = ["maxcut100", "theta30", "rand120", "blk4x60", "coupled3x70", "densec40", "densea40", "matcomp60", "mix4", "sdplp40",
         "sdpslack30", "coupledlp"]


def _cases():
    out = [("edge%d" % n, dc.edge_matrix(n)) for n in dc.EDGE_SIZES]
    out += [(name, S) for name, (S, _) in dc.closed_form().items()]
    return out


CASES = _cases()


@pytest.mark.parametrize("name,S", CASES, ids=[c[0] for c in CASES])
def test_lanczos_against_eigvalsh(name, S):
    """theta lies within res + 64 n eps ||S||_2 of some eigenvalue, never below lambda_min - 64 n eps ||S||_2, and on a breakdown
    (an invariant Krylov space: every Ritz value exact, and the start vector has a component along every eigenvector) it is
    lambda_min to 64 n eps ||S||_2.  The slack that the model assembles from the instance is S itself."""
    n = S.shape[0]
    prob = instances.prescribed_slack(S)
    Sl = dm.slack(prob, -np.diag(S))[0]
    assert np.array_equal(Sl.dense().astype(np.float64), S)
    x = np.random.default_rng(1).standard_normal(n)
    assert np.abs(Sl.matvec(x.astype(dm.LD)).astype(np.float64) - S @ x).max() <= 1e-13 * max(1.0, np.abs(S).sum(axis=1).max()) * np.abs(x).max()
    ev = np.linalg.eigvalsh(S)
    nrm = max(abs(ev[0]), abs(ev[-1]))
    slop = 64 * n * dm.EPS * nrm
    for ncv in dc.NCVS:
        for tol, r in dm.lanczos(Sl, dc.TOLS, ncv, 600).items():
            d = np.abs(ev - r.theta).min()
            assert d <= r.res + slop, (ncv, tol, r, d)
            assert r.theta >= ev[0] - slop, (ncv, tol, r)
            if r.breakdown:
                assert abs(r.theta - ev[0]) <= slop, (ncv, tol, r)
                assert r.matvecs <= r.m + r.restarts * r.m
            else:
                keep = min(dm.KEEP_MAX, r.m - 1)
                assert r.matvecs == r.m + r.restarts * (r.m - keep)
                assert r.restarts == 600 or r.m < 2 or r.res <= tol * max(dm.EPS23, abs(r.theta))


def test_expected_breakdowns():
    """the closed-form cases break down where their spectrum says: after as many steps as the slack has distinct eigenvalues
    with a component in the start vector, whenever the subspace is at least that large"""
    for name, (S, steps) in dc.closed_form().items():
        if steps is None:
            continue
        Sl = dm.slack(instances.prescribed_slack(S), -np.diag(S))[0]
        for ncv in dc.NCVS:
            r = dm.lanczos(Sl, 1e-10, ncv, 600)
            if ncv >= steps:
                assert r.breakdown and r.matvecs == steps and r.restarts == 0, (name, ncv, r)


def test_precisions_agree_on_the_product_count():
    """The table behind the count comparison of tests/test_dual_edges.py: over every edge size and closed-form spectrum, every
    ncv and both tolerances, the cases on which the float64 and the extended-precision model run a different number of products.
    Here: none (so no case is exempt from the count for that reason); the spread of theta between the two stays below
    2e-14 ||S||_2."""
    differ, worst = [], 0.0
    for name, S in CASES:
        prob = instances.prescribed_slack(S)
        lam = -np.diag(S)
        a, b = dm.slack(prob, lam, dm.LD)[0], dm.slack(prob, lam, np.float64)[0]
        nrm = max(np.linalg.norm(S, 2), 1e-300)
        for ncv in dc.NCVS:
            ras, rbs = dm.lanczos(a, dc.TOLS, ncv, 600, dm.LD), dm.lanczos(b, dc.TOLS, ncv, 600, np.float64)
            for tol in dc.TOLS:
                ra, rb = ras[tol], rbs[tol]
                worst = max(worst, abs(ra.theta - rb.theta) / nrm)
                if ra.matvecs != rb.matvecs or ra.breakdown != rb.breakdown:
                    differ.append((name, ncv, tol, ra.matvecs, rb.matvecs))
    print("worst spread / ||S||_2: %.2e; product counts differ on %s" % (worst, differ))
    assert differ == []
    assert worst <= 2e-14


def _fake_solution(path, seed, rank=3):
    m, b, dims, ent = dm.read_sdpa(path)
    rng = np.random.default_rng(seed)
    cones, R, x = [], [], {}
    for k, n in enumerate(dims):
        if n < 0:
            x[k] = rng.random(-n)
            R.append(None)
            cones.append(SimpleNamespace(x=x[k], R=None))
        else:
            R.append(rng.standard_normal((n, rank)) / np.sqrt(n))
            cones.append(SimpleNamespace(x=None, R=R[-1]))
    y = rng.standard_normal(m)
    return SimpleNamespace(y=y, cones=cones), R, x, y


@pytest.mark.parametrize("name", NAMED)
def test_certificate_against_numpy_certificate(name):
    """both are float64-or-better evaluations of the same sums: they agree to 1e-13 of the sum of the absolute terms"""
    path = common.instance_path(name)
    sol, R, x, y = _fake_solution(path, 11)
    want = numpy_certificate(path, sol)
    m, b, dims, ent = dm.read_sdpa(path)
    b = np.asarray(b)
    for dtype in (dm.LD, np.float64):
        c = dm.certificate(path, R, x, y, dtype)
        assert abs(float(c["cx"]) - want["pobj"]) <= 1e-13 * float(c["cx_abs"])
        assert abs(float(c["bl"]) - want["dobj"]) <= 1e-13 * max(float(c["bl_abs"]), 1e-300)
        den = 1 + abs(want["pobj"]) + abs(want["dobj"])
        assert abs(float(c["sx"]) / den - want["err6"]) <= 1e-13 * float(c["sx_abs"]) / den
        assert abs(float(c["nrm2"]) / (1 + np.abs(b).sum()) - want["err1"]) <= 1e-13 * max(1.0, float(c["nrm2"]))
        assert abs(float(c["ninf"]) / (1 + c["binf"]) - want["err1_inf"]) <= 1e-13 * max(1.0, float(c["ninf"]))
        assert c["binf"] == np.abs(b).max()
        S = want["S"]
        for k, n in enumerate(dims):
            if n < 0:
                assert abs(float(c["lp_min"][k]) - S[k].diagonal().min()) <= 1e-13 * max(1.0, np.abs(S[k].diagonal()).max())
        Sm = dm.slack(path, y, dtype)
        for k in range(len(dims)):
            dense = np.diag(Sm[k].diagonal().astype(np.float64)) if Sm[k].is_lp else Sm[k].dense().astype(np.float64)
            assert np.abs(dense - S[k].toarray()).max() <= 1e-13 * max(1.0, np.abs(S[k]).max())


@pytest.mark.parametrize("name", NAMED)
def test_dual_infeasibility_against_the_oracle_slot(name, oracle_lib):
    """sum_k |min(theta_k, 0)| (plus the LP columns' shares) with the model driven to 1e-10 against the oracle's slot"""
    path = common.instance_path(name)
    lam = np.random.default_rng(5).standard_normal(instances.NAMED[name]()["m"])
    s = common.oracle_session(path)
    try:
        s.be.set_vec(host.VEC_LAMBDA, lam)
        want = s.be.dual_infeasibility()
    finally:
        s.close()
    got, mins, nmv, results, lp = dm.dual_infeasibility(path, lam, tol=1e-10)
    ex_tot, ex = common.exact_dual_infeasibility(instances.NAMED[name](), lam)
    assert got == pytest.approx(want, rel=1e-8)
    assert got == pytest.approx(ex_tot, rel=1e-8)
    assert np.allclose(mins, ex, rtol=1e-8, atol=1e-10)
