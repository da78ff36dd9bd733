"""CG iteration 0 folded into the operator kernel on cones of the one-kernel front (k_spmm_ell's CG0 form):
LORADS_FUSE_CG0=0 restores k_cg_update as a launch of its own, with the same step length (rr / (rr + ||w||^2)) and the same
per-element arithmetic, so the two forms must agree bit for bit."""
import numpy as np
import pytest

from lorads_amd import host
from tests import common


def _run(path, env, steps, **kw):
    """phase 1 + `steps` ADMM iterations (every third one through the separate entry points) under `env`; tolerances that
    change from step to step give speculation misses and solves of one and of many iterations"""
    with common.environment(env):
        s = common.hip_session(path, phase1Tol=1e-2, **kw)
    try:
        s.alm()
        s.alm_to_admm()
        s.be.init_constr(host.PAIR_UV)
        res0 = s.results()
        rho = min(res0["admm_rho"] if res0["admm_rho"] > 0 else res0["alm_rho"], 5000.0)
        e = s.be.update_dimacs(host.PAIR_UV)
        n0 = s.hip_launch_count()
        log = []
        for it in range(steps):
            tol = [min(1e-2 * e, 1e-8), 1e-4, 1e-12, 1e-6][it % 4]
            if it % 3 == 2:
                c = s.be.admm_update_var(rho, tol, 800)
                p, d, e = s.be.cal_obj(host.PAIR_UV), s.be.cal_dual_obj(), s.be.update_dimacs(host.PAIR_UV)
            else:
                c, p, d, e = s.be.admm_step(rho, tol, 800)
            s.be.update_dual_var(rho)
            log.append((c, p, d, e))
        prof = s.hip_profile_read()
        return dict(log=log, U=[s.be.get_mat(host.MAT_U, k) for k in range(s.nblk)],
                    V=[s.be.get_mat(host.MAT_V, k) for k in range(s.nblk)], lam=s.be.get_vec(host.VEC_LAMBDA),
                    launches=s.hip_launch_count() - n0, misses=prof["speculation_misses"], solves=prof["cg_solves"],
                    cg=prof["cg_iters"])
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,tlr,cw,steps", [("rand120", None, "1", 40), ("rand4000", 4.0, None, 40),
                                               ("coupled3x70", None, "1", 40), ("rand20000", None, None, 10)])
def test_iteration_zero_in_the_operator_is_bitwise_the_separate_update(built, name, tlr, cw, steps):
    path = common.instance_path(name) if name in ("rand120", "coupled3x70") else common.generated_instance(name)
    kw = dict(timesLogRank=tlr) if tlr else {}
    env = {"LORADS_OP_CW": cw} if cw else {}
    a = _run(path, env, steps, **kw)
    b = _run(path, dict(env, LORADS_FUSE_CG0="0"), steps, **kw)
    print(name, "launches fused / separate:", a["launches"], b["launches"], "misses", a["misses"], "solves", a["solves"],
          "cg", a["cg"], "per step", [x[0] for x in a["log"]])
    for it, (x, y) in enumerate(zip(a["log"], b["log"])):
        assert x == y, (it, x, y)
    assert np.array_equal(a["lam"], b["lam"])
    for X, Y in zip(a["U"] + a["V"], b["U"] + b["V"]):
        assert np.array_equal(X, Y)
    assert (a["misses"], a["solves"], a["cg"]) == (b["misses"], b["solves"], b["cg"])
    # the fused form really ran: one launch fewer per solve that reached iteration 0's update
    assert a["launches"] < b["launches"], (a["launches"], b["launches"])
    # ... over solves of more than one iteration as well
    assert a["cg"] > a["solves"], (a["cg"], a["solves"])
