"""The rows per workgroup of the two row-tile gather kernels, k_front_cw and k_spmm_ell (row_deal).

LORADS_ROW_DEAL=0 keeps 32 rows per workgroup, the default deals a cone of more than 32 rows per compute unit evenly over the
compute units, and an integer 1..32 forces that many rows for every cone, which brings the tile edges to small cones: 5 rows leave
three of a workgroup's four wavefronts without a row, 27 is no multiple of a wavefront's eight lane groups (and no divisor of most
cone sizes), 32 is the trivial case.  The deal changes which rows share a workgroup, i.e. how the partial sums of the norms are
grouped, and nothing else: 32 against 0 is bit for bit, 5 and 27 move last bits only.

Bounds: 1e-12 relative to scale for factors and multipliers, 1e-12 relative for the objectives, the bound of
tests/test_fixed_count_sweeps.py (regrouped partial sums of at most a few thousand terms move the sums by a few 1e-16)."""
import functools
import math

import numpy as np
import pytest

from lorads_amd import host
from tests import common
from tests import test_fixed_count_sweeps as fcs

BOUND = 1e-12
CASES = {  # name -> (environment, parameters, ADMM steps)
    "rand120": ({"LORADS_OP_CW": "1"}, {}, 40),
    "rand123": ({"LORADS_OP_CW": "1"}, {}, 40),   # (123 rows: the last workgroup is partial at 5 and at 27 rows per workgroup)
    "hub16": ({"LORADS_OP_CW": "1"}, {}, 40),     # rows 0-2 hold 60 slots: the CSR tails of both kernels run
    "wide60": ({"LORADS_OP_CW": "1"}, {}, 40),
    "rand4000": ({}, dict(timesLogRank=4.0), 10),
}


def _path(name):
    if name == "rand123":
        from lorads_amd import instances
        return common.generated_instance(name, lambda: instances.randsparse(123, 40, 2001, c_edges=150, n_diag=2, n_off=3, r0=3))
    return fcs._path(name)


def rule(n, ncu):
    """row_deal of the HIP library, restated: (rows per workgroup, grid)"""
    g0 = -(-n // 32)
    if g0 <= ncu:
        return 32, g0
    k = -(-g0 // ncu)
    rpw = min(32, -(-n // (k * ncu)))
    return rpw, -(-n // rpw)


def maxpart(n):
    """capacity of a partial-sum slot of a one-cone context (ctx_init)"""
    return max(4096, (((n + 3) // 4 + 1) + 255) // 256 * 256)


REPEAT_TOLS = [1e-8, 1e-8, 1e-8, 1e-8, 1e-3, 1e-8, 1e-8, 1e-12, 1e-8, 1e-8]


def _run_fresh(name, deal, extra=(), repeat=False):
    """phase 1 + the case's ADMM steps (every third one through the separate entry points, tolerances that change from step to step)
    with LORADS_ROW_DEAL=`deal` (None: unset) and the switches `extra`.  repeat: 70 steps whose tolerances mostly repeat, every
    seventh through the separate entry points, rho raised every tenth -- launch chains come up again, so a context that replays
    captured chains does (the schedule of test_graph_replay_is_bitwise_the_launch_by_launch_iteration)"""
    env, params, steps = CASES[name]
    env = dict(env, **dict(extra))
    if deal is not None:
        env["LORADS_ROW_DEAL"] = str(deal)
    s = common.hip_session_with_env(_path(name), env, dict(params, phase1Tol=1e-2))
    try:
        s.alm()
        s.alm_to_admm()
        s.be.init_constr(host.PAIR_UV)
        res0 = s.results()
        rho = min(res0["admm_rho"] if res0["admm_rho"] > 0 else res0["alm_rho"], 5000.0)
        e = s.be.update_dimacs(host.PAIR_UV)
        log = []
        for it in range(70 if repeat else steps):
            tol = REPEAT_TOLS[it % 10] if repeat else [min(1e-2 * e, 1e-8), 1e-4, 1e-12, 1e-6][it % 4]
            if it % 7 == 6 if repeat else it % 3 == 2:
                c = s.be.admm_update_var(rho, tol, 800)
                p, d, e = s.be.cal_obj(host.PAIR_UV), s.be.cal_dual_obj(), s.be.update_dimacs(host.PAIR_UV)
            else:
                c, p, d, e = s.be.admm_step(rho, tol, 800)
            s.be.update_dual_var(rho)
            if repeat and it % 10 == 9:
                rho *= 1.2
            log.append((c, p, d, e))
        prof = s.hip_profile_read()
        n = s.block_shape(0)[0]
        return dict(log=log, U=s.be.get_mat(host.MAT_U, 0), V=s.be.get_mat(host.MAT_V, 0), lam=s.be.get_vec(host.VEC_LAMBDA),
                    cg=prof["cg_iters"], solves=prof["cg_solves"], deal=s.hip_row_deal_stats(0), n=n, kind=s.hip_operator_kind(0),
                    image=s.hip_block_image(0), spec=s.hip_spec_front_stats(), graphs=s.hip_graph_stats())
    finally:
        s.close()


@functools.lru_cache(maxsize=None)
def _run(name, deal, extra=(), repeat=False):
    """_run_fresh, once per test process and left unchanged by whoever reads it"""
    return _run_fresh(name, deal, extra, repeat)


def _on_front_path(res):
    assert res["kind"] == fcs.CW and res["image"]["front_cw"] == 1, (res["kind"], res["image"])


def _assert_bitwise(a, b):
    for it, (x, y) in enumerate(zip(a["log"], b["log"])):
        assert x == y, (it, x, y)
    assert np.array_equal(a["lam"], b["lam"]) and np.array_equal(a["U"], b["U"]) and np.array_equal(a["V"], b["V"])
    assert (a["cg"], a["solves"]) == (b["cg"], b["solves"])


# ---- 1. 32 rows per workgroup through the new argument against the switch off
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rand120", "hub16"])
def test_forced_32_is_bitwise_the_switch_off(built, name):
    a, b = _run(name, 32), _run(name, 0)
    _on_front_path(a)
    n = a["n"]
    assert (a["deal"]["rpw"], a["deal"]["grid"]) == (32, -(-n // 32)) == (b["deal"]["rpw"], b["deal"]["grid"])
    _assert_bitwise(a, b)


# ---- 2. forced 5 and 27 against the switch off: the last bits of regrouped sums
@pytest.mark.gpu
@pytest.mark.parametrize("deal", [5, 27])
@pytest.mark.parametrize("name", ["rand120", "hub16", "wide60", "rand4000"])
def test_forced_deals_against_the_switch_off(built, name, deal):
    a, b = _run(name, deal), _run(name, 0)
    _on_front_path(a)
    assert (a["deal"]["rpw"], a["deal"]["grid"]) == (deal, -(-a["n"] // deal)), a["deal"]
    worst = dict(U=common.rel_to_scale(a["U"], b["U"]), V=common.rel_to_scale(a["V"], b["V"]), lam=common.rel_to_scale(a["lam"], b["lam"]),
                 obj=max(max(abs(x[1] - y[1]) / max(abs(y[1]), 1e-300), abs(x[2] - y[2]) / max(abs(y[2]), 1e-300))
                         for x, y in zip(a["log"], b["log"])))
    print(name, deal, "worst", {k: "%.2e" % v for k, v in worst.items()}, "cg per step", [x[0] for x in a["log"]])
    assert [x[0] for x in a["log"]] == [y[0] for y in b["log"]], "CG iteration counts"
    assert (a["cg"], a["solves"]) == (b["cg"], b["solves"])
    assert all(v <= BOUND for v in worst.values()), worst


# ---- 3. the forced deals against the extended-precision model, fixed counts of sweeps
@pytest.mark.gpu
@pytest.mark.parametrize("deal", [5, 27])
@pytest.mark.parametrize("name,env,schedule", [("rand120", {"LORADS_OP_CW": "1"}, fcs.FULL), ("hub16", {"LORADS_OP_CW": "1"}, fcs.FULL),
                                               ("wide60", {"LORADS_OP_CW": "1"}, fcs.FULL), ("rand4000", {}, fcs.SHORT)])
def test_forced_deals_against_the_model(built, monkeypatch, name, env, schedule, deal):
    seen = []

    def session(path, env_, params, separable=None):  # (the deal of the very context that runs the schedule)
        s = common.hip_session_with_env(path, env_, params, separable)
        seen.append((s.hip_row_deal_stats(0), s.block_shape(0)[0]))
        return s

    monkeypatch.setattr(fcs, "_session", session)
    facts, worst = fcs.run_case(name, dict(env, LORADS_ROW_DEAL=str(deal)), schedule=schedule)
    (stats, n), = seen
    assert (stats["rpw"], stats["grid"]) == (deal, -(-n // deal)), (stats, n)
    assert facts["kinds"] == [fcs.CW] and facts["images"][0]["front_cw"] == 1, facts
    assert max(worst["factors"], worst["vectors"], worst["scalars"]) <= BOUND, worst


# ---- 4. a forced deal is bit for bit itself in a fresh context (hub16: the tails; rand123: a partial last workgroup at 5 and at 27)
@pytest.mark.gpu
@pytest.mark.parametrize("deal", [5, 27])
@pytest.mark.parametrize("name", ["hub16", "rand123"])
def test_forced_deal_is_deterministic(built, name, deal):
    a, b = _run(name, deal), _run_fresh(name, deal)
    _on_front_path(a)
    assert (a["deal"]["rpw"], a["deal"]["grid"]) == (deal, -(-a["n"] // deal)) and a["deal"] == b["deal"]
    if name == "rand123":
        assert a["n"] % deal != 0
    _assert_bitwise(a, b)


# ---- 5. at 27 rows per workgroup the existing switches stay bit for bit against each other
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rand120", "rand4000"])
@pytest.mark.parametrize("switch", ["LORADS_FUSE_CG0", "LORADS_SPEC_FRONT", "LORADS_GRAPH"])
def test_switches_at_27_rows(built, name, switch):
    if switch == "LORADS_GRAPH":
        a, b = _run(name, 27, (("LORADS_GRAPH", "1"),), True), _run_fresh(name, 27, (("LORADS_GRAPH", "0"),), True)
    else:
        a, b = _run(name, 27), _run_fresh(name, 27, ((switch, "0"),))
    _on_front_path(a)
    assert a["deal"]["rpw"] == 27 == b["deal"]["rpw"]
    if switch == "LORADS_SPEC_FRONT":
        assert a["spec"]["adopted"] > 0 and b["spec"]["enqueued"] == 0, (a["spec"], b["spec"])
    if switch == "LORADS_GRAPH":  # (chains really were captured and replayed on one side, none on the other)
        print(name, "graphs", a["graphs"], b["graphs"])
        assert a["graphs"]["replayed"] >= 10 and b["graphs"]["captured"] == 0 == b["graphs"]["replayed"], (a["graphs"], b["graphs"])
    _assert_bitwise(a, b)


# ---- 6. the rule
def test_rule_restated():
    assert rule(20000, 256) == (27, 741)
    assert rule(40000, 256) == (32, 1250)
    assert rule(10000, 256) == (20, 500)
    assert rule(8192, 256) == (32, 256) and rule(8193, 256) == (17, 482)
    for ncu in (1, 2, 3, 7, 104, 256, 304):
        for n in list(range(1, 700)) + [4000, 19999, 20000, 20001, 65537, 1 << 20]:
            rpw, grid = rule(n, ncu)
            g0 = -(-n // 32)
            assert 1 <= rpw <= 32 and grid * rpw >= n and (grid - 1) * rpw < n and grid <= maxpart(n), (n, ncu, rpw, grid)
            if g0 <= ncu:
                assert (rpw, grid) == (32, g0)
            # the fullest compute unit never gets more rows than before
            assert -(-grid // ncu) * rpw <= -(-g0 // ncu) * 32, (n, ncu, rpw, grid)


@pytest.mark.gpu
@pytest.mark.parametrize("name,cus", [("rand120", [1, 2, 3, 4, 256]), ("hub16", [1, 3, 7, 25, 26, 256]), ("rand4000", [4, 7, 33, 100, 124, 125, 256])])
def test_rule_on_pretended_compute_units(built, name, cus):
    env, params, _ = CASES[name]
    for ncu in cus:
        s = common.hip_session_with_env(_path(name), dict(env, LORADS_ROW_DEAL_CUS=str(ncu)), dict(params, phase1Tol=1e-2))
        try:
            st, n = s.hip_row_deal_stats(0), s.block_shape(0)[0]
        finally:
            s.close()
        rpw, grid, g0 = st["rpw"], st["grid"], -(-n // 32)
        assert st["ncu"] == ncu and (rpw, grid) == rule(n, ncu), (st, n)
        assert grid * rpw >= n and rpw <= 32 and grid <= maxpart(n)
        if g0 <= ncu:
            assert rpw == 32
        assert math.ceil(grid / ncu) * rpw <= math.ceil(g0 / ncu) * 32
    # the device's own count without the pretence, and the switch off whatever the count
    for env2, want in ((dict(env), None), (dict(env, LORADS_ROW_DEAL="0", LORADS_ROW_DEAL_CUS="3"), (32, None))):
        s = common.hip_session_with_env(_path(name), env2, dict(params, phase1Tol=1e-2))
        try:
            st, n = s.hip_row_deal_stats(0), s.block_shape(0)[0]
        finally:
            s.close()
        assert (st["rpw"], st["grid"]) == (rule(n, st["ncu"]) if want is None else (32, -(-n // 32))), (st, n)
