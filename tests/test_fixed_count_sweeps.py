"""Fixed-count ADMM sweeps of every operator form against the extended-precision model (tests/admm_model.py).

A truncated CG is a fixed rational function of its inputs: after exactly K iterations (tol 0), or stopped by a tolerance that the
model's residual history puts between two clearly different residuals, no iteration count and no tolerance is left to absorb an error
of the device.  Each case sets a seeded state (set_mat / set_vec, init_constr(PAIR_UV)), runs a schedule of sweeps with the dual update
between them on the device and on the model, and checks after every sweep: U and V per cone, the CG count exactly, the device's
constraint sums against A(U V^T) formed by the model from the device's OWN factors (so a missed step of the recurrence that keeps them
shows apart from CG rounding), lambda, and the step's pObj, dObj and err1.  Every case also checks that its form really ran
(operator kind, block image, one-launch statistics, launch counts): a case that silently falls back tests nothing.

Bounds: relative to the vector's largest entry (dObj: to ||b||_1 max |lambda|), at most 100x the worst error measured on the MI355X
per group of cases and never above 1e-11 (factors, constraint sums); the measured figure stands next to each bound."""
import os

import numpy as np
import pytest

from lorads_amd import host
from tests import common
from tests.admm_model import AdmmModel, stopping_tol

pytestmark = pytest.mark.gpu

RHO = 1.5
# worst rel-to-scale error measured on the MI355X over all cases of a group (factors / m-vectors / scalars), and its bound
BOUNDS = {
    "default": 1e-12,  # measured 1.5e-13 (theta30, constraint sums); theta50 1.6e-13, hub16 1.4e-14, every other case <= 1e-14
    # (the variants of the one-launch iteration, tests/test_one_launch_variants.py: this cap and below it max(32 x the spread of the
    # model in float64, 1e-14) per case; measured <= 1.3e-14 (n = 4128, factors), every other case <= 4.9e-15)
}


def _path(name):
    return common.instance_path(name) if os.path.exists(common.instance_path(name)) else common.generated_instance(name)


_session = common.hip_session_with_env


# schedules: (entry point, maxit, tol) -- tol 0.0 runs exactly maxit iterations per solve; a tuple (j, ...) asks the model for a
# tolerance that stops some solve after exactly j iterations (the first j of the tuple that has one; see stopping_tol)
FULL = [("sweep", 1, 0.0), ("step", 24, 0.0), ("sweep", 30, (3, 5, 4, 2, 6, 7, 8)), ("step", 2, 0.0),
        ("step", 30, (6, 2, 7, 8, 4, 3, 5))]
SHORT = [("sweep", 2, 0.0), ("step", 1, 0.0), ("sweep", 24, 0.0)]
HEADLINE = [("step", 1, 0.0), ("sweep", 2, 0.0), ("step", 2, 0.0)]
RANKS = [("sweep", 2, 0.0), ("step", 1, 0.0)]


def find_stop(model, name, i, js, maxit, fixed, stops):
    """the tolerance of schedule entry i whose stops are asked for by the tuple js, from the model alone: (tol, maxit); the
    iteration it stops at is appended to `stops` (None: no such tolerance, and the sweep runs maxit iterations at tolerance 0)"""
    if fixed:
        # the stop is looked for among the first 40 iterations; with every solve stopped by then, maxit plays no part
        js = tuple(j for j in js if j not in stops) + js
        found = stopping_tol(model, RHO, js, maxit, probe_maxit=40) or stopping_tol(model, RHO, js, maxit, ratio=1.25, probe_maxit=40)
        stops.append(found[1] if found else None)
        assert found, (name, i, "no tolerance that stops every solve early", js)
        return found[0], maxit
    pref = js + tuple(j for j in range(1, 16) if j not in js)
    found = None
    # a stop not taken yet first; a solve that never nears the tolerance runs to maxit, so a smaller maxit leaves fewer
    # residuals to keep clear of
    for js in (tuple(j for j in pref if j not in stops), pref):
        for mx in (maxit, 21, 12, 8, 6, 4):
            found = stopping_tol(model, RHO, js, mx) or stopping_tol(model, RHO, js, mx, ratio=1.25)
            if found:
                maxit = mx
                break
        if found:
            break
    stops.append(found[1] if found else None)
    return (found[0] if found else 0.0), maxit


def run_case(name, env=None, params=None, schedule=FULL, ranks=None, separable=None, hook=False, seed=5, path=None, tag=None,
             stamps=False, spread=False):
    """runs the schedule on the device and the model; returns (session facts, worst errors by group).
    path: the instance's file where `name` is no named one.  A schedule entry may carry a fourth field "fixed": its maxit stays
    what it says whatever tolerance the model finds (the tolerance is then looked for among the first iterations only, and every
    solve of the sweep must stop by it).  tag: the one-launch form's next tag (lorads_hip_persist_set_tag), set once its plan
    exists.  stamps: the one-launch form's stamps are on for the schedule and facts["l2"] holds what its latest launch decided
    (lorads_hip_persist_stamps, word 15; None: no such launch).  spread: the same schedule also runs on the model in float64 and
    worst["spread"] is the largest difference between the two models over every compared quantity (what the reference's own
    arithmetic leaves open: a bound taken from it owes nothing to the device)."""
    path = path or _path(name)
    s = _session(path, env or {}, params or {}, separable)
    try:
        calls = []
        if hook:
            s.set_allreduce(lambda ptr, count, on_device: calls.append(count))
        if ranks is not None:
            s.be.resize_rank([ranks] * s.nblk if isinstance(ranks, int) else ranks)
        model = AdmmModel.from_file(path)
        assert model.m == s.m and model.nb == s.nblk
        U, V, lam = common.random_uv_state(s, seed)
        be = s.be
        common.load_uv_state(be, U, V, lam)
        model.set_state(U, V, lam)
        worst = dict(factors=0.0, vectors=0.0, scalars=0.0)
        m64 = None
        if spread:
            m64 = AdmmModel.from_file(path, dtype=np.float64)
            m64.set_state(U, V, lam)
            worst["spread"] = 0.0
        n0, p0 = s.hip_launch_count(), s.hip_persist_stats()["iterations"]
        if tag is not None:
            s.hip_persist_set_tag(tag)
        if stamps:
            s.hip_persist_stamps(True)
        counts, stops, persist_calls = [], [], []
        for i, entry in enumerate(schedule):
            kind, maxit, tol = entry[:3]
            fixed = len(entry) > 3 and entry[3] == "fixed"
            pnow = s.hip_persist_stats()["iterations"]
            if isinstance(tol, tuple):
                tol, maxit = find_stop(model, name, i, tol, maxit, fixed, stops)
            if kind == "sweep":
                its = be.admm_update_var(RHO, tol, maxit)
                mits, _ = model.sweep(RHO, tol, maxit)
            else:
                its, p, d, e = be.admm_step(RHO, tol, maxit)
                mits, mp, md, me, _ = model.step(RHO, tol, maxit)
                dscale = float(np.sum(np.abs(model.b)) * np.max(np.abs(model.lam)))
                for lbl, x, y, sc in (("pObj", p, mp, 1.0), ("dObj", d, md, dscale), ("err1", e, me, 0.0)):
                    err = abs(x - float(y)) / max(abs(float(y)), sc, 1e-300)
                    worst["scalars"] = max(worst["scalars"], err)
            counts.append(its)
            persist_calls.append(s.hip_persist_stats()["iterations"] - pnow)
            assert its == mits, (name, i, "CG iterations", its, mits)
            if m64 is not None:
                if kind == "sweep":
                    its64, _ = m64.sweep(RHO, tol, maxit)
                else:
                    its64, p64, d64, e64, _ = m64.step(RHO, tol, maxit)
                    for x, y, sc in ((p64, mp, 1.0), (d64, md, dscale), (e64, me, 0.0)):
                        worst["spread"] = max(worst["spread"], abs(float(x) - float(y)) / max(abs(float(y)), sc, 1e-300))
                assert its64 == mits, (name, i, "CG iterations of the model in float64", its64, mits)
                for k in range(s.nblk):
                    worst["spread"] = max(worst["spread"], common.rel_to_scale(m64.U[k], model.U[k]), common.rel_to_scale(m64.V[k], model.V[k]))
                worst["spread"] = max(worst["spread"], common.rel_to_scale(m64.csum, model.csum))
            Ud = [be.get_mat(host.MAT_U, k) for k in range(s.nblk)]
            Vd = [be.get_mat(host.MAT_V, k) for k in range(s.nblk)]
            for k in range(s.nblk):
                worst["factors"] = max(worst["factors"], common.rel_to_scale(Ud[k], model.U[k]), common.rel_to_scale(Vd[k], model.V[k]))
            # the device's constraint sums against A(.) of its own factors: A(U V^T) after a sweep, A(R R^T) after a step's evaluation
            if kind == "sweep":
                want = model.auv(Ud, Vd)
            else:
                Rd = [(u + v) / 2 for u, v in zip(Ud, Vd)]
                want = model.auv(Rd, Rd)
            worst["vectors"] = max(worst["vectors"], common.rel_to_scale(be.get_vec(host.VEC_CONSTR_SUM), want))
            be.update_dual_var(RHO)
            model.update_dual(RHO)
            worst["vectors"] = max(worst["vectors"], common.rel_to_scale(be.get_vec(host.VEC_LAMBDA), model.lam))
            if m64 is not None:
                m64.update_dual(RHO)
                worst["spread"] = max(worst["spread"], common.rel_to_scale(m64.lam, model.lam))
        # every tolerance sweep found its stop, and at different iterations where there are two (speculation over- and undershoots)
        assert all(stops), (name, "no tolerance that stops a solve at a clear iteration", stops)
        assert len(stops) < 2 or len(set(stops)) >= 2, (name, "the tolerance sweeps stop at the same iteration", stops)
        facts = dict(kinds=[s.hip_operator_kind(k) for k in range(s.nblk)], images=[s.hip_block_image(k) for k in range(s.nblk)],
                     persist=s.hip_persist_stats()["iterations"] - p0, launches=s.hip_launch_count() - n0, calls=len(calls),
                     ranks=[s.block_shape(k)[1] for k in range(s.nblk)], stops=stops, counts=counts, persist_calls=persist_calls,
                     stats=s.hip_persist_stats(), plan=s.hip_persist_plan(), dense=[s.hip_dense_plan(k) for k in range(s.nblk)],
                     graph=s.hip_graph_stats(), layouts=[s.hip_cw_layout(k) for k in range(s.nblk)])
        if stamps:
            word = s.hip_persist_stamps(False)[15]
            facts["l2"] = (word >> 1) & 3 if word & 1 else None  # bit 0: granules through the XCD's L2, bit 1: factor rows too
        print(name, env, "worst", {k: "%.2e" % v for k, v in worst.items()}, "counts", counts, "stops at", stops,
              "kinds", facts["kinds"], "launches", facts["launches"], "persist", facts["persist"])
        return facts, worst
    finally:
        s.close()


def _check(worst, group="default"):
    b = BOUNDS[group]
    assert worst["factors"] <= b and worst["vectors"] <= b and worst["scalars"] <= b, (group, worst)


CW = "k_cw+k_spmm_ell"


# ---- kind 4: k_front_cw + k_wsum + k_spmm_ell, iteration 0's update in k_spmm_ell (CG0) and as k_cg_update (LORADS_FUSE_CG0=0).
# hub8 / hub16: rows 0-2 hold 40 / 60 slots, so the CSR tails of k_front_cw and k_spmm_ell run at slot width 8 / 16, and the last
# workgroup of the front holds rows past n (810 rows).  wide60: ten times more constraints than rows, every row over 16 slots, and
# more constraint values than k_spmm_ell has threads (the CG0 form's grid-stride w_acc loop).  These cases found the front's lanes
# of rows past n writing row 0's tail contributions, racing row 0's own lanes (k_front_cw: now bounded by the row's activity).
@pytest.mark.parametrize("name,env,width,schedule", [
    ("rand120", {"LORADS_OP_CW": "1"}, 8, FULL),
    ("hub8", {"LORADS_OP_CW": "1"}, 8, FULL),
    ("hub16", {"LORADS_OP_CW": "1"}, 16, FULL),
    ("wide60", {"LORADS_OP_CW": "1"}, 16, FULL),
    ("rand4000", {}, 16, SHORT),
    ("rand20000", {}, 16, HEADLINE),
])
def test_one_kernel_front_cones_fused_and_separate_iteration_zero(built, name, env, width, schedule):
    fused, wf = run_case(name, env, schedule=schedule)
    sep, ws = run_case(name, dict(env, LORADS_FUSE_CG0="0"), schedule=schedule)
    for facts in (fused, sep):
        assert facts["kinds"] == [CW], facts["kinds"]
        assert facts["images"][0]["front_cw"] == 1 and facts["images"][0]["slot_width"] == width, facts["images"][0]
    # the CG0 form really ran: one launch fewer per solve that reached iteration 0's update
    assert fused["launches"] < sep["launches"], (fused["launches"], sep["launches"])
    _check(wf)
    _check(ws)


# ---- kinds 0 / 1 (Gram form / k_sval), kind 2 (Max-Cut diagonal, one launch and launch by launch), kind 3 (+32: bipartite), dense
@pytest.mark.parametrize("name,env,want", [
    ("rand120", {"LORADS_OP_CW": "0"}, "k_pairdots+k_sgram+k_spmm2"),
    ("theta30", {}, None),
    ("maxcut100", {}, "k_op_diag"),
    ("maxcut100", {"LORADS_PERSIST": "0"}, "k_op_diag"),
    ("blk4x60", {}, "k_op_diag"),
    ("blk4x60", {"LORADS_PERSIST": "0"}, "k_op_diag"),
    ("matcomp60", {}, "k_op_entry_bip+k_op_entry_bip"),
    ("matcomp60", {"LORADS_ENTRY_BIP": "0"}, "k_op_entry"),
    ("densea40", {}, "+k_dense_cx_b(dense A_i)"),
    ("densec40", {}, None),
])
def test_operator_forms(built, name, env, want):
    facts, worst = run_case(name, env)
    if want is not None:
        assert all(want in k for k in facts["kinds"]), facts["kinds"]
    if name == "theta30":
        assert facts["kinds"] == ["k_pairdots+k_sgram+k_spmm2"], facts["kinds"]
    if name == "densea40":
        assert facts["kinds"] == ["k_pairdots+k_cv+k_sval+k_spmm2+k_dense_cx_b(dense A_i)"], facts["kinds"]
    if name == "densec40":
        assert facts["images"][0]["dense_c"] == 1, facts["images"][0]
        _check(worst)
        return
    if name.startswith(("maxcut", "blk4x60")):
        # the one-launch ADMM iteration of Max-Cut-type cones ran for every step (default) / never (LORADS_PERSIST=0)
        if env.get("LORADS_PERSIST") == "0":
            assert facts["persist"] == 0
        else:
            assert facts["persist"] > 0, facts
    _check(worst)


def test_worse_conditioned_gram_cone(built):
    """theta50 (Lovasz theta, m = 104): the CG amplifies rounding most here; kind 1 (k_sval) is covered by densea40 above"""
    facts, worst = run_case("theta50", {"LORADS_OP_CW": "0"}, seed=6)  # (seed 5 offers one stopping iteration only)
    assert facts["kinds"] == ["k_pairdots+k_sgram+k_spmm2"], facts["kinds"]
    _check(worst)


# ---- other contexts: merged lockstep sweep, the LP block, the convergence test in launches of its own, sharded forms on one rank
@pytest.mark.parametrize("name,env", [("mix4", {}), ("blkmix5", {"LORADS_COMMON_RANK": "1"})])
def test_merged_lockstep_sweeps(built, name, env):
    facts, worst = run_case(name, env)
    # the merged view really ran: the same schedule cone by cone (LORADS_NO_MERGE=1) takes more launches
    alone, worst_alone = run_case(name, dict(env, LORADS_NO_MERGE="1"))
    assert facts["launches"] < alone["launches"], (facts["launches"], alone["launches"])
    _check(worst)
    _check(worst_alone)


@pytest.mark.parametrize("name", ["sdplp40", "coupledlp"])
def test_lp_block(built, name):
    """the LP block is the model's closed form per column (no CG: the exact counts would differ if it ran one)"""
    facts, worst = run_case(name)
    assert AdmmModel.from_file(_path(name)).cones[-1].is_lp and facts["ranks"][-1] == 1, facts["ranks"]
    _check(worst)


@pytest.mark.parametrize("name,env,separable,hook", [
    ("rand120", {"LORADS_OP_CW": "1", "LORADS_LAZY_SCALARS": "0"}, None, False),
    ("maxcut100", {"LORADS_PERSIST": "0", "LORADS_LAZY_SCALARS": "0"}, None, False),
    ("rand120", {"LORADS_OP_CW": "1"}, False, True),
    ("blk4x60", {}, True, True),
])
def test_other_contexts(built, name, env, separable, hook):
    facts, worst = run_case(name, env, separable=separable, hook=hook)
    if hook:
        assert facts["calls"] > 0, "the hook was never called: not the sharded path"
    if env.get("LORADS_LAZY_SCALARS") == "0":  # (the convergence test in k_cg_check launches of its own: more launches)
        assert facts["launches"] > run_case(name, {k: v for k, v in env.items() if k != "LORADS_LAZY_SCALARS"})[0]["launches"]
    _check(worst)


# ---- the row-kernel dispatch of the rank (lg_for, use_v2, NS_SWITCH) on one kind-4 and one kind-2 cone; odd ranks unpadded too
RANK_LIST = [2, 8, 40, 41, 64, 66, 127, 128, 130, 200]


@pytest.mark.parametrize("name,env,want", [("rand4000", {}, CW), ("maxcut800", {}, "k_op_diag")])
@pytest.mark.parametrize("r", RANK_LIST)
def test_rank_dispatch(built, name, env, want, r):
    envs = [env] + ([dict(env, LORADS_PAD_ODD_RANK="0")] if r % 2 else [])
    for e in envs:
        facts, worst = run_case(name, e, params=dict(timesLogRank=0.1), schedule=RANKS, ranks=r)
        assert facts["ranks"] == [r] and facts["kinds"] == [want], facts
        _check(worst)


def test_recurrence_across_the_exact_refresh(built):
    """33 sweeps at maxit 1 on a small cone whose constraint values are kept by recurrence (k_cw): the constraint sums at every
    sweep, across the exact refresh of every 32nd sweep"""
    facts, worst = run_case("rand120", {"LORADS_OP_CW": "1"}, schedule=[("sweep", 1, 0.0)] * 33)
    assert facts["kinds"] == [CW]
    _check(worst)
