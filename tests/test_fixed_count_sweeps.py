"""Fixed-count ADMM sweeps of every operator form against the extended-precision model (tests/admm_model.py).

A truncated CG is a fixed rational function of its inputs: after exactly K iterations (tol 0), or stopped by a tolerance that the
model's residual history puts between two clearly different residuals, no iteration count and no tolerance is left to absorb an error
of the device.  Each case sets a seeded state (set_mat / set_vec, init_constr(PAIR_UV)), runs a schedule of sweeps with the dual update
between them on the device and on the model, and checks after every sweep: U and V per cone, the CG count exactly, the device's
constraint sums against A(U V^T) formed by the model from the device's OWN factors (so a missed step of the recurrence that keeps them
shows apart from CG rounding), lambda, and the step's pObj, dObj and err1.  Every case also checks that its form really ran
(operator kind, block image, one-launch statistics, launch counts): a case that silently falls back tests nothing.

No solve of these schedules passes on its initial residual (stopping_tol excludes such tolerances): that exit of the CG, the count it
returns and what the host does behind it are pinned by tests/test_immediate_exits.py, through the same run_case (schedule entries
that load a solved state, and tolerances asked of the model's pattern search, see Want).

Bounds: relative to the vector's largest entry (dObj: to ||b||_1 max |lambda|), at most 100x the worst error measured on the MI355X
per group of cases and never above 1e-11 (factors, constraint sums); the measured figure stands next to each bound."""
import os

import numpy as np
import pytest

from lorads_amd import host
from tests import common
from tests.admm_model import RUN, AdmmModel, lp_levels, passed_at_once, pattern_tol, solved_state, stopping_tol

pytestmark = pytest.mark.gpu

RHO = 1.5
# worst rel-to-scale error measured on the MI355X over all cases of a group (factors / m-vectors / scalars), and its bound
BOUNDS = {
    "default": 1e-12,  # measured 1.5e-13 (theta30, constraint sums); theta50 1.6e-13, hub16 1.4e-14, every other case <= 1e-14
    # (the variants of the one-launch iteration, tests/test_one_launch_variants.py: this cap and below it max(32 x the spread of the
    # model in float64, 1e-14) per case; measured <= 1.3e-14 (n = 4128, factors), every other case <= 4.9e-15)
    # (solves that pass on their initial residual, tests/test_immediate_exits.py: measured <= 6.8e-15 (theta30, constraint sums),
    # scalars <= 3.6e-14 (mix4, pObj))
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


class Want:
    """the tolerance of a schedule entry, asked of the model's pattern search (admm_model.pattern_tol) at the state the entry starts
    from: u, v -- what the U- and the V-solve of the cones in `cones` (None: every cone with a CG) are to do: 0 = pass on the initial
    residual, RUN = iterate, None = whatever the model says; the solves of the other cones: `other`.  A U-solve is asked to pass
    only where the cone's constraints touch no earlier cone (elsewhere an earlier solve moves its right-hand side: None).
    stops: some solve marked RUN is stopped after exactly j iterations, for the first j of the tuple that has a tolerance.
    each: "free" -- where no tolerance shows the pattern on all cones together, the first cone for which one shows it, the others
    doing whatever the model says; "other" -- the first cone k for which a tolerance shows (u, v) on k and `other` on the rest."""

    def __init__(self, u, v, cones=None, other=None, stops=None, each=False):
        self.u, self.v, self.cones, self.other, self.stops, self.each = u, v, cones, other, stops, each

    def __repr__(self):
        return "Want(%r, %r, %r, %r, %r, %r)" % (self.u, self.v, self.cones, self.other, self.stops, self.each)

    def pattern(self, model, cones):
        out = []
        for k, cn in enumerate(model.cones):
            if cn.is_lp:
                continue
            u, v = (self.u, self.v) if cones is None or k in cones else (self.other, self.other)
            if u == 0 and any(np.intersect1d(cn.cons, model.cones[j].cons).size for j in range(k)):
                u = None
            out += [u, v]
        return out

    def find(self, model, maxit):
        """(tol, per-solve counts) or None"""
        ncg = [k for k, cn in enumerate(model.cones) if not cn.is_lp]
        for cones in ([] if self.each == "other" else [self.cones]) + ([(k,) for k in ncg] if self.each else []):
            pat = self.pattern(model, cones)
            if cones is not self.cones and self.each == "free":
                pat = [x if t // 2 == ncg.index(cones[0]) else None for t, x in enumerate(pat)]
            for j in self.stops or (None,):
                found = pattern_tol(model, RHO, maxit, pat, stop=j)
                if found:
                    return found
        return None


# what the model alone decides for a case -- a Want's tolerance, a solved state -- does not depend on the device's switches: found
# once per (instance, ranks, seed, what the schedule did so far) and shared by the cases that differ in their env only
_plans = {}


def _memo(key, make):
    if key not in _plans:
        _plans[key] = make()
    return _plans[key]


def solved_uv_state(s, model, spec, seed):
    """the state of a ("load", spec) entry: U, V, lambda seeded as random_uv_state (spec["seed"], default: the case's), with the
    U (spec["solve"] == "U"; "V": the V) of the cones spec["cones"] (None: all) replaced by the converged solve for the other"""
    import copy
    U, V, lam = common.random_uv_state(s, spec.get("seed", seed))
    probe = copy.deepcopy(model)
    probe.set_state(U, V, lam)
    U, V = solved_state(probe, RHO, spec.get("cones"), 0 if spec["solve"] == "U" else 1)
    return U, V, lam


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
             stamps=False, spread=False, reads=True, probe=False):
    """runs the schedule on the device and the model; returns (session facts, worst errors by group).
    path: the instance's file where `name` is no named one.  A schedule entry may carry a fourth field "fixed": its maxit stays
    what it says whatever tolerance the model finds (the tolerance is then looked for among the first iterations only, and every
    solve of the sweep must stop by it).  tag: the one-launch form's next tag (lorads_hip_persist_set_tag), set once its plan
    exists.  stamps: the one-launch form's stamps are on for the schedule and facts["l2"] holds what its latest launch decided
    (lorads_hip_persist_stamps, word 15; None: no such launch).  spread: the same schedule also runs on the model in float64 and
    worst["spread"] is the largest difference between the two models over every compared quantity (what the reference's own
    arithmetic leaves open: a bound taken from it owes nothing to the device).

    Immediate exits (tests/test_immediate_exits.py): an entry ("load", spec) loads a solved state into the device and the model
    (solved_uv_state); a tolerance may be a Want, answered by the model's pattern search -- no tolerance fails the case; an entry
    whose fourth field is "unless found" runs only where the NEXT entry's Want has no tolerance at the state before it.  After
    every sweep the factor of every solve that the model says passed on its initial residual must be bit for bit what the device
    held before.  facts["solves"]: the model's per-solve counts of every sweep; facts["lp_moved"]: the smallest change of an LP
    column per sweep; facts["params"]: (tolerance, iteration limit) of every sweep.  reads=False: the device's factors and vectors are read after the last entry only (every read between two
    steps discards a front enqueued ahead, and so does every statistic but the fronts' own: facts["persist_calls"] stays empty);
    counts and scalars are still compared per entry.  probe: facts["probes"] holds per
    entry the front statistics (and, with reads, the speculation misses so far)."""
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
        key0 = (path, tuple(s.block_shape(k)[1] for k in range(s.nblk)), seed)
        trail = []  # what the schedule has done so far, as the key of what the model decides next
        held = [[np.array(u) for u in U], [np.array(v) for v in V]]  # the device's factors as loaded or last read
        moved = [[False] * s.nblk, [False] * s.nblk]  # has a solve (or the LP sweep) changed the factor since?
        solves, lp_moved, probes, params_used = [], [], [], []
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
            if entry[0] == "load":
                U, V, lam = _memo((key0, tuple(trail), repr(entry)), lambda: solved_uv_state(s, model, entry[1], seed))
                common.load_uv_state(be, U, V, lam)
                for mdl in (model, m64) if m64 is not None else (model,):
                    mdl.set_state(U, V, lam)
                held = [[np.array(u) for u in U], [np.array(v) for v in V]]
                moved = [[False] * s.nblk, [False] * s.nblk]
                trail.append(repr(entry))
                continue
            kind, maxit, tol = entry[:3]
            fixed = len(entry) > 3 and entry[3] == "fixed"
            if len(entry) > 3 and entry[3] == "unless found":
                nxt = schedule[i + 1]
                if _memo((key0, tuple(trail), repr(nxt)), lambda: nxt[2].find(model, nxt[1])):
                    continue
            pnow = s.hip_persist_stats()["iterations"] if reads else 0  # (every statistic but the fronts' own discards a front in flight)
            if isinstance(tol, tuple):
                tol, maxit = find_stop(model, name, i, tol, maxit, fixed, stops)
            elif isinstance(tol, Want):
                found = _memo((key0, tuple(trail), repr(entry)), lambda: tol.find(model, maxit))
                assert found, (name, i, "the model finds no tolerance that shows the pattern", tol)
                tol = found[0]
            trail.append(repr(entry))
            params_used.append((tol, maxit))
            if kind == "sweep":
                its = be.admm_update_var(RHO, tol, maxit)
                mits, log = model.sweep(RHO, tol, maxit)
            else:
                its, p, d, e = be.admm_step(RHO, tol, maxit)
                mits, mp, md, me, log = model.step(RHO, tol, maxit)
                dscale = float(np.sum(np.abs(model.b)) * np.max(np.abs(model.lam)))
                for lbl, x, y, sc in (("pObj", p, mp, 1.0), ("dObj", d, md, dscale), ("err1", e, me, 0.0)):
                    err = abs(x - float(y)) / max(abs(float(y)), sc, 1e-300)
                    worst["scalars"] = max(worst["scalars"], err)
            counts.append(its)
            if reads:
                persist_calls.append(s.hip_persist_stats()["iterations"] - pnow)
            solves.append(tuple(x[2] for x in log))
            assert its == mits, (name, i, "CG iterations", its, mits, solves[-1])
            for k, half, it, hist in log:
                moved[half][k] = moved[half][k] or not passed_at_once(it, hist, tol)
            for k, cn in enumerate(model.cones):
                if cn.is_lp:
                    moved[0][k] = moved[1][k] = True
            if probe:
                probes.append(dict(front=s.hip_spec_front_stats()))
                if reads:
                    probes[-1]["misses"] = s.hip_profile_read()["speculation_misses"]
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
            if not reads and i < len(schedule) - 1:
                be.update_dual_var(RHO)
                model.update_dual(RHO)
                if m64 is not None:
                    m64.update_dual(RHO)
                continue
            Ud = [be.get_mat(host.MAT_U, k) for k in range(s.nblk)]
            Vd = [be.get_mat(host.MAT_V, k) for k in range(s.nblk)]
            for half, F in enumerate((Ud, Vd)):
                for k in range(s.nblk):  # a solve that passed on its initial residual has touched nothing
                    assert moved[half][k] or np.array_equal(F[k], held[half][k]), (name, i, "a solve that passed moved its factor", "UV"[half], k)
            if model.cones[-1].is_lp:
                lp_moved.append(float(min(np.min(np.abs(Ud[-1] - held[0][-1])), np.min(np.abs(Vd[-1] - held[1][-1])))))
            held, moved = [Ud, Vd], [[False] * s.nblk, [False] * s.nblk]
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
                     graph=s.hip_graph_stats(), layouts=[s.hip_cw_layout(k) for k in range(s.nblk)], solves=solves, lp_moved=lp_moved,
                     probes=probes, params=params_used, levels=[lp_levels(model, k) if cn.is_lp else None for k, cn in enumerate(model.cones)])
        if probe:
            facts["misses"] = s.hip_profile_read()["speculation_misses"]
        if stamps:
            word = s.hip_persist_stamps(False)[15]
            facts["l2"] = (word >> 1) & 3 if word & 1 else None  # bit 0: granules through the XCD's L2, bit 1: factor rows too
        print(name, env, "worst", {k: "%.2e" % v for k, v in worst.items()}, "counts", counts, "solves", solves, "stops at", stops,
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


# (columns, levels, longest level) of the LP block's level schedule, which decide the path: one level runs k_lp_sweep_flat, one
# thread per column -- sdpslack30 in one workgroup, sdpslack300 in two --; several run k_lp_sweep, one workgroup of 256 threads that
# strides over each level -- sdplp300's level 0 takes a second trip --; coupledlp_free's last column has a cost and no entry
LP_SHAPES = dict(sdplp40=(52, 4, 40), coupledlp=(18, 8, 3), sdpslack30=(30, 1, 30), sdpslack300=(300, 1, 300), sdplp300=(312, 3, 300),
                 coupledlp_free=(19, 8, 4))


@pytest.mark.parametrize("name", ["sdplp40", "coupledlp", "sdpslack30", "sdpslack300", "sdplp300", "coupledlp_free"])
def test_lp_block(built, name):
    """the LP block is the model's closed form per column (no CG: the exact counts would differ if it ran one)"""
    facts, worst = run_case(name)
    model = AdmmModel.from_file(_path(name))
    assert model.cones[-1].is_lp and facts["ranks"][-1] == 1, facts["ranks"]
    levels = facts["levels"][-1]
    assert (model.cones[-1].n, len(levels), max(levels)) == LP_SHAPES[name], (name, levels)
    if name == "coupledlp_free":
        assert not np.any(model.cones[-1].a_row == 18) and 18 in model.cones[-1].c_row  # (an empty entry range, and a cost)
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
