"""CG solves that stop on their initial residual (CGSolve's first exit: done = 2, the solve does nothing), in every operator form and
launch-saving variant, against the extended-precision model (tests/admm_model.py).

tests/test_fixed_count_sweeps.py and its siblings exclude that exit by construction (stopping_tol rejects every tolerance a solve may
pass at once).  The exit is written once per way of starting a solve -- k_cg_init and its copies on carrier kernels, the head of
k_op_diag, k_cg_init_seg, the one-launch iteration, k_cw with a solve's start on board, the closed gate of k_cg_update, the CG0 form
of k_spmm_ell -- and the host has behaviour of its own behind it: finish_sweep returns the cone's previous count for such a solve
(DESIGN.md section 5, Q7), the speculation history records 0, and a front enqueued ahead is adopted only while that history holds
an iteration.  A wrong row store, a missed constraint refresh or a wrong average there would show as slower convergence only.

The inputs are the model's alone (admm_model.pattern_tol, solved_state): tolerance 0.5, which every solve of these states passes;
factors that already hold a converged solve, whose residual is rounding; tolerances at which the U-solves iterate and the V-solves
behind them pass.  run_case (tests/test_fixed_count_sweeps.py) checks after every sweep: the returned count against the model's
(exact, stale counts included), U and V bit for bit against what the device held for every solve the model says passed, every other
factor, the device's constraint sums against A(.) of its own factors, lambda and the step's scalars within BOUNDS["default"].  Every
case asserts from the model's log that solves really passed at once and others really ran, and that its form really ran.

Bound 1e-12 relative to scale (BOUNDS["default"]).  Measured on the MI355X, worst over the cases of an instance (factors / m-vectors /
scalars), and per-solve counts that ran (U, V per cone; P is (0,..), (0,..), (24,..), (0,..) everywhere, returned 0, 0, 48, 48 per cone):

    rand120    1.6e-15 / 1.9e-15 / 4.1e-16   UV (0,3) (3,2) -> 3, 5     VU (1,0) (0,0) -> 2, 2
               SPEC (0,0) x 6, (3,1), (2,0), (6,3) -> 0 x 6, 4, 4, 9
    hub16      6.0e-15 / 2.6e-15 / 2.3e-16   UV (0,3) (3,2)             VU (1,0) (0,0)
    theta30    2.4e-15 / 6.8e-15 / 8.3e-16   UV (0,6) (1,1) -> 6, 2     VU (1,0) (0,0)
    densea40   1.7e-15 / 1.0e-15 / 3.7e-16   UV (0,3) (3,2)             VU (1,0) (0,0)
    densec40   7.0e-16 / 1.2e-15 / 8.3e-16   UV (0,3) (3,3)             VU (2,0) (0,0) -> 4, 4
    maxcut100  1.5e-15 / 1.2e-15 / 4.9e-16   UV (0,3) (3,1) -> 3, 4     VU (1,0) (0,0)     SPEC ... (3,2), (3,2), (3,1) -> 5, 5, 4
    blk4x60    1.3e-15 / 1.1e-15 / 2.0e-16   UV (0,5,0,6,0,5,0,6) (3,1,4,1,3,1,3,1) -> 22, 17   MIX (0,2,3,2,0,2,3,2) (0,..) -> 14, 16
    matcomp60  4.0e-15 / 9.2e-16 / 3.8e-16   UV (0,3) (3,1)             VU (1,0) (0,0)
    mix4       6.2e-15 / 2.5e-15 / 3.6e-14   UV (0,3,0,8,0,3,0,6) (3,1,7,3,2,1,4,2) -> 20, 23
               MIX1 (0,1,8,3,0,1,1,2) (0,..) (0,0,1,0,0,0,0,0) (0,..) -> 16, 14, 10, 10
    blkmix5    1.6e-15 / 5.9e-16 / 1.8e-16   UV (0,5,0,6,0,5,0,5,0,5) (6,3,6,3,6,3,6,2,6,2) -> 26, 43
               MIX1 (0,5,5,6,0,5,4,5,5,5) (0,..) (1,0,0,0,0,0,0,0,0,0) (0,..) -> 40, 52, 44, 44
    sdplp40    6.8e-16 / 7.3e-16 / 1.9e-16   UV (0,3) (3,1)             VU (1,0) (0,0)
    coupledlp  2.9e-15 / 2.1e-15 / 4.3e-16   UV (0,3,0,3) (3,0,6,0) -> 6, 18   VU (1,0,0,0) (0,0,0,0) -> 2, 2

The file's 68 cases run 13.5 s on one MI355X."""
import pytest

from tests.admm_model import RUN
from tests.test_fixed_count_sweeps import CW, Want, _check, run_case

pytestmark = pytest.mark.gpu

STOPS = (3, 4, 5, 6, 2, 7, 8, 1)
ALL_PASS = 0.5  # (every solve of these states starts below 0.16 ||b||_1; the model decides, and every case asserts what it said)

# P: nothing but the LP columns moves in entries 0, 1 and 3; entry 3 adds the stale counts of entry 2 (24 per solve)
P = [("sweep", 30, ALL_PASS), ("step", 30, ALL_PASS), ("step", 24, 0.0), ("sweep", 30, ALL_PASS)]
# UV: U holds the converged U-solve: it passes, the V-solves run and one is stopped at a clear j; then V holds the converged V-solve
# for a U loaded at random: the U-solves run, and what the V-solves then do the model decides
UV = [("load", dict(solve="U")), ("step", 30, Want(0, RUN, stops=STOPS)),
      ("load", dict(solve="V", seed=6)), ("step", 30, Want(RUN, None, stops=STOPS))]
# VU: the U-solves iterate and the V-solves behind them pass (behind one fixed sweep where the seeded state has no such tolerance);
# the all-pass step behind it adds every cone's latest count twice more
VU = [("sweep", 1, 0.0, "unless found"), ("sweep", 30, Want(RUN, 0, each="free")), ("step", 30, ALL_PASS)]
# MIX: cones 0 and 2 solved, the others not: solves that pass and solves that run side by side in one lockstep sweep / one launch;
# MIX1: then, from the seeded state, a tolerance at which one cone's U-solve iterates while every other solve passes (cones of one
# kind and size, as blk4x60's, have no such tolerance)
MIX = [("load", dict(solve="U", cones=(0, 2))), ("step", 30, Want(0, RUN, cones=(0, 2), other=RUN, stops=STOPS)), ("step", 30, ALL_PASS)]
MIX1 = MIX + [("load", dict(solve="U", cones=())), ("sweep", 30, Want(RUN, 0, other=0, each="other")), ("step", 30, ALL_PASS)]
# SPEC: six all-pass steps fill the speculation window (4) with zeros; the next step needs j >= 3 iterations with none enqueued
# and completes through the resume path; two more steps
SPEC = [("step", 30, ALL_PASS)] * 6 + [("step", 30, Want(RUN, None, stops=(3, 4, 5, 6, 7, 8)))] + [("step", 30, Want(RUN, None, stops=STOPS))] * 2
SCHEDULES = dict(P=P, UV=UV, VU=VU, MIX=MIX, MIX1=MIX1, SPEC=SPEC)


def _zeros(facts, i):
    return all(c == 0 for c in facts["solves"][i])


def check_exits(name, which, facts):
    """what the model's log must show for the schedule to test anything: solves that passed at once, and solves that ran"""
    sv, counts = facts["solves"], facts["counts"]
    ncg = len(sv[0]) // 2
    if which == "P":
        assert _zeros(facts, 0) and _zeros(facts, 1) and _zeros(facts, 3), (name, sv)
        assert sv[2] == (24,) * (2 * ncg) and counts == [0, 0, 48 * ncg, 48 * ncg], (name, counts)
    elif which == "UV":
        assert sv[0][0] == 0 and all(c >= 1 for c in sv[0][1::2]), (name, sv)   # cone 0's solved U passed, every V-solve ran
        assert all(c >= 1 for c in sv[1][0::2]), (name, sv)                      # the mirror: every U-solve ran
    elif which == "VU":
        run, stale = sv[-2], sv[-2][0::2]
        assert any(run[2 * k] >= 1 and run[2 * k + 1] == 0 for k in range(ncg)), (name, sv)
        assert _zeros(facts, -1), (name, sv)
        assert any(stale) and counts[-1] >= 2 * max(stale), (name, counts, sv)
    elif which in ("MIX", "MIX1"):
        assert sv[0][0] == 0 and sv[0][4] == 0 and sv[0][2] >= 1 and sv[0][6] >= 1 and all(c >= 1 for c in sv[0][1::2]), (name, sv)
        assert _zeros(facts, 1) and counts[1] == 2 * sum(sv[0][1::2]), (name, sv, counts)   # (each cone's V-solve was its latest)
        if which == "MIX1":
            assert sorted(sv[2])[-1] >= 1 and sorted(sv[2])[-2] == 0, (name, sv)   # one solve iterated, every other passed
            assert _zeros(facts, 3), (name, sv)
    elif which == "SPEC":
        assert all(_zeros(facts, i) for i in range(6)) and max(sv[6]) >= 3 and sv[6][0] >= 1, (name, sv)
    if facts["lp_moved"]:  # the LP block has no CG and adds no count; its columns are updated in an all-pass sweep all the same
        assert all(d > 0 for d in facts["lp_moved"]), (name, facts["lp_moved"])


def run(name, which, env=None, **kw):
    facts, worst = run_case(name, env, schedule=SCHEDULES[which], **kw)
    check_exits(name, which, facts)
    _check(worst)
    return facts


# ---- kind 4: k_front_cw + k_wsum + k_spmm_ell; iteration 0's update in k_spmm_ell (CG0: it must not be applied for a solve that
# passed) and as k_cg_update (its closed gate still leaves the average); k_cw with a solve's start on board; the convergence test in
# launches of its own (LORADS_LAZY_SCALARS=0).  hub16: CSR tails, the front's last workgroup past n
@pytest.mark.parametrize("which", ["P", "UV", "VU"])
@pytest.mark.parametrize("name,width", [("rand120", 8), ("hub16", 16)])
def test_one_kernel_front_cones(built, name, width, which):
    env = {"LORADS_OP_CW": "1"}
    fused = run(name, which, env)
    sep = run(name, which, dict(env, LORADS_FUSE_CG0="0"))
    for facts in (fused, sep):
        assert facts["kinds"] == [CW], facts["kinds"]
        assert facts["images"][0]["front_cw"] == 1 and facts["images"][0]["slot_width"] == width, facts["images"][0]
    # the CG0 form really ran: one launch fewer per solve that reached iteration 0's update
    assert fused["launches"] < sep["launches"], (fused["launches"], sep["launches"])
    if name == "rand120":
        for e, other in ((env, fused), (dict(env, LORADS_FUSE_CG0="0"), sep)):
            eager = run(name, which, dict(e, LORADS_LAZY_SCALARS="0"))
            assert eager["kinds"] == [CW] and eager["launches"] > other["launches"], (eager["launches"], other["launches"])


# ---- kinds 0 / 1 (Gram form / k_sval) and the dense forms
@pytest.mark.parametrize("which", ["P", "UV", "VU"])
@pytest.mark.parametrize("name,env,want", [
    ("rand120", {"LORADS_OP_CW": "0"}, ["k_pairdots+k_sgram+k_spmm2"]),
    ("theta30", {}, ["k_pairdots+k_sgram+k_spmm2"]),
    ("densea40", {}, ["k_pairdots+k_cv+k_sval+k_spmm2+k_dense_cx_b(dense A_i)"]),
    ("densec40", {}, None),
])
def test_gram_and_dense_forms(built, name, env, want, which):
    facts = run(name, which, env)
    if want is not None:
        assert facts["kinds"] == want, facts["kinds"]
    if name == "densec40":
        assert facts["images"][0]["dense_c"] == 1, facts["images"][0]


# ---- kind 2 (Max-Cut diagonal): the one-launch iteration (its own exit, and its row stores behind it) and launch by launch (the
# head of k_op_diag); an odd rank as it is; kind 3 (single-entry constraints), bipartite and plain
@pytest.mark.parametrize("which", ["P", "UV", "VU"])
@pytest.mark.parametrize("name,env,ranks,want", [
    ("maxcut100", {}, None, "k_op_diag"),
    ("maxcut100", {"LORADS_PERSIST": "0"}, None, "k_op_diag"),
    ("maxcut100", {"LORADS_PAD_ODD_RANK": "0"}, 5, "k_op_diag"),   # (from the rank timesLogRank 0.1 gives: a rank only grows)
    ("blk4x60", {}, None, "k_op_diag"),
    ("blk4x60", {"LORADS_PERSIST": "0"}, None, "k_op_diag"),
    ("matcomp60", {}, None, "k_op_entry_bip+k_op_entry_bip"),
    ("matcomp60", {"LORADS_ENTRY_BIP": "0"}, None, "k_op_entry"),
])
def test_diagonal_and_entry_forms(built, name, env, ranks, want, which):
    facts = run(name, which, env, ranks=ranks, params=dict(timesLogRank=0.1) if ranks else None)
    assert all(want in k for k in facts["kinds"]), facts["kinds"]
    if ranks is not None:
        assert facts["ranks"] == [ranks], facts["ranks"]
    if want == "k_op_diag":
        if env.get("LORADS_PERSIST") == "0" or env.get("LORADS_PAD_ODD_RANK") == "0":  # (persist_eligible: even device ranks only)
            assert facts["persist"] == 0
        else:  # every sweep of the schedule, the all-pass ones included, was one launch
            assert all(c == 1 for c in facts["persist_calls"]), facts["persist_calls"]


# ---- contexts of several cones: the merged lockstep sweep (mix4: cones of three kinds) and the one-launch iteration of several
# Max-Cut cones (blkmix5), with cones that pass and cones that run side by side (MIX)
@pytest.mark.parametrize("which", ["P", "UV", "MIX1"])
@pytest.mark.parametrize("name,env", [("mix4", {}), ("blkmix5", {"LORADS_COMMON_RANK": "1"})])
def test_several_cones_side_by_side(built, name, env, which):
    facts = run(name, which, env)
    alone = run(name, which, dict(env, LORADS_NO_MERGE="1"))
    # the merged view really ran: the same schedule cone by cone takes more launches
    assert facts["launches"] < alone["launches"], (facts["launches"], alone["launches"])
    if name == "blkmix5":
        assert all(c == 1 for c in facts["persist_calls"]), facts["persist_calls"]
    if name == "mix4":
        # cone by cone with the merged cone in place: the library reads LORADS_NO_BATCH at every sweep, not when the context is made
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("LORADS_NO_BATCH", "1")
            batchless = run(name, which, dict(env, LORADS_NO_BATCH="1"))
        assert facts["launches"] < batchless["launches"], (facts["launches"], batchless["launches"])
        # (no statistic shows where the solves' start ran: the per-cone scalar kernels are not among the counted launches)
        run(name, which, dict(env, LORADS_SEG_CARRY_INIT="0"))


@pytest.mark.parametrize("which", ["P", "UV", "MIX"])
def test_lockstep_start_of_the_solves_as_its_own_launch(built, which):
    """k_cg_init_seg rides on iteration 0's operator kernel only where the merged cone is of Max-Cut type and an iteration is
    enqueued (blk4x60 launch by launch): there as a launch of its own (LORADS_SEG_CARRY_INIT=0), and carried.  In the all-pass
    sweeps no iteration is enqueued once the window is all zero, and the kernel runs alone in either form."""
    env = {"LORADS_PERSIST": "0"}
    carried = run("blk4x60", which, env)
    own = run("blk4x60", which, dict(env, LORADS_SEG_CARRY_INIT="0"))
    assert carried["persist"] == 0 and own["persist"] == 0 and all("k_op_diag" in k for k in carried["kinds"] + own["kinds"])


# ---- sharded forms on one rank (the all-reduce hook), and the LP block behind cones whose solves pass
@pytest.mark.parametrize("which", ["P", "UV", "VU"])
@pytest.mark.parametrize("name,env,separable", [("rand120", {"LORADS_OP_CW": "1"}, False), ("blk4x60", {}, True)])
def test_sharded_forms_on_one_rank(built, name, env, separable, which):
    facts = run(name, which, env, separable=separable, hook=True)
    assert facts["calls"] > 0, "the hook was never called: not the sharded path"


@pytest.mark.parametrize("which", ["P", "UV", "VU"])
@pytest.mark.parametrize("name", ["sdplp40", "coupledlp"])
def test_lp_block_behind_solves_that_pass(built, name, which):
    facts = run(name, which)
    assert facts["ranks"][-1] == 1 and facts["levels"][-1] and len(facts["lp_moved"]) >= 2, facts["ranks"]


# ---- the host behind an immediate exit: the speculation history records 0, nothing is enqueued for a solve whose window is all
# zero, and a front enqueued ahead is adopted only while B.spec[0] >= 1 (spec_front_adopt)
def _in_flight(st):
    return st["enqueued"] - st["adopted"] - st["discarded"] - st["blocked"]


@pytest.mark.parametrize("name,env", [
    ("rand120", {"LORADS_OP_CW": "1"}),
    ("rand120", {"LORADS_OP_CW": "1", "LORADS_SPEC_FRONT": "0"}),
    ("rand120", {"LORADS_OP_CW": "1", "LORADS_HANDOVER_ON_FRONT": "0"}),
    ("rand120", {"LORADS_OP_CW": "1", "LORADS_GRAPH": "0"}),
    ("rand120", {"LORADS_OP_CW": "1", "LORADS_GRAPH": "0", "LORADS_SPEC_FRONT": "0"}),
    ("rand120", {"LORADS_OP_CW": "1", "LORADS_GRAPH": "0", "LORADS_HANDOVER_ON_FRONT": "0"}),
    ("maxcut100", {"LORADS_PERSIST": "0"}),
    ("mix4", {}),
])
def test_speculation_behind_all_pass_steps(built, name, env):
    """SPEC twice: with the device's state read after every step (all of run_case's checks; every read discards a front in flight),
    and read at the end only -- the plain loop admm_step, update_dual_var, in which a front enqueued ahead stays in flight.

    The counters are asserted from the code's rules.  The speculated count of a solve is the largest of its last 4 (the history
    starts as 1, 1, 1, 1; a solve that passed records 0), so: before step i the U-solve's is 1 for i = 1, 2, 3 and 0 for i = 4, 5, 6;
    a step with 0 adopts nothing and discards the front in flight; step 6 finds no iteration enqueued, resumes, and blocks the front
    enqueued behind it.  A front is enqueued at all only for one one-kernel-front cone whose steps go launch by launch
    (spec_front_ok; a context this small replays its steps as captured chains unless LORADS_GRAPH=0, and a chain has its own)."""
    read = run(name, "SPEC", env, probe=True)
    misses = [p["misses"] for p in read["probes"]]
    assert misses[5] == 0, (name, "an all-pass step resumed a solve", misses)
    assert misses[6] >= 1, (name, "the step behind a window of zeros completed without the resume path", misses)
    plain = run(name, "SPEC", env, probe=True, reads=False)
    assert plain["solves"] == read["solves"] and plain["counts"] == read["counts"]
    assert plain["misses"] == read["misses"], (plain["misses"], read["misses"])   # (what is enqueued does not depend on the reads)
    st = [dict(enqueued=0, adopted=0, discarded=0, blocked=0)] + [p["front"] for p in plain["probes"]]
    print(name, env, "front statistics per step", [tuple(s.values()) for s in st[1:]], "misses", misses)
    fronts = name == "rand120" and env.get("LORADS_SPEC_FRONT") != "0"
    if name == "rand120":
        assert plain["kinds"] == [CW] and (plain["graph"]["enabled"] == 0) == (env.get("LORADS_GRAPH") == "0"), plain["graph"]
    # a step is replayed (graph_this_step) unless its parameters and those of the step before it both differ from their predecessors'
    par = plain["params"]
    changed = [i > 0 and par[i] != par[i - 1] for i in range(len(par))]
    by_launch = [not plain["graph"]["enabled"] or (changed[i] and changed[i - 1]) for i in range(len(par))]
    for i in range(len(SPEC)):
        b, a = st[i], st[i + 1]
        d = {k: a[k] - b[k] for k in a}
        assert 0 <= _in_flight(a) <= 1 and 0 <= d["enqueued"] <= 1, (i, st)
        if not (fronts and by_launch[i]):
            assert d["enqueued"] == 0, ("a front was enqueued behind a step that cannot have one", i, st)
        if 4 <= i <= 6 or not by_launch[i]:  # the U-solve's last four counts are all zero / a replayed chain has its own front
            assert d["adopted"] == 0 and d["discarded"] == _in_flight(b), ("a front was adopted with no iteration enqueued", i, st)
        if i < 6:
            assert d["blocked"] == 0, (i, st)
        if i == 6:
            assert d["blocked"] == d["enqueued"], ("the front behind a step that resumed was not blocked", i, st)
    if not (fronts and all(by_launch)):
        return
    assert all(st[i + 1]["enqueued"] - st[i]["enqueued"] == 1 for i in range(7)), st
    assert st[4]["adopted"] >= 1, ("no front was adopted while the window still held an iteration", st)
    assert st[4]["adopted"] == st[7]["adopted"], st
