"""Every variant of the one-launch ADMM iteration (csrc/hip/persist.inc) against the extended-precision model (tests/admm_model.py).

The harness is run_case of tests/test_fixed_count_sweeps.py: a seeded state, a schedule of sweeps and steps with the dual update
between them on the device and on the model, and after every sweep the factors, the exact CG counts, the constraint sums, lambda,
pObj, dObj and err1.  What this module adds is the choice of cases: each is the smallest shape that reaches one of

  * the fourteen instantiations k_admm_diag<NS, ROWS> (LORADS_PERSIST_ROWS; ROWS = 4 fetches its row info again before each use),
  * the rows-per-workgroup edges of each ROWS (a team of one workgroup has no exchange at all),
  * the four forms of team_allreduce -- region A in one step, region A in two levels (teams of more than 64 workgroups), one
    sub-team through the XCD's L2 (region F; pk_collect takes a second trip past 64 slots), several sub-teams (regions F, X, B) --
    chosen by LORADS_PERSIST_L2 / LORADS_PERSIST_MAP and the team's size,
  * several unequal cones with idle blocks under each knob,
  * the reset of the granule tags before they wrap (lorads_hip_persist_set_tag puts a context next to it),
  * the hand-over between the one-launch and the launch-by-launch form inside one context (persist_ready refuses maxit >= 3993),

and every case asserts from the host's plan (lorads_hip_persist_plan, lorads_hip_persist_stats) and from the launch's own report
(lorads_hip_persist_stamps, word 15) that it ran the variant it names.  A (rows, rank) pair without an instantiation is an
EXPECTED refusal and is listed as such.

Bounds.  The cap is BOUNDS["default"] = 1e-12 of test_fixed_count_sweeps.  Below it every case has a bound of its own that owes
nothing to the device: the same schedule runs on the model in float64 as well, `spread` is the largest rel-to-scale difference
between the two models over everything compared, and the case allows max(32 spread, 1e-14) (the convention of
tests/test_fixed_count_alm.py).  Model alone, n = 33 .. 4128: spread 0.7e-15 .. 6.3e-15, bounds 2e-14 .. 2e-13."""
import pytest

from lorads_amd import instances
from tests import common
from tests.test_fixed_count_sweeps import BOUNDS, FULL, SHORT, RANKS, run_case

pytestmark = pytest.mark.gpu

# group of cases: (worst device-against-model figure measured on the MI355X, its quantity and case, that case's bound by the rule
# above, the figure as a fraction of the bound).  No case came nearer to its bound than 0.04 of it.
MEASURED = {
    "every instantiation": (1.10e-15, "factors, k_admm_diag<2, 1> r 30", 3.6e-14, 0.03),
    "pairs without instantiation (launch by launch)": (1.27e-15, "factors, <5, 2>", 3.5e-14, 0.04),
    "row edges": (2.77e-15, "factors, rows 4 n 129", 7.3e-14, 0.04),
    "row edges, n 2 (launch by launch)": (1.59e-14, "err1 to itself (model spread 4.1e-14: the 1e-12 cap)", 1.0e-12, 0.02),
    "exchange forms, n 2080": (3.81e-15, "factors, r 4 no knob (one sub-team of 65)", 1.0e-13, 0.04),
    "exchange forms, n 4128": (1.27e-14, "factors, LORADS_PERSIST_L2=0 (model spread 5.7e-14: the 1e-12 cap)", 1.0e-12, 0.01),
    "several cones": (4.87e-15, "factors, blkmix5 LORADS_PERSIST_ROWS=4", 1.1e-13, 0.04),
    "tag wrap": (1.02e-15, "factors, blk4x60 (both cases)", 3.7e-14, 0.03),
    "form hand-over": (1.52e-15, "scalars, maxcut100", 6.2e-14, 0.02),
}

LAUNCH_TAGS = 16384                           # PK_TAGS_PER_LAUNCH
TAG_RESET = 0xffffffff - 4 * LAUNCH_TAGS      # a launch that finds the next tag above this clears the granules and starts at 0
STOPS_A, STOPS_B = (3, 5, 4, 2, 6, 7, 8), (6, 2, 7, 8, 4, 3, 5)
P, L = 3992, 3993                             # the largest maxit that runs as one launch, the smallest that is refused
HANDOVER = [("step", P, STOPS_A, "fixed"), ("sweep", L, STOPS_B, "fixed"), ("step", P, STOPS_A, "fixed"), ("step", L, STOPS_B, "fixed"),
            ("sweep", P, STOPS_A, "fixed"), ("step", P, STOPS_B, "fixed"), ("step", L, STOPS_A, "fixed"), ("step", P, STOPS_B, "fixed")]
BLKMIX5_N = [90, 120, 150, 260, 200]


def _maxcut(n, seed=None):
    """a Max-Cut cone of n rows with about 2 n edges (seeded), written once per test process.  Fewer edges where 2 n would make
    the objective dense by the reference's rule (more than 0.1 n (n + 1) / 2 stored entries: below n = 64), since a cone with a
    dense C is not of the one-launch kind; some rows of such a graph have no neighbour at all."""
    sparse = int(0.05 * n * (n + 1)) - n
    edges = max(1, min(2 * n, sparse, n * (n - 1) // 2))
    return common.generated_instance("mc%d" % n, make=lambda: instances.maxcut(n, edges, seed or 7000 + n))


def _steps(ranks):
    """column steps of 16 columns that the widest cone takes (an odd rank runs padded to the next even one)"""
    return max((r + r % 2 + 15) // 16 for r in ranks)


def _groups(ns, rows):
    return [-(-n // (32 * rows)) for n in ns]


def _expected_plan(ns, rows, plan, linear):
    """persist_build's deal of the teams to blocks, from the device's own occupancy and CU count: (xcd_map, grid, sub-teams of each
    cone as lists of sizes)"""
    G = _groups(ns, rows)
    cap_x = plan["occ"] * (plan["ncu"] // 8)
    order = sorted(range(len(G)), key=lambda k: -G[k])  # (stable: largest first, ties in file order)
    load, xcd_of, ok = [0] * 8, {}, not linear and plan["ncu"] % 8 == 0
    for k in order:
        x = min(range(8), key=lambda y: (load[y], y))
        xcd_of[k] = x
        load[x] += G[k]
        ok = ok and load[x] <= cap_x
    if ok:
        return True, 8 * max(load), [[g] for g in G]
    subs, b0 = [], 0
    for g in G:
        sizes = [sum(1 for b in range(b0, b0 + g) if b % 8 == x) for x in range(8)]
        subs.append([z for z in sizes if z])
        b0 += g
    return False, sum(G), subs


def _assert_plan(facts, ns, rows, column_steps, linear=False, allow_l2=True):
    """the case ran the variant it names: rows, column steps, grid, map, teams and sub-teams, every call as one launch, and what
    the launch itself decided about the L2 forms (cone 0's team reports)"""
    st, plan = facts["stats"], facts["plan"]
    print("plan", plan, "stats", st, "l2", facts.get("l2"), "one-launch calls", facts["persist_calls"])
    assert st["available"] == 1 and st["rows"] == rows and st["column_steps"] == column_steps, st
    assert plan["allow_l2"] == (1 if allow_l2 else 0) and plan["occ"] >= 1 and plan["ncu"] >= 8, plan
    xcd, grid, subs = _expected_plan(ns, rows, plan, linear)
    assert plan["xcd_map"] == (1 if xcd else 0) and st["workgroups"] == grid, (plan, st, xcd, grid)
    assert plan["team"] == max(_groups(ns, rows)) and plan["sub_teams"] == max(len(x) for x in subs) and \
        plan["sub_team"] == max(max(x) for x in subs), (plan, subs)
    if linear:
        assert plan["xcd_map"] == 0, plan
    assert all(x == 1 for x in facts["persist_calls"]), facts["persist_calls"]
    # cone 0's team: granules through the L2 (bit 0) once the launch has verified its placement, factor rows too (bit 1) where the
    # team is one sub-team; a team of one workgroup exchanges nothing
    g0 = _groups(ns, rows)[0]
    want = 0 if (not allow_l2 or g0 == 1) else (3 if len(subs[0]) == 1 else 1)
    assert facts["l2"] == want, (facts["l2"], want, plan)
    return xcd, subs


def _bound(worst):
    return min(max(32.0 * worst["spread"], 1e-14), BOUNDS["default"])


def _check(label, worst):
    b = _bound(worst)
    print(label, "worst", {k: "%.2e" % v for k, v in worst.items()}, "bound %.2e" % b, "used %.2f" % (
        max(worst["factors"], worst["vectors"], worst["scalars"]) / b))
    assert worst["factors"] <= b and worst["vectors"] <= b and worst["scalars"] <= b, (label, worst, b)


def _run(n, r, env, schedule=FULL, **kw):
    return run_case("mc%d" % n, env, params=dict(timesLogRank=0.1), schedule=schedule, ranks=r, path=_maxcut(n), stamps=True,
                    spread=True, **kw)


# ---- all fourteen instantiations: one cone of 200 rows (teams of 7 / 4 / 2 workgroups at 1 / 2 / 4 rows per lane group, the last
# one partly filled), r = 16 NS - 2 (the last column step half used); r = 16 NS and an odd rank (17, padded to 18) besides
INSTANCES = [(ns, 1, 16 * ns - 2) for ns in range(1, 9)] + [(ns, 2, 16 * ns - 2) for ns in range(1, 5)] + \
            [(ns, 4, 16 * ns - 2) for ns in range(1, 3)] + [(2, 1, 32), (6, 1, 96), (7, 1, 112), (2, 2, 17)]


@pytest.mark.parametrize("ns,rows,r", INSTANCES)
def test_every_instantiation(built, ns, rows, r):
    facts, worst = _run(200, r, {"LORADS_PERSIST_ROWS": str(rows)})
    assert facts["ranks"] == [r], facts["ranks"]
    assert _steps([r]) == ns
    _assert_plan(facts, [200], rows, ns)
    assert facts["plan"]["team"] == {1: 7, 2: 4, 4: 2}[rows]
    assert facts["persist"] == len(FULL), facts["persist"]
    _check("k_admm_diag<%d, %d> r %d" % (ns, rows, r), worst)


# ---- (rows, NS) pairs that have no instantiation: the context runs launch by launch, and says so
REFUSED = [(ns, 2) for ns in range(5, 9)] + [(ns, 4) for ns in range(3, 9)]


@pytest.mark.parametrize("ns,rows", REFUSED)
def test_pairs_without_instantiation_are_refused(built, ns, rows):
    r = 16 * ns - 2
    facts, worst = run_case("mc200", {"LORADS_PERSIST_ROWS": str(rows)}, params=dict(timesLogRank=0.1), schedule=RANKS, ranks=r,
                            path=_maxcut(200), spread=True)
    print("stats", facts["stats"], "plan", facts["plan"])
    assert facts["ranks"] == [r] and facts["kinds"] == ["k_op_diag"], facts
    assert facts["stats"]["available"] == 0 and facts["persist"] == 0 and facts["persist_calls"] == [0] * len(RANKS), facts
    assert facts["plan"]["tag"] == -1 and facts["plan"]["team"] == 0, facts["plan"]
    _check("refused <%d, %d>" % (ns, rows), worst)


# ---- rows per workgroup: 32 / 64 / 128 at 1 / 2 / 4 rows per lane group; one row more is a second workgroup.  n = 2 cannot be of
# the one-launch kind (two rows with any entry of C are a dense objective by the reference's rule, and persist_eligible keeps
# dense-C cones launch by launch): an expected refusal, pinned on the form that runs
@pytest.mark.parametrize("rows,n", [(1, 2), (1, 32), (1, 33), (2, 64), (2, 65), (4, 127), (4, 128), (4, 129)])
def test_row_edges(built, rows, n):
    facts, worst = _run(n, 2, {"LORADS_PERSIST_ROWS": str(rows)})
    if n == 2:
        print("stats", facts["stats"], "plan", facts["plan"], "image", facts["images"][0])
        assert facts["images"][0]["dense_c"] == 1 and facts["stats"]["available"] == 0 and facts["persist"] == 0, facts
    else:
        assert facts["images"][0]["dense_c"] == 0, facts["images"][0]
        _assert_plan(facts, [n], rows, 1)
        assert facts["plan"]["team"] == (2 if n > 32 * rows else 1), facts["plan"]
        assert facts["persist"] == len(FULL), facts["persist"]
    _check("rows %d n %d" % (rows, n), worst)


# ---- the exchange forms of team_allreduce
@pytest.mark.parametrize("n,r,env,schedule,form", [
    (2080, 4, {"LORADS_PERSIST_L2": "0"}, FULL, "A2"),      # 65 workgroups: region A in two levels, 64 + 1
    (4128, 4, {"LORADS_PERSIST_L2": "0"}, FULL, "A3"),      # 129 workgroups: 64 + 64 + 1
    (2080, 4, {"LORADS_PERSIST_MAP": "linear"}, FULL, "FXB"),  # eight sub-teams of 9 / 8: regions F, X, B
    (2080, 4, {}, FULL, "default"),                         # the XCD map where it fits: one sub-team of 65, two trips of pk_collect
    (2080, 34, {}, SHORT, "default"),                       # three column steps on a large team, once per map
    (2080, 34, {"LORADS_PERSIST_MAP": "linear"}, SHORT, "FXB"),
])
def test_exchange_forms(built, n, r, env, schedule, form):
    facts, worst = _run(n, r, env, schedule=schedule)
    linear, allow = env.get("LORADS_PERSIST_MAP") == "linear", env.get("LORADS_PERSIST_L2") != "0"
    xcd, subs = _assert_plan(facts, [n], 1, _steps([r]), linear=linear, allow_l2=allow)
    plan = facts["plan"]
    assert plan["team"] == (65 if n == 2080 else 129), plan
    if form in ("A2", "A3"):
        assert facts["l2"] == 0 and plan["allow_l2"] == 0, (facts["l2"], plan)
    elif form == "FXB":
        assert plan["sub_teams"] == 8 and plan["sub_team"] == 9 and sorted(subs[0]) == [8] * 7 + [9] and facts["l2"] == 1, (plan, subs)
    else:
        # 65 workgroups fit one XCD's share of the compute units at three or more workgroups per unit; the plan says which holds
        assert xcd == (65 <= plan["occ"] * (plan["ncu"] // 8) and plan["ncu"] % 8 == 0), plan
        if xcd:
            assert plan["sub_teams"] == 1 and plan["sub_team"] == 65 and facts["l2"] == 3, (plan, facts["l2"])
        else:
            assert plan["sub_teams"] == 8 and plan["sub_team"] == 9 and facts["l2"] == 1, (plan, facts["l2"])
    assert facts["persist"] == len(schedule), facts["persist"]
    _check("n %d r %d %s" % (n, r, env), worst)


# ---- several cones of unequal n and rank, idle blocks on the XCD map
@pytest.mark.parametrize("env,rows", [({"LORADS_PERSIST_MAP": "linear"}, 1), ({"LORADS_PERSIST_L2": "0"}, 1),
                                      ({"LORADS_PERSIST_ROWS": "2"}, 2), ({"LORADS_PERSIST_ROWS": "4"}, 4)])
def test_several_cones(built, env, rows):
    facts, worst = run_case("blkmix5", env, stamps=True, spread=True)
    assert len(set(facts["ranks"])) > 1, facts["ranks"]
    linear, allow = env.get("LORADS_PERSIST_MAP") == "linear", env.get("LORADS_PERSIST_L2") != "0"
    xcd, subs = _assert_plan(facts, BLKMIX5_N, rows, _steps(facts["ranks"]), linear=linear, allow_l2=allow)
    if xcd:  # five teams on eight XCDs: idle blocks
        assert facts["stats"]["workgroups"] > sum(_groups(BLKMIX5_N, rows)), facts["stats"]
    assert facts["persist"] == len(FULL), facts["persist"]
    _check("blkmix5 %s" % env, worst)


# ---- the tags' reset: (a) three launches before it, so that it falls into the schedule with a dual update pending; (b) the whole
# schedule just below it (the largest tags a launch ever uses).  (The L-BFGS team's own tags, 16 per launch, are not covered.)
@pytest.mark.parametrize("name", ["maxcut100", "blk4x60"])
@pytest.mark.parametrize("case", ["reset", "below"])
def test_tag_wrap(built, name, case):
    tag = TAG_RESET + 1 - 3 * LAUNCH_TAGS if case == "reset" else TAG_RESET - (len(FULL) - 1) * LAUNCH_TAGS
    facts, worst = run_case(name, {}, tag=tag, stamps=True, spread=True)
    print("plan", facts["plan"], "one-launch calls", facts["persist_calls"])
    assert facts["persist_calls"] == [1] * len(FULL), facts["persist_calls"]
    # the next tag: two launches after the reset / the last launch started exactly at the threshold
    want = (len(FULL) - 3) * LAUNCH_TAGS if case == "reset" else TAG_RESET + LAUNCH_TAGS
    assert facts["plan"]["tag"] == want and want < 2 ** 32, (facts["plan"], want)
    _check("%s tags %s" % (name, case), worst)


def test_set_tag_needs_a_plan(built, monkeypatch):
    monkeypatch.setenv("LORADS_PERSIST", "0")
    s = common.hip_session(common.instance_path("maxcut100"))
    try:
        assert s.hip_persist_stats()["available"] == 0
        with pytest.raises(Exception):
            s.hip_persist_set_tag(5)
    finally:
        s.close()


# ---- both directions of the hand-over between the forms inside one context: what the one-launch form carries ((C V) of
# LORADS_PERSIST_CARRY), what the launch-by-launch form keeps (t_uv_valid), and the pending dual update across the switch
@pytest.mark.parametrize("name", ["maxcut100", "blk4x60"])
def test_form_hand_over(built, name):
    facts, worst = run_case(name, {}, schedule=HANDOVER, stamps=True, spread=True)
    print("one-launch calls", facts["persist_calls"], "counts", facts["counts"], "stops", facts["stops"])
    assert facts["persist_calls"] == [1 if maxit == P else 0 for _, maxit, _, _ in HANDOVER], facts["persist_calls"]
    assert max(facts["counts"]) < 40 * 2 * len(facts["ranks"]), facts["counts"]  # (every solve stopped by its tolerance)
    _check("%s hand-over" % name, worst)
