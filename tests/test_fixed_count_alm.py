"""Consecutive phase-1 inner iterations of every device form against the extended-precision model (tests/alm_model.py).

Each case sets a seeded state (set_mat / set_vec, init_constr(PAIR_RR)) and runs the same inner iterations on the device and on the
model WITHOUT any resync, so an error in what is carried from one iteration to the next -- the ring's rotation, the older pair's alpha
and beta, y_new = y_new + Grad, the constraint sums' recurrence -- has nowhere to hide.  tau comes from the host's scalar line search
on the MODEL's coefficients and goes to both sides: no comparison depends on a branch of the cubic falling differently.  After every
iteration the case compares p1, p2, a, b, c, d, the direction D, q1, q2, R, Grad, ||Grad||^2, err1 and the device's constraint sums
against A(R R^T) formed by the model from the device's OWN R (a missed term of the recurrence then shows apart from rounding).
`path` is "fused" (alm_front / alm_step) or "slots" (the seven separate entries).  Every case also asserts that the form it names
really ran (one-launch statistics, launch counts per direction, hook calls and their sizes, operator kind, block image).

Bounds (alm_model.plan; nothing is taken from the device): e64(i) is the worst rel-to-scale difference, over all compared quantities
of iteration i, between the model in float64 and in longdouble on the same tau schedule.  A case compares the iterations before the
first with e64 > 3e-13 -- never fewer than 4 (history <= 2: no pair, one pair, two pairs, the ring's first overwrite), L + 3 in the
longer-history group, the whole schedule where it has 3 -- and no compared iteration sits near a branch point (|cos(D, Grad)| and
|cos(y, s)| >= 0.05 in the model).  The bound per case is max(32 max_i e64(i), 1e-14), never above 1e-11, relative to the quantity's
largest entry (p1 .. d: to the magnitudes of their terms; ||Grad||^2, err1: to themselves).  MEASURED holds the worst figure seen on
the MI355X per group, next to the bounds the rule gave there.

The longdouble model takes about 10 s for the three iterations of rand20000 and of maxcut20000 at r = 40 and 17 s for matcomp50000 at
r = 22, so all three full-size instances are in the list."""
import os

import numpy as np
import pytest

from lorads_amd import host, instances
from tests import common
from tests.alm_model import AlmModel, descent_tau, plan, record_errors

pytestmark = pytest.mark.gpu

# group of cases: (worst device-against-model figure measured on the MI355X, its quantity and case, the bounds the rule gave in the
# group, the worst figure as a fraction of its case's bound).  The device's constraint sums sit within 4.1e-16 of A(R R^T) of its own R
# in every case.  No case came nearer to its bound than 0.09 of it, and no case found a kernel error.
MEASURED = {
    "default one-launch direction": (3.6e-14, "D/R/Grad, blk4x60 history 1", (9.2e-14, 2.8e-12), 0.09),
    "its three variants": (1.9e-14, "q1/q2, maxcut100", (2.3e-13, 2.8e-12), 0.04),
    "every NP, rand120": (6.2e-15, "D/R/Grad, NP 2 history 1", (9.2e-14, 2.3e-13), 0.07),
    "every NP, rand4000": (2.2e-15, "D/R/Grad, NP 2 r 41", (3.6e-14, 7.3e-14), 0.04),
    "the form steps aside": (5.3e-14, "D/R/Grad, theta30", (1.6e-13, 1.8e-12), 0.03),
    "stage by stage": (3.1e-14, "D/R/Grad, maxcut100 fused", (2.3e-13, 2.8e-12), 0.04),
    "longer histories": (2.8e-14, "D/R/Grad, mix4 history 3 slots", (1.2e-13, 1.0e-12), 0.04),
    "Gram form on one GPU": (1.7e-14, "D/R/Grad, sdplp40", (2.3e-13, 5.0e-13), 0.03),
    "with a hook (Gram, per dot, separable)": (2.7e-14, "D/R/Grad, sdplp40 per dot", (2.3e-13, 5.0e-13), 0.05),
    "LP block, dense storage, Gram-operator cones": (1.1e-13, "q1/q2, theta50", (1.8e-13, 1.8e-12), 0.06),
    "rank dispatch": (6.8e-14, "D/R/Grad, maxcut800 r 41 unpadded", (3.7e-14, 3.2e-12), 0.04),
    "full size": (1.7e-15, "coefficients, maxcut20000", (2.0e-14, 4.3e-14), 0.05),
    "the fallback": (9.1e-15, "D/R/Grad, team form history 1", (1.0e-13, 1.2e-13), 0.09),
}

SMALL = dict(iters=10, rho=0.7, lam_scale=0.1, seed=5)
SHORT = dict(iters=3, rho=0.7, lam_scale=0.1, seed=5)
# the fallback: maxcut100 at rank 10, lam = 3 N(0, 1), rho = 0.02, iteration 0 steps to half the larger root of 4 a tau^2 + 3 b tau + 2 c
# (y.s = tau^2 (4 a tau^2 + 3 b tau + 2 c) < 0 there): cos(y, s) = -0.67, cos(D, Grad) = +0.98 at iteration 1 in the model
FALLBACK = dict(iters=6, rho=0.02, lam_scale=3.0, seed=5, descent_first=True)

_GEN = {"rand121": lambda: instances.randsparse(121, 40, 2001, c_edges=150, n_diag=2, n_off=3, r0=3)}  # (an odd cone dimension)


def _path(name):
    if name in _GEN:
        return common.generated_instance(name, make=_GEN[name])
    return common.instance_path(name) if os.path.exists(common.instance_path(name)) else common.generated_instance(name)


_plans = {}


def _plan(key, path, R, lam, sched, hist, min_iters):
    """the model's side of a case, shared by the cases that run the same state and schedule in other device forms (in memory only)"""
    if key not in _plans:
        if len(_plans) >= 2:
            _plans.pop(next(iter(_plans)))

        def tau_of(i, coef):
            if i == 0 and sched.get("descent_first"):
                tau = descent_tau(coef)
                assert tau is not None, "the quadratic of y.s has no positive root here"
                return tau
            return common.linesearch_tau(coef)[0]
        _plans[key] = plan(path, R, lam, sched["rho"], sched["iters"], hist, tau_of, min_iters=min_iters)
    return _plans[key]


def _mats(be, which, nb):
    return [be.get_mat(which, k) for k in range(nb)]


def run_case(name, env=None, params=None, schedule=SMALL, hist=2, ranks=None, separable=None, hook=False, path="fused", file=None):
    """runs the schedule on the model and on the device; returns (facts of the session, worst errors by group, bound, records).
    file: the instance's file where `name` is no named one."""
    env, params = env or {}, params or {}
    file = file or _path(name)
    rho = schedule["rho"]
    # the case's switches: most are read when the context is created, LORADS_LBFGS_TEAM_NP when the first fused step builds the team,
    # so they stay set for the whole case and are restored after it
    with common.environment(env):
        s = common.hip_session(file, separable=separable, lbfgs_len=hist, **params)
        try:
            calls = []
            if hook:
                s.set_allreduce(lambda ptr, count, on_device: calls.append(count))
            if ranks is not None:
                s.be.resize_rank([ranks] * s.nblk if isinstance(ranks, int) else ranks)
            be, nb = s.be, s.nblk
            shapes = [s.block_shape(k) for k in range(nb)]
            R, lam = common.random_r_state(s, schedule["seed"], schedule["lam_scale"])
            iters = schedule["iters"]
            min_iters = iters if iters < 4 else (hist + 3 if hist > 2 else 4)
            recs, e64, bound, model = _plan((name, tuple(shapes), hist, tuple(sorted(schedule.items()))), file, R, lam, schedule, hist,
                                            min_iters)
            assert model.m == s.m and model.nb == nb
            common.load_r_state(be, R, lam)
            worst = dict(coefficients=0.0, factors=0.0, vectors=0.0, scalars=0.0, own_csum=0.0)
            first_miss = None
            dir_launches, dir_calls, step_launches, fallbacks = [], [], [], []
            team0 = s.hip_lbfgs_team_stats()["launches"]
            lag0 = be.alm_cal_grad(rho)
            grad_prev = _mats(be, host.MAT_GRAD, nb)
            front = be.alm_front(rho, 0) if path == "fused" else None
            for i, want in enumerate(recs):
                tau = want["tau"]
                if path == "fused":
                    p1, p2, coef = front
                    got = dict(D=_mats(be, host.MAT_U, nb), q1=be.get_vec(host.VEC_Q1), q2=be.get_vec(host.VEC_Q2))
                    n0 = s.hip_launch_count()
                    lag, err1, np1, np2, ncoef = be.alm_step(rho, tau, i + 1)
                    step_launches.append(s.hip_launch_count() - n0)
                    front = (np1, np2, ncoef)
                else:
                    n0, c0 = s.hip_launch_count(), len(calls)
                    be.lbfgs_direction(i)
                    dir_launches.append(s.hip_launch_count() - n0)
                    dir_calls.append(calls[c0:])
                    got = dict(D=_mats(be, host.MAT_U, nb))
                    p1, p2 = be.alm_q12p12()
                    coef = be.alm_linesearch_coeffs(rho, p1, p2)
                    got.update(q1=be.get_vec(host.VEC_Q1), q2=be.get_vec(host.VEC_Q2))
                    be.set_y_as_neg_grad()
                    be.alm_update_var(tau)
                    lag = be.alm_cal_grad(rho)
                    be.set_lbfgs_his_two(tau)
                    err1 = be.update_dimacs(host.PAIR_RR)
                got.update(p1=p1, p2=p2, a=coef[0], b=coef[1], c=coef[2], d=coef[3], lagNormSq=lag, err1=err1,
                           R=_mats(be, host.MAT_R, nb), Grad=_mats(be, host.MAT_GRAD, nb), csum=be.get_vec(host.VEC_CONSTR_SUM))
                if i == 0:
                    got["lag0"] = lag0
                err = record_errors(got, want)
                Rd = [r.astype(model.dtype) for r in got["R"]]  # (the device's own R, its row dots summed in extended precision)
                err["own_csum"] = common.rel_to_scale(got["csum"], model.auv(Rd, Rd).astype(np.float64))
                for key, v in err.items():
                    worst[key] = max(worst[key], v)
                    if v > bound and first_miss is None:
                        first_miss = (i, key, v)
                if want["fallback"]:  # D = -Grad of the device's own gradient, to the bit (and the model's within the bound, above)
                    fallbacks.append(i)
                    assert all(np.array_equal(d, -g) for d, g in zip(got["D"], grad_prev)), (name, env, i, "D is not -Grad")
                grad_prev = got["Grad"]
            st = s.hip_lbfgs_team_stats()
            facts = dict(team=dict(st, launches=st["launches"] - team0), kinds=[s.hip_operator_kind(k) for k in range(nb)],
                         images=[s.hip_block_image(k) for k in range(nb)], ranks=[sh[1] for sh in shapes], iters=len(recs),
                         dir_launches=dir_launches, dir_calls=dir_calls, step_launches=step_launches, calls=list(calls),
                         fallbacks=fallbacks, elements=sum(a * b for a, b in shapes), hist=hist, lp=[cn.is_lp for cn in model.cones], m=s.m,
                         dense=[s.hip_dense_plan(k) for k in range(nb)], layouts=[s.hip_cw_layout(k) for k in range(nb)])
            print(name, env, path, "history", hist, "ranks", facts["ranks"], "iterations", len(recs), "e64 %.1e" % max(e64[:len(recs)]),
                  "bound %.1e" % bound, "worst", {k: "%.1e" % v for k, v in worst.items()}, "team", facts["team"],
                  "launches/direction", dir_launches, "launches/step", step_launches,
                  "hook calls by size", {n: calls.count(n) for n in sorted(set(calls))}, "fallback at", fallbacks,
                  "cos(D,Grad)", ["%.2f" % r["cos_dg"] for r in recs])
            assert first_miss is None, (name, env, path, hist, "first miss (iteration, group, error)", first_miss, "bound", bound, worst,
                                        "e64", e64)
            return facts, worst, bound, recs
        finally:
            s.close()


def _nn(i, L):
    return 0 if i == 0 else (i if i <= L - 1 else L)


def _took_team(facts):
    assert facts["team"]["available"] == 1 and facts["team"]["launches"] == facts["iters"], facts["team"]


def _took_stages(facts):
    """the stage-by-stage recursion ran every direction of the slot path: ST_FIRST, nn alpha stages, nn w stages, k_use_grad_p"""
    assert facts["team"]["launches"] == 0, facts["team"]
    assert facts["dir_launches"] == [2 * _nn(i, facts["hist"]) + 2 for i in range(facts["iters"])], facts["dir_launches"]


# ---- the default: the one-launch direction of the fused step (one cone, or cones merged into one view, that sees every constraint)
@pytest.mark.parametrize("hist", [2, 1])
@pytest.mark.parametrize("name", ["rand120", "maxcut100", "matcomp60", "mix4", "blk4x60"])
def test_default_one_launch_direction(built, name, hist):
    facts, _, _, _ = run_case(name, hist=hist)
    _took_team(facts)


@pytest.mark.parametrize("switch", ["LORADS_ALM_FUSED_TAIL", "LORADS_ALM_FOLD_CV", "LORADS_ALM_SVAL_DIRECT"])
@pytest.mark.parametrize("name", ["rand120", "maxcut100", "matcomp60"])
def test_variants_of_the_shared_passes(built, name, switch):
    """each switch against the default on the same state: the bounds, and the launches per fused step that show the switch acted.
    LORADS_ALM_FUSED_TAIL=0 takes the launch-by-launch tail everywhere (more launches).  LORADS_ALM_FOLD_CV=0 gives the constraints'
    bookkeeping a launch of its own (k_cv_res_rd: one more per step) where the fold applies, i.e. where every constraint is one
    diagonal or one single entry (maxcut100, matcomp60); on rand120 the fold never applies and the counts must be EQUAL.
    LORADS_ALM_SVAL_DIRECT=0 puts k_sval behind k_alm_update (one more per step) where every pattern entry belongs to one constraint
    (Block::sv_direct: maxcut100, matcomp60); rand120's constraints share entries (176 positions for 200 entries), so k_sval runs
    either way and the counts must be EQUAL.  Which of the two holds is worked out here from the block image and the file's entries."""
    base, _, _, _ = run_case(name)
    facts, _, _, _ = run_case(name, {switch: "0"})
    _took_team(facts)
    img = facts["images"][0]
    cone = AlmModel.from_file(_path(name)).cones[0]
    single_entry = bool((img["diag_only"] or img["entry_only"]) and img["na"] == img["nrow"])
    unshared = len(np.unique(cone.a_row * cone.n + cone.a_col)) == len(cone.a_row)
    assert (single_entry, unshared) == ((False, False) if name == "rand120" else (True, True)), (name, single_entry, unshared, img)
    got, was = facts["step_launches"], base["step_launches"]
    if switch == "LORADS_ALM_FUSED_TAIL":
        assert all(g > w for g, w in zip(got, was)), (got, was)
    else:
        acts = single_entry if switch == "LORADS_ALM_FOLD_CV" else unshared
        assert got == [w + (1 if acts else 0) for w in was], (name, switch, acts, got, was)


# ---- every instantiation of the team kernel; the vector's end falls inside a thread's slices (the buffer's range check keeps the tail)
NPS = [1, 2, 3, 4, 6, 8, 12]


@pytest.mark.parametrize("hist", [2, 1])
@pytest.mark.parametrize("np_", NPS)
def test_every_np_of_the_team_kernel_small(built, np_, hist):
    facts, _, _, _ = run_case("rand120", {"LORADS_LBFGS_TEAM_NP": str(np_)}, hist=hist)
    _took_team(facts)
    assert facts["team"]["pairs"] == np_ and 1 <= facts["team"]["workgroups"] <= 3, facts["team"]
    assert facts["team"]["workgroups"] == -(-(facts["elements"] // 2) // (256 * np_)), (facts["team"], facts["elements"])


@pytest.mark.parametrize("hist", [2, 1])
@pytest.mark.parametrize("r", [40, 41])
@pytest.mark.parametrize("np_", NPS)
def test_every_np_of_the_team_kernel_rand4000(built, np_, r, hist):
    facts, _, _, _ = run_case("rand4000", {"LORADS_LBFGS_TEAM_NP": str(np_)}, params=dict(timesLogRank=0.1), schedule=SHORT, hist=hist,
                              ranks=r)
    _took_team(facts)
    assert facts["team"]["pairs"] == np_ and facts["ranks"] == [r], facts


# ---- the form steps aside
def test_steps_aside_odd_element_count(built):
    """n = 121 at rank 3 unpadded: 363 doubles are no whole number of pairs (lteam_build: all_elem & 1)"""
    env = {"LORADS_PAD_ODD_RANK": "0"}
    facts, _, _, _ = run_case("rand121", env, params=dict(timesLogRank=0.1), ranks=3)
    assert facts["elements"] == 363 and facts["team"]["available"] == 0 and facts["team"]["launches"] == 0, facts
    _took_stages(run_case("rand121", env, params=dict(timesLogRank=0.1), ranks=3, path="slots")[0])


def test_steps_aside_history_three(built):
    """history 3 is above what the one launch holds (lteam_ready: L > 2)"""
    facts, _, _, _ = run_case("rand120", hist=3)
    assert facts["team"]["available"] == 0 and facts["team"]["launches"] == 0, facts["team"]
    _took_stages(run_case("rand120", hist=3, path="slots")[0])


def test_steps_aside_dense_objective(built):
    """theta30: the objective matrix is stored dense, and the fused step's one-cone branch -- the only caller of lteam_ready -- is not
    taken for a cone with dense storage (lorads_hip_alm_step: !dense_c && !dense_a); the plan is never built"""
    facts, _, _, _ = run_case("theta30")
    assert facts["images"][0]["dense_c"] == 1 and facts["team"]["available"] == 0 and facts["team"]["launches"] == 0, facts
    _took_stages(run_case("theta30", path="slots")[0])


def test_steps_aside_coupled_cones(built):
    """coupled3x70: constraints that couple the cones leave no merged view, so the context is not one cone that sees every constraint
    (lorads_hip_alm_step: solo(c) is null) and lteam_ready is never asked"""
    facts, _, _, _ = run_case("coupled3x70")
    assert len(facts["kinds"]) == 3 and facts["team"]["available"] == 0 and facts["team"]["launches"] == 0, facts
    _took_stages(run_case("coupled3x70", path="slots")[0])


# ---- stage by stage
@pytest.mark.parametrize("path", ["fused", "slots"])
@pytest.mark.parametrize("name", ["rand120", "maxcut100", "matcomp60", "mix4", "blk4x60", "coupled3x70"])
def test_stage_by_stage_form(built, name, path):
    facts, _, _, _ = run_case(name, {"LORADS_LBFGS_TEAM": "0"}, path=path)
    assert facts["team"]["launches"] == 0, facts["team"]
    if path == "slots":
        _took_stages(facts)


@pytest.mark.parametrize("path", ["fused", "slots"])
@pytest.mark.parametrize("hist", [3, 5])
@pytest.mark.parametrize("name", ["rand120", "mix4"])
def test_longer_histories(built, name, hist, path):
    """at least L + 3 iterations: nn takes every value and the ring wraps"""
    facts, _, _, _ = run_case(name, hist=hist, path=path)
    assert facts["iters"] >= hist + 3 and facts["team"]["launches"] == 0, facts
    if path == "slots":
        _took_stages(facts)


# ---- Gram forms
@pytest.mark.parametrize("name", ["rand120", "mix4", "sdplp40", "densea40"])
def test_gram_form_on_one_gpu(built, name):
    """LORADS_LBFGS_GRAM=2: k_gram, k_gram_final, k_lincomb per direction past iteration 0 (one copy at iteration 0)"""
    facts, _, _, _ = run_case(name, {"LORADS_LBFGS_GRAM": "2"}, path="slots")
    assert facts["team"]["launches"] == 0 and facts["dir_launches"] == [1] + [3] * (facts["iters"] - 1), facts["dir_launches"]
    # the fused path (the one launch off: it would take the direction where it applies): every step holds the NEXT direction, which
    # takes 3 launches where the stage form takes 2 nn + 2
    fused, _, _, _ = run_case(name, {"LORADS_LBFGS_GRAM": "2", "LORADS_LBFGS_TEAM": "0"})
    stage, _, _, _ = run_case(name, {"LORADS_LBFGS_TEAM": "0"})
    assert fused["team"]["launches"] == 0 and stage["team"]["launches"] == 0, (fused["team"], stage["team"])
    assert fused["step_launches"] == [w - (2 * _nn(i + 1, 2) + 2 - 3) for i, w in enumerate(stage["step_launches"])], \
        (fused["step_launches"], stage["step_launches"])


@pytest.mark.parametrize("gram", ["1", "0"])
@pytest.mark.parametrize("name", ["rand120", "mix4", "sdplp40", "densea40"])
def test_sharded_directions_with_a_hook(built, name, gram):
    """an all-reduce hook on one rank (the sum over one rank is the identity): LORADS_LBFGS_GRAM=1 takes ONE collective per
    direction, of the (2 nn + 1)(2 nn + 2) / 2 products; =0 one collective of one double per dot, 2 nn + 1 of them"""
    facts, _, _, _ = run_case(name, {"LORADS_LBFGS_GRAM": gram}, separable=False, hook=True, path="slots")
    assert facts["team"]["launches"] == 0, facts["team"]
    for i, got in enumerate(facts["dir_calls"]):
        nn = _nn(i, 2)
        nv = 2 * nn + 1
        want = ([nv * (nv + 1) // 2] if nn else []) if gram == "1" else [1] * nv
        assert got == want, (name, gram, i, got, want)
    # the fused path: the same collectives outside the directions, plus the front of the iteration after the last (one more
    # direction and one more q1 / q2 collective); the directions' own collectives by their sizes
    fused, _, _, _ = run_case(name, {"LORADS_LBFGS_GRAM": gram}, separable=False, hook=True)
    n = fused["iters"]
    other = len(facts["calls"]) - sum(len(c) for c in facts["dir_calls"])
    per_dir = [(1 if _nn(i, 2) else 0) if gram == "1" else 2 * _nn(i, 2) + 1 for i in range(n + 1)]
    assert fused["team"]["launches"] == 0 and len(fused["calls"]) == other + 1 + sum(per_dir), (len(fused["calls"]), other, per_dir)
    assert fused["m"] not in (6, 15) and 2 * fused["m"] + 2 not in (6, 15), fused["m"]
    assert (fused["calls"].count(6), fused["calls"].count(15)) == ((1, n - 1) if gram == "1" else (0, 0)), fused["calls"]


def test_separable_shard_with_a_hook(built):
    """blk4x60 as a separable shard: scalars only go through the hook"""
    for path in ("fused", "slots"):
        facts, _, _, _ = run_case("blk4x60", separable=True, hook=True, path=path)
        m = facts["images"][0]["nrow"]
        assert facts["team"]["launches"] == 0 and len(facts["calls"]) > 0 and max(facts["calls"]) < m, (facts["team"], facts["calls"])


# ---- LP block, dense storage, Gram-operator cones
@pytest.mark.parametrize("path", ["fused", "slots"])
@pytest.mark.parametrize("name", ["sdplp40", "coupledlp", "sdpslack30", "densea40", "densec40", "theta30", "theta50"])
def test_lp_block_dense_storage_and_gram_operator_cones(built, name, path):
    facts, _, _, _ = run_case(name, path=path)
    if name in ("sdplp40", "coupledlp", "sdpslack30"):
        assert facts["ranks"][-1] == 1 and facts["lp"][-1] and not any(facts["lp"][:-1]), (facts["ranks"], facts["lp"])
    if name == "densea40":
        assert facts["images"][0]["dense_a"] > 0 and "dense A_i" in facts["kinds"][0], facts
    if name in ("densec40", "theta30", "theta50"):
        assert facts["images"][0]["dense_c"] == 1, facts["images"][0]
    if name in ("theta30", "theta50"):
        assert facts["kinds"] == ["k_pairdots+k_sgram+k_spmm2"], facts["kinds"]


# ---- the rank dispatch of the phase-1 row kernels (k_spmm2, k_pairdots_rrd, k_cv_res_rd, the team kernel's NP); odd ranks unpadded too
RANK_LIST = [2, 8, 40, 41, 64, 66, 127, 128, 130, 200]


@pytest.mark.parametrize("name", ["rand4000", "maxcut800"])
@pytest.mark.parametrize("r", RANK_LIST)
def test_rank_dispatch(built, name, r):
    for env in [{}] + ([{"LORADS_PAD_ODD_RANK": "0"}] if r % 2 else []):
        facts, _, _, _ = run_case(name, env, params=dict(timesLogRank=0.1), schedule=SHORT, ranks=r)
        assert facts["ranks"] == [r], facts["ranks"]
        _took_team(facts)
        # the layout really differs: an odd rank runs as r + 1 columns unless LORADS_PAD_ODD_RANK=0, and the team's size shows which
        cols = r + (r % 2 if not env else 0)
        n = facts["images"][0]["n"]
        assert facts["team"]["workgroups"] == -(-(n * cols // 2) // (256 * facts["team"]["pairs"])), (facts["team"], n, cols)
        stage, _, _, _ = run_case(name, dict(env, LORADS_LBFGS_TEAM="0"), params=dict(timesLogRank=0.1), schedule=SHORT, ranks=r)
        assert stage["team"]["launches"] == 0


# ---- full size
@pytest.mark.timeout(1200)
@pytest.mark.parametrize("name,params,ranks", [("rand20000", dict(timesLogRank=0.1), 40), ("maxcut20000", dict(timesLogRank=0.1), 40),
                                               ("matcomp50000", dict(timesLogRank=2.0), None)])
def test_full_size(built, name, params, ranks):
    """BASELINE configs 3b and 3a at r = 40 and config 5 at its own rank (22): 3 iterations, the team form (more than one pair of
    doubles per thread and vector) and the stage form.  From these starts the host's own tau stores a pair with y.s < 0 on maxcut20000
    (the model takes the fallback at iteration 1, cos(D, Grad) = +1.00) and on matcomp50000 (iteration 2, +0.54), as it does on
    maxcut800 at ranks 2 and 8 in the rank dispatch: the branch is met by line-search steps too, and both forms match it there."""
    facts, _, _, _ = run_case(name, params=params, schedule=SHORT, ranks=ranks)
    _took_team(facts)
    assert facts["team"]["pairs"] > 1 and facts["ranks"] == [ranks or 22], facts
    stage, _, _, _ = run_case(name, {"LORADS_LBFGS_TEAM": "0"}, params=params, schedule=SHORT, ranks=ranks)
    assert stage["team"]["launches"] == 0


# ---- the fallback D = -Grad, taken by the model and by the device at iteration 1
@pytest.mark.parametrize("hist", [2, 1])
@pytest.mark.parametrize("form,env,path", [
    ("team", {}, "fused"),
    ("stage", {"LORADS_LBFGS_TEAM": "0"}, "fused"),
    ("stage", {"LORADS_LBFGS_TEAM": "0"}, "slots"),
    ("gram", {"LORADS_LBFGS_GRAM": "2"}, "slots"),
])
def test_the_fallback_is_taken(built, form, env, path, hist):
    facts, _, _, recs = run_case("maxcut100", env, params=dict(timesLogRank=0.1), schedule=FALLBACK, hist=hist, ranks=10, path=path)
    assert recs[0]["cos_ys"] <= -0.1 and recs[1]["fallback"] and recs[1]["cos_dg"] >= 0.1, (recs[0]["cos_ys"], recs[1]["cos_dg"])
    assert 1 in facts["fallbacks"] and facts["ranks"] == [10], facts
    if form == "team":
        _took_team(facts)
    elif form == "stage" and path == "slots":
        _took_stages(facts)
    elif form == "gram":
        assert facts["dir_launches"] == [1] + [3] * (facts["iters"] - 1), facts["dir_launches"]
    else:
        assert facts["team"]["launches"] == 0


def test_the_fallback_is_taken_with_a_hook(built):
    """the sharded Gram form (one collective per direction) and the per-dot form take the branch too"""
    for gram in ("1", "0"):
        facts, _, _, recs = run_case("maxcut100", {"LORADS_LBFGS_GRAM": gram}, params=dict(timesLogRank=0.1), schedule=FALLBACK, ranks=10,
                                     separable=False, hook=True, path="slots")
        assert recs[1]["fallback"] and 1 in facts["fallbacks"] and len(facts["calls"]) > 0, facts
