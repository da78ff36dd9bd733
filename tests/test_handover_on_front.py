"""A step's result hand-over carried on the launch of the next step's U front (LORADS_HANDOVER_ON_FRONT): workgroup 0 of
k_front_cw's hand-over form runs the body of k_publish_final, workgroup b > 0 is row workgroup b - 1.  The switch changes which launch
the hand-over's workgroup belongs to, never what anybody computes, so everything must agree bit for bit with
LORADS_HANDOVER_ON_FRONT=0 in a second context: every step's (CG count, pObj, dObj, err1), the final U, V, lambda and the
speculation statistics.

Sizes: rs24 (24 rows: one row tile, the grid is the hand-over workgroup plus one), rand120 with LORADS_OP_CW=1 (a partly filled last
row tile; rank 9, which the device pads to 10 -- and rank 9 as it is, where nothing is enqueued ahead and every hand-over goes
alone), hub16 (CSR tails in both visits), coupled3x70 (three cones: never speculates)."""
import functools

import numpy as np
import pytest

from lorads_amd import host, instances
from tests import common
from tests import test_spec_front as tsf

ON, OFF = {}, {"LORADS_HANDOVER_ON_FRONT": "0"}
NOGRAPH = {"LORADS_GRAPH": "0"}   # every step launch by launch (a replayed chain has its own front and its own hand-over)


def _path(name):
    if name == "rs24":
        # (29 entries of C at most: above 30 it would be stored dense and leave the one-kernel front)
        return common.generated_instance(name, lambda: instances.randsparse(24, 12, 2201, c_edges=5, n_diag=2, n_off=3, r0=2))
    return tsf._case(name)[0]


def _loop_fresh(name, env, steps, const=False, deviate=None, at=5, hook=False, stop_at=None, split=False):
    """phase 1, then `steps` times admm_step + update_dual_var at the tolerance cycle of test_spec_front (const: 1e-8 throughout);
    split: every third step goes through admm_update_var and the separate evaluation entries; `deviate`: one of test_spec_front's
    deviations behind step `at`.  The two statistics are read after every step (both entries leave a front in flight alone), the
    launch count -- which does not -- before the first step and after the last."""
    env = dict(env)
    env.setdefault("LORADS_OP_CW", "1")
    s, calls = tsf._open(_path(name), env, hook=hook, phase1Tol=1e-2)
    try:
        s.alm()
        s.alm_to_admm()
        be = s.be
        be.init_constr(host.PAIR_UV)
        res0 = s.results()
        ctl = dict(rho=min(res0["admm_rho"] if res0["admm_rho"] > 0 else res0["alm_rho"], 5000.0), skip_dual=False, split=False)
        e = be.update_dimacs(host.PAIR_UV)
        tol_of = tsf.CONST if const else tsf.CYCLE
        log, per_step = [], []
        n0 = s.hip_launch_count()
        for it in range(steps):
            tol = tol_of(it, e)
            h0, m0 = s.hip_handover_stats(), s.hip_spec_front_stats()
            if ctl["split"] or (split and it % 3 == 2):
                ctl["split"] = False
                c = be.admm_update_var(ctl["rho"], tol, 800)
                p, d, e = be.cal_obj(host.PAIR_UV), be.cal_dual_obj(), be.update_dimacs(host.PAIR_UV)
            else:
                c, p, d, e = be.admm_step(ctl["rho"], tol, 800)
            h1, m1 = s.hip_handover_stats(), s.hip_spec_front_stats()
            per_step.append(dict(on_front=h1["on_front"] - h0["on_front"], alone=h1["alone"] - h0["alone"],
                                 enqueued=m1["enqueued"] - m0["enqueued"], adopted=m1["adopted"] - m0["adopted"],
                                 blocked=m1["blocked"] - m0["blocked"]))
            log.append((c, p, d, e))
            if stop_at is not None and it == stop_at:   # (close() with a front in flight)
                return dict(log=log, spec=m1, hand=h1, per_step=per_step, calls=calls)
            if deviate and it == at:
                deviate(s, ctl["rho"], "after_step", ctl)
            if ctl["skip_dual"]:
                ctl["skip_dual"] = False
            else:
                be.update_dual_var(ctl.get("dual_rho") or ctl["rho"])
                ctl["dual_rho"] = None
            if deviate and it == at:
                deviate(s, ctl["rho"], "after_dual", ctl)
            if ctl.get("window") and it == at + 3:   # (a timing window opened by the deviation: closed three steps later)
                ctl["window"] = False
                s.hip_profile(0, 1)
        spec, hand = s.hip_spec_front_stats(), s.hip_handover_stats()
        prof = s.hip_profile_read()
        launches = s.hip_launch_count() - n0
        return dict(log=log, U=[be.get_mat(host.MAT_U, k) for k in range(s.nblk)], V=[be.get_mat(host.MAT_V, k) for k in range(s.nblk)],
                    lam=be.get_vec(host.VEC_LAMBDA), misses=prof["speculation_misses"], solves=prof["cg_solves"], cg=prof["cg_iters"],
                    spec=spec, hand=hand, per_step=per_step, launches=launches, calls=calls, image=s.hip_block_image(0))
    finally:
        s.close()


@functools.lru_cache(maxsize=None)
def _loop(name, env=(), steps=40, const=False, what=None, hook=False, split=False):
    """_loop_fresh, once per test process and left unchanged by whoever reads it"""
    return _loop_fresh(name, dict(env), steps, const=const, deviate=tsf.DEVIATIONS[what] if what else None, hook=hook, split=split)


def _pair(name, env=(), **kw):
    """(default, LORADS_HANDOVER_ON_FRONT=0) of the same loop, compared bit for bit"""
    on = _loop(name, tuple(sorted(dict(env, **ON).items())), **kw)
    off = _loop(name, tuple(sorted(dict(env, **OFF).items())), **kw)
    tsf._same(on, off)
    assert on["spec"] == off["spec"], (on["spec"], off["spec"])
    assert off["hand"]["on_front"] == 0, off["hand"]
    for a, b in zip(on["per_step"], off["per_step"]):   # every hand-over arrives, one way or the other
        assert a["on_front"] + a["alone"] == b["alone"], (a, b)
    return on, off


# ---- 1. the plain loop, 40 steps, changing tolerance
PLAIN = {
    "rs24": {},
    "rand120": {},
    "hub16": {},
    "rand120_deal5": {"LORADS_ROW_DEAL": "5"},       # the row index is not 32 * blockIdx
    "rand120_rank9": {"LORADS_PAD_ODD_RANK": "0"},   # the odd rank as it is: no front is enqueued ahead, every hand-over goes alone
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(PLAIN))
def test_plain_loop_is_bitwise_the_loop_with_two_launches(built, case):
    name = case.split("_")[0]
    on, off = _pair(name, tuple(PLAIN[case].items()))
    print(case, "hand-overs", on["hand"], "fronts", on["spec"], "misses", on["misses"], "front_cw", on["image"]["front_cw"])
    # by default every front that is enqueued ahead carries the hand-over it used to follow
    assert on["hand"]["on_front"] == on["spec"]["enqueued"], (on["hand"], on["spec"])
    assert on["image"]["front_cw"] == 1, on["image"]
    if case != "rand120_rank9":
        assert on["hand"]["on_front"] > 0, on["hand"]
    if name == "rs24":
        assert on["image"]["n"] <= 32   # one row tile


# ---- 2. the statistics of the default
@pytest.mark.gpu
def test_every_step_but_the_first_has_its_hand_over_carried(built):
    """launch by launch at a fixed tolerance (a step that resumes a solve hands over once more, alone, in either context)"""
    steps = 12
    on, off = _pair("rand120", tuple(NOGRAPH.items()), steps=steps, const=True)
    print("per step", [(p["on_front"], p["alone"]) for p in on["per_step"]], "launches", on["launches"], off["launches"])
    for it, p in enumerate(on["per_step"]):
        if it >= 1:
            assert p["on_front"] == 1, (it, on["per_step"])
    assert all(p["on_front"] == 0 and p["alone"] >= 1 for p in off["per_step"]), off["per_step"]
    # one launch fewer for every carried hand-over, and nothing else moved
    assert off["launches"] - on["launches"] == on["hand"]["on_front"] >= steps - 1, (off["launches"], on["launches"], on["hand"])


# ---- 3. where the hand-over must go alone
@pytest.mark.gpu
def test_alone_inside_a_profiling_window(built):
    on, off = _pair("rand120", tuple(NOGRAPH.items()), steps=12, const=True, what="profile_window")
    print([(p["on_front"], p["alone"]) for p in on["per_step"]])
    for it in (6, 7, 8):   # (opened behind step 5, closed behind step 8)
        assert (on["per_step"][it]["on_front"], on["per_step"][it]["alone"]) == (0, 1), (it, on["per_step"])
    assert on["per_step"][4]["on_front"] == 1 and on["per_step"][10]["on_front"] == 1, on["per_step"]


@pytest.mark.gpu
def test_alone_with_an_allreduce_hook(built):
    on, off = _pair("rand120", tuple(NOGRAPH.items()), steps=8, const=True, hook=True)
    assert on["calls"], "the hook was never called: not the sharded path"
    assert on["hand"]["on_front"] == 0 and on["hand"]["alone"] == off["hand"]["alone"], (on["hand"], off["hand"])


@pytest.mark.gpu
def test_alone_on_three_cones(built):
    on, off = _pair("coupled3x70")
    assert on["spec"]["enqueued"] == 0 and on["hand"]["on_front"] == 0, (on["spec"], on["hand"])


@pytest.mark.gpu
def test_a_second_dual_update_discards_the_front_and_keeps_its_hand_over(built):
    """the front behind step 5 has carried step 5's hand-over when the second update_dual_var discards it: the results were read
    long ago, step 6 launches its own front (and adopts none), and nothing changes"""
    on, off = _pair("rand120", tuple(NOGRAPH.items()), steps=12, const=True, what="dual_twice")
    print([(p["on_front"], p["alone"], p["adopted"]) for p in on["per_step"]])
    assert on["per_step"][5]["on_front"] == 1 and on["per_step"][6]["adopted"] == 0, on["per_step"]
    assert on["spec"]["discarded"] >= 1, on["spec"]


@pytest.mark.gpu
def test_a_blocked_front_still_hands_over(built):
    """rand120's tolerance cycle makes solves miss their speculation inside a step: the front behind such a step finds its gate shut
    and writes nothing, its hand-over workgroup publishes all the same (the host would wait for ever otherwise), and the resumed
    pass ends in a hand-over of its own"""
    on, off = _pair("rand120", tuple(NOGRAPH.items()))
    print([(p["on_front"], p["alone"], p["blocked"]) for p in on["per_step"]], on["misses"])
    assert on["misses"] > 0 and on["spec"]["blocked"] > 0, (on["misses"], on["spec"])
    for it, p in enumerate(on["per_step"]):
        if p["blocked"]:
            assert p["on_front"] == 1 and p["alone"] >= 1, (it, p)
            if it + 1 < len(on["per_step"]):
                assert on["per_step"][it + 1]["adopted"] == 0, (it, on["per_step"][it + 1])


# ---- 4. carried and lone hand-overs in turn
@pytest.mark.gpu
def test_carried_and_lone_hand_overs_alternate(built):
    """every third step through admm_update_var, cal_obj, cal_dual_obj, update_dimacs: their hand-overs go alone, those of the
    admm_steps between them ride, and host and device count the sequence numbers alike -- a wait that met a flag already consumed
    would return the previous step's numbers, one that missed its flag would never return"""
    on, off = _pair("rand120", tuple(NOGRAPH.items()), steps=15, const=True, split=True)
    print([(p["on_front"], p["alone"]) for p in on["per_step"]])
    for it, p in enumerate(on["per_step"]):
        if it % 3 == 2:
            assert p["on_front"] == 0 and p["alone"] >= 1, (it, p)
        elif it >= 1:
            assert p["on_front"] == 1, (it, p)


# ---- 5. close() with a carrying front in flight
@pytest.mark.gpu
def test_close_with_a_carrying_front_in_flight(built):
    on = _loop_fresh("rand120", dict(NOGRAPH, **ON), 6, const=True, stop_at=5)
    off = _loop_fresh("rand120", dict(NOGRAPH, **OFF), 6, const=True, stop_at=5)
    assert on["log"] == off["log"]
    assert tsf._in_flight(on["spec"]) == 1 and on["per_step"][5]["on_front"] == 1, (on["spec"], on["per_step"])
