"""The cuts in the solve front's chain of dependent loads (k_front_cw, LORADS_FRONT_CHAIN): the neighbour
rows loaded without the mask of the slice beyond r, the row's own operands requested late.  Either leaves the arithmetic as it
is -- the same products added in the same order -- so any mask must agree with LORADS_FRONT_CHAIN=0 bit for bit.  (The held
batch of slots 4..7, the objective list's row-indexed head, the hand-over form's XCD shift and the CG0 form's early average row
were measured and dropped, profiles/r11_tried_and_dropped.txt: there is no head array and so no builder to check on the CPU; the
seam instance stays, its rows of 8, 9 and 17+ neighbours end an objective trip at every place one can end.)"""
import os

import numpy as np
import pytest

from lorads_amd import host, instances
from tests import common

FC_ALL = 3


def _untouched():
    return instances.randsparse_untouched_rows(130, 50, 2201, rows=[0, 7, 64, 129], c_edges=160, n_diag=2, n_off=3, r0=3)


SEAM_SEED = 10


def _seam():
    return instances.randsparse(96, 60, SEAM_SEED, c_edges=900, n_diag=2, n_off=4, r0=3)


MAKE = {"untouched130": _untouched, "seam96": _seam}


def _path(name):
    if name in MAKE:
        return common.generated_instance(name, MAKE[name])
    if name in ("rand120", "hub8", "hub16") and os.path.exists(common.instance_path(name)):
        return common.instance_path(name)
    return common.generated_instance(name)


def _objective_lists(prob):
    """row -> [(neighbour, c)]: the objective's adjacency as the front walks it (both orientations, duplicates summed,
    neighbours ascending, the diagonal once)"""
    n = prob["blocks"][0]
    rows = [dict() for _ in range(n)]
    for mat, _blk, i, j, v in prob["entries"]:
        if mat != 0:
            continue
        i, j = i - 1, j - 1
        rows[i][j] = rows[i].get(j, 0.0) - v   # (F0 = -C)
        if i != j:
            rows[j][i] = rows[j].get(i, 0.0) - v
    return [sorted(r.items()) for r in rows]


def _run(path, env, steps, rank=None, **kw):
    """phase 1 + `steps` ADMM iterations (every third one through the separate entry points) under `env`; tolerances that
    change from step to step give speculation misses and solves of one and of many iterations"""
    s = common.hip_session_with_env(path, env, dict(phase1Tol=1e-2, **kw))
    try:
        if rank is not None:
            s.be.resize_rank([rank] * s.nblk)
        kind = s.hip_operator_kind(0)
        mask = s.hip_front_chain()
        eff = s.hip_front_chain(effective=True)
        shape = s.block_shape(0)
        s.alm()
        s.alm_to_admm()
        s.be.init_constr(host.PAIR_UV)
        res0 = s.results()
        rho = min(res0["admm_rho"] if res0["admm_rho"] > 0 else res0["alm_rho"], 5000.0)
        e = s.be.update_dimacs(host.PAIR_UV)
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
        ho = s.hip_handover_stats()
        return dict(log=log, U=[s.be.get_mat(host.MAT_U, k) for k in range(s.nblk)],
                    V=[s.be.get_mat(host.MAT_V, k) for k in range(s.nblk)], lam=s.be.get_vec(host.VEC_LAMBDA),
                    misses=prof["speculation_misses"], solves=prof["cg_solves"], cg=prof["cg_iters"], kind=kind, mask=mask,
                    rank=s.block_shape(0)[1], shape=shape, handover=ho, eff=eff)
    finally:
        s.close()


def _same(a, b):
    for it, (x, y) in enumerate(zip(a["log"], b["log"])):
        assert x == y, (it, x, y)
    assert np.array_equal(a["lam"], b["lam"])
    for X, Y in zip(a["U"] + a["V"], b["U"] + b["V"]):
        assert np.array_equal(X, Y)
    assert (a["misses"], a["solves"], a["cg"]) == (b["misses"], b["solves"], b["cg"])


_ref = {}


def _compare(name, env, mask=None, tlr=None, rank=None, steps=24):
    """the run under `env` with LORADS_FRONT_CHAIN = `mask` (None: the default) against the same run at 0 (computed once per setting)"""
    path = _path(name)
    kw = dict(timesLogRank=tlr) if tlr else {}
    key = (name, tuple(sorted(env.items())), tlr, rank, steps)
    if key not in _ref:
        _ref[key] = _run(path, dict(env, LORADS_FRONT_CHAIN="0"), steps, rank=rank, **kw)
    b = _ref[key]
    a = _run(path, dict(env, **({} if mask is None else {"LORADS_FRONT_CHAIN": str(mask)})), steps, rank=rank, **kw)
    print(name, env, "mask", a["mask"], "rank", a["rank"], "misses", a["misses"], "solves", a["solves"], "cg", a["cg"],
          "hand-overs", a["handover"])
    assert b["mask"] == 0 and a["mask"] == (FC_ALL if mask is None else mask), (a["mask"], b["mask"])
    assert a["kind"] == b["kind"] == "k_cw+k_spmm_ell", (a["kind"], b["kind"])   # (the cone is on the k_front_cw path)
    _same(a, b)
    assert a["cg"] > a["solves"], (a["cg"], a["solves"])   # solves of more than one iteration as well
    return a


CW = {"LORADS_OP_CW": "1"}
_N = {"rand120": 120, "hub16": 810, "untouched130": 130}   # rows of the cone


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,tlr", [("rand120", CW, None), ("hub8", CW, None), ("hub16", CW, None), ("untouched130", CW, None),
                                          ("seam96", CW, None), ("rand4000", {}, 4.0)])
def test_default_cuts_are_bitwise_the_uncut_front(built, name, env, tlr):
    if name == "seam96":   # the head / CSR seam: rows with exactly 8, with 9 and with more than 16 neighbours
        counts = {len(r) for r in _objective_lists(_seam())}
        assert 8 in counts and 9 in counts and max(counts) >= 17, sorted(counts)
    a = _compare(name, env, tlr=tlr)
    if name == "rand4000":   # many workgroups, and the hand-over form of the front is live
        assert a["handover"]["on_front"] > 0, a["handover"]


VARIANTS = [("deal5", {"LORADS_ROW_DEAL": "5"}, None), ("deal32", {"LORADS_ROW_DEAL": "32"}, None),
            ("no_lds", {"LORADS_FRONT_LDS": "0"}, None), ("rank50", {}, 50), ("rank7", {}, -7),
            ("handover_alone", {"LORADS_HANDOVER_ON_FRONT": "0"}, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rand120", "hub16", "untouched130"])
@pytest.mark.parametrize("variant,env,rank", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_variants_are_bitwise_the_uncut_front(built, name, variant, env, rank):
    """rank 50: above the LDS park's 48 (grown to, the rank rule caps these cones below it); rank 7: odd, padded to 8 on the
    device (the rule gives ceil(timesLogRank * ln n), aimed at from below).  no_lds and rank50 launch the form without the
    park, which does not take the cuts: they pin the dispatch (the effective mask is 0, the same kernel runs on both sides),
    they do not cover the cuts."""
    tlr = None
    if rank is not None and rank < 0:
        rank, tlr = None, (-rank - 0.5) / np.log(_N[name])
    a = _compare(name, dict(CW, **env), tlr=tlr, rank=rank)
    assert a["eff"] == (0 if variant in ("no_lds", "rank50") else FC_ALL), (variant, a["eff"])
    if variant == "rank50":
        assert a["rank"] == 50, a["rank"]
    if variant == "rank7":
        assert a["rank"] == 7, a["rank"]


@pytest.mark.gpu
@pytest.mark.parametrize("bit", [1, 2])
def test_every_single_cut_is_bitwise_the_uncut_front(built, bit):
    _compare("hub16", CW, mask=bit)
