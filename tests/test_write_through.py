"""The row outputs of k_front_cw and k_spmm_ell stored through the L2 (LORADS_WT_STORES).

The switch picks the store instruction of six arrays (bit 0 the front's initial residual, 1 its right-hand side, 2 the slot
contributions, 3 x and r of CG iteration 0 inside k_spmm_ell, 4 the average R written there, 5 the output of the plain k_spmm_ell)
and moves no arithmetic, so every comparison here is bit for bit: the per-step log (CG count, pObj, dObj, err1), U, V, lambda, the
total CG iterations and solves.  The schedule is the one of tests/test_row_deal.py (tolerances that change from step to step:
speculation misses, gated-off launches, every third step through the separate entry points)."""
import functools

import pytest

from lorads_amd import host
from tests import common
from tests import test_fixed_count_sweeps as fcs
from tests import test_row_deal as rd

FULL = 63
BITS = {1: "front r0", 2: "front rhs", 4: "contributions", 8: "CG0 x and r", 16: "average R", 32: "plain out"}


@functools.lru_cache(maxsize=None)
def _wt(name, mask, deal=None, repeat=False, extra=()):
    """test_row_deal's run with LORADS_WT_STORES=`mask`, plus the mask the very context that ran it reports (key "wt"); once per
    test process, left unchanged by whoever reads it"""
    seen = []
    orig = common.hip_session_with_env

    def session(path, env, params, separable=None):
        s = orig(path, env, params, separable)
        seen.append(s.hip_wt_stores())
        return s

    common.hip_session_with_env = session
    try:
        res = rd._run_fresh(name, deal, (("LORADS_WT_STORES", str(mask)),) + tuple(extra), repeat)
    finally:
        common.hip_session_with_env = orig
    (wt,) = seen
    return dict(res, wt=wt)


def _same(a, b, mask):
    assert a["wt"] == mask and b["wt"] == 0, (a["wt"], b["wt"])
    assert a["kind"] == fcs.CW and a["image"]["front_cw"] == 1, (a["kind"], a["image"])
    assert a["deal"] == b["deal"]
    rd._assert_bitwise(a, b)


# ---- 1. every array through the L2 against plain stores everywhere
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rand120", "rand123", "hub16", "wide60", "rand4000"])
def test_full_mask_is_bitwise_plain_stores(built, name):
    a, b = _wt(name, FULL), _wt(name, 0)
    if name == "rand123":  # (a partial last workgroup: its inactive lane groups store nothing, whatever the instruction)
        assert a["n"] % a["deal"]["rpw"] != 0, a["deal"]
    if name == "hub16":    # (rows 0-2 hold 60 slots, more than either fixed width: the CSR-tail contribution stores run)
        assert 0 < a["image"]["slot_width"] <= 16
    if name == "rand4000":  # (the `j0 < r` edge of the last column slice)
        assert a["image"]["rank"] % 16 != 0, a["image"]
    print(name, "speculative fronts", a["spec"], "cg per step", [x[0] for x in a["log"]])
    if name == "rand120":  # (fronts enqueued ahead of their step were taken and were discarded: both launch paths stored)
        assert a["spec"]["adopted"] > 0, a["spec"]
    _same(a, b, FULL)


# ---- 2. the mask travels in the kernel arguments, so it survives the replay of captured launch chains
@pytest.mark.gpu
def test_full_mask_under_graph_replay(built):
    g = (("LORADS_GRAPH", "1"),)
    a, b = _wt("rand120", FULL, None, True, g), _wt("rand120", 0, None, True, g)
    print("graphs", a["graphs"], b["graphs"])
    assert a["graphs"]["replayed"] >= 10 and b["graphs"]["replayed"] >= 10, (a["graphs"], b["graphs"])
    _same(a, b, FULL)


# ---- 3. array by array
@pytest.mark.gpu
@pytest.mark.parametrize("bit", sorted(BITS))
def test_single_bit_is_bitwise_plain_stores(built, bit):
    _same(_wt("hub16", bit), _wt("hub16", 0), bit)


@pytest.mark.gpu
def test_reported_mask(built):
    """what the context reports is what its kernels get: bits beyond the six arrays are dropped, an unset switch gives the default"""
    assert sorted(BITS) == [1 << i for i in range(6)] and sum(BITS) == FULL
    env, params, _ = rd.CASES["rand120"]
    for setting, want in (("255", FULL), ("0", 0), ("5", 5), (None, None)):
        e = dict(env) if setting is None else dict(env, LORADS_WT_STORES=setting)
        s = common.hip_session_with_env(rd._path("rand120"), e, dict(params, phase1Tol=1e-2))
        try:
            got = s.hip_wt_stores()
        finally:
            s.close()
        assert (0 <= got <= FULL) if want is None else got == want, (setting, got)


# ---- 4. together with forced row deals: workgroups with three wavefronts idle (5) and a tile that is no multiple of eight (27)
@pytest.mark.gpu
@pytest.mark.parametrize("deal", [5, 27])
def test_full_mask_at_forced_deals(built, deal):
    a, b = _wt("rand123", FULL, deal), _wt("rand123", 0, deal)
    assert a["deal"]["rpw"] == deal and a["n"] % deal != 0, a["deal"]
    _same(a, b, FULL)


# ---- 5. the 8-byte row stores
def _run_odd(mask, r=7, steps=6):
    """rand120 at rank `r` (odd) as it is, LORADS_PAD_ODD_RANK=0, from a seeded (U, V, lambda): `steps` ADMM steps"""
    env = {"LORADS_OP_CW": "1", "LORADS_PAD_ODD_RANK": "0", "LORADS_WT_STORES": str(mask)}
    s = common.hip_session_with_env(rd._path("rand120"), env, dict(timesLogRank=0.1))  # (a small rank to grow from)
    try:
        s.be.resize_rank([r] * s.nblk)
        U, V, lam = common.random_uv_state(s, 5)
        common.load_uv_state(s.be, U, V, lam)
        log = [s.be.admm_step(1.5, [1e-6, 1e-10, 1e-3][it % 3], 40) for it in range(steps)]
        prof = s.hip_profile_read()
        return dict(log=log, U=s.be.get_mat(host.MAT_U, 0), V=s.be.get_mat(host.MAT_V, 0), lam=s.be.get_vec(host.VEC_LAMBDA),
                    cg=prof["cg_iters"], solves=prof["cg_solves"], wt=s.hip_wt_stores(), kind=s.hip_operator_kind(0),
                    image=s.hip_block_image(0), shape=s.block_shape(0))
    finally:
        s.close()


@pytest.mark.gpu
def test_eight_byte_row_stores(built):
    """Reachable in the plain form only: an odd rank that is not padded to even (LORADS_PAD_ODD_RANK=0) runs the operator's second
    half as k_spmm_ell<8, false, NS, EW>, whose `out` rows are stored one double at a time (bit 5: store8).  The one-kernel front and
    the CG0 form exist for even ranks alone (front_cw_ok and spmm_cw ask for 16-byte rows), so bits 0-4 have no 8-byte row form to
    reach; the contributions (bit 2) are 8-byte stores at every rank and run in every other test of this file."""
    a, b = _run_odd(32), _run_odd(0)
    assert (a["wt"], b["wt"]) == (32, 0)
    assert a["shape"][1] == 7 and a["image"]["rank"] == 7, (a["shape"], a["image"])
    # the fixed-width slot list is there and the cone is on the k_cw path: spmm_cw launches k_spmm_ell, not the CSR fallback
    assert a["kind"] == fcs.CW and a["image"]["use_cw"] == 1 and a["image"]["slot_width"] in (8, 16), (a["kind"], a["image"])
    assert a["cg"] > a["solves"] > 0, (a["cg"], a["solves"])  # (iterations beyond 0: the plain form ran)
    rd._assert_bitwise(a, b)
