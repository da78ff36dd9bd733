"""The constraint-wise operator (kind 4) and its neighbours on constraints of UNEQUAL size, against the extended-precision models.

Every other kind-4 instance of the suite comes from instances.randsparse, whose constraints all have one size, and build_block
(csrc/hip/build.inc) then always lays the cone out the same way.  The instances here (lorads_amd/instances.py) have constraints of
1 .. 40 or 1 .. 256 entries, or one trace row next to single-entry rows, and reach

  * k_cw on the constraint CSR (ca_ell == 0): a trip count per wavefront, the odd tail of its two-entries-per-trip loop, constraints
    over one, two and three trips at 8 lanes per entry and over many at 32 and 64 (rank 258: lg_for = 64),
  * k_wsum over more than one trip of 32 contributions (cs_w > 32),
  * the older front under the constraint-wise operator because a few huge constraints leave no contribution array (cs_w == 0),
  * a dense objective on a kind-4 cone, which the cone takes without any switch (m >= 256),
  * kind-4 cones in a context of several cones, where row_idx is not the identity, merged and cone by cone,
  * the Gram form (k_cv, k_sgram, k_spmm2) on the same unequal rows (LORADS_OP_CW=0),
  * the CSR forms of the equal-size instances that only a switch reaches (LORADS_NO_ELL, LORADS_NO_SLOT_ELL),

and every case asserts from the library's own read-outs (operator kind, block image, lorads_hip_cw_layout) that it ran the form it
names.  The harnesses are run_case of tests/test_fixed_count_sweeps.py (ADMM) and of tests/test_fixed_count_alm.py (phase 1).

Bounds (ADMM).  Per case max(32 x spread, 1e-14), spread being the largest rel-to-scale difference between the model in float64 and
in long double over everything compared (the rule of tests/test_one_launch_variants.py), and never above 1e-11, the ceiling of
tests/test_fixed_count_sweeps.py: nothing of it comes from the device.  The CPU test below holds 32 x spread <= 1e-11 on every
instance at its default rank, so no case leans on the ceiling there.  The phase-1 cases keep that harness's own bounds.  The
figures measured on the MI355X stand next to the cases."""
import collections

import numpy as np
import pytest

from lorads_amd import host, instances
from tests import common
from tests import test_fixed_count_alm as alm
from tests.admm_model import AdmmModel
from tests.test_fixed_count_sweeps import FULL, RANKS, RHO, SHORT, find_stop, run_case

CEILING = 1e-11
CW = "k_cw+k_spmm_ell"
GRAM = "k_pairdots+k_sgram+k_spmm2"
S1, S2 = instances.SIZES_1_40, instances.SIZES_1_256

# instance: (the constraint sizes of its cones in file order, schedule of the plain ADMM case)
SIZES = {
    "mixsz130": ([[a + b for a, b in S1 * 2]], FULL),
    "bigsz200": ([[a + b for a, b in S2]], FULL),
    "mixsz300": ([[a + b for a, b in (S1 * 16)[:260]]], SHORT),
    "theta64x300": ([[64] + [1] * 300], FULL),
    "mixblk3": ([[a + b for a, b in S1], [a + b for a, b in S1[:12]] + [1] * 6, [1] * 50], FULL),
}
FORCED = {"mixsz130": {"LORADS_OP_CW": "1"}, "bigsz200": {"LORADS_OP_CW": "1"}, "mixsz300": {}, "theta64x300": {},
          "mixblk3": {"LORADS_OP_CW": "1"}}


def _path(name):
    return common.generated_instance(name)


def _bound(worst):
    return min(max(32.0 * worst["spread"], 1e-14), CEILING)


def _check(label, worst):
    b = _bound(worst)
    print(label, "worst", {k: "%.2e" % v for k, v in worst.items()}, "bound %.2e" % b, "used %.3f" % (
        max(worst["factors"], worst["vectors"], worst["scalars"]) / b))
    assert 32.0 * worst["spread"] <= CEILING, (label, "the model's own spread is above the ceiling: another seed", worst)
    assert worst["factors"] <= b and worst["vectors"] <= b and worst["scalars"] <= b, (label, worst, b)


# ---- CPU: the instances are what their size lists say, and the model alone finds the schedule's stops and agrees with itself
@pytest.mark.parametrize("name", sorted(SIZES))
def test_instances_and_model_spread(name):
    sizes, _ = SIZES[name]
    prob = instances.NAMED[name]()
    assert [abs(n) for n in prob["blocks"]] == {"mixsz130": [130], "bigsz200": [200], "mixsz300": [300], "theta64x300": [64],
                                                "mixblk3": [90, 70, 50]}[name]
    assert prob["m"] == sum(len(z) for z in sizes) and max(prob["blocks"]) <= 300 and prob["m"] <= 301
    count = collections.Counter((mat, blk) for mat, blk, i, j, v in prob["entries"] if mat > 0)
    got, m0 = [], 0
    for k, z in enumerate(sizes):  # (block_diag numbers the constraints cone after cone)
        got.append([count.get((m0 + i + 1, k + 1), 0) for i in range(len(z))])
        m0 += len(z)
    assert got == sizes and sum(count.values()) == sum(sum(z) for z in sizes), name
    assert len({(mat, blk, i, j) for mat, blk, i, j, v in prob["entries"]}) == len(prob["entries"]), "a position given twice"
    # the model alone on the FULL schedule from the seeded state, at the ranks a session gives the cones
    path = _path(name)
    s = host.Session.open(path)
    try:
        s.set_params(verbose=0)
        s.prepare(1, 0)
        U, V, lam = common.random_uv_state(s, 5)
    finally:
        s.close()
    model, m64 = AdmmModel.from_file(path), AdmmModel.from_file(path, dtype=np.float64)
    model.set_state(U, V, lam)
    m64.set_state(U, V, lam)
    stops, spread = [], 0.0
    for i, (kind, maxit, tol) in enumerate(FULL):
        if isinstance(tol, tuple):
            tol, maxit = find_stop(model, name, i, tol, maxit, False, stops)
        if kind == "sweep":
            (its, _), (its64, _) = model.sweep(RHO, tol, maxit), m64.sweep(RHO, tol, maxit)
        else:
            its, p, d, e, _ = model.step(RHO, tol, maxit)
            its64, p64, d64, e64, _ = m64.step(RHO, tol, maxit)
            dscale = float(np.sum(np.abs(model.b)) * np.max(np.abs(model.lam)))
            for x, y, sc in ((p64, p, 1.0), (d64, d, dscale), (e64, e, 0.0)):
                spread = max(spread, abs(float(x) - float(y)) / max(abs(float(y)), sc, 1e-300))
        assert its == its64, (name, i, "CG iterations of the model in float64", its64, its)
        for k in range(model.nb):
            spread = max(spread, common.rel_to_scale(m64.U[k], model.U[k]), common.rel_to_scale(m64.V[k], model.V[k]))
        spread = max(spread, common.rel_to_scale(m64.csum, model.csum))
        model.update_dual(RHO)
        m64.update_dual(RHO)
        spread = max(spread, common.rel_to_scale(m64.lam, model.lam))
    print(name, "stops", stops, "spread %.2e" % spread)
    assert len(stops) == 2 and all(stops) and len(set(stops)) == 2, (name, stops)
    assert 32.0 * spread <= CEILING, (name, spread)


# ---- GPU: ADMM sweeps
# mixblk3's Max-Cut cone (50 rows, 130 stored entries of C) has a DENSE objective by the reference's rule (more than 0.1 n (n + 1) / 2
# = 127.5 entries), and a context with a dense-C cone has no merged view (build_merged): its two kind-4 cones run cone by cone with
# and without LORADS_NO_MERGE.  mixblk3s is the same context with 60 edges in the Max-Cut cone (110 entries: sparse), which merges.
SEVERAL = ("mixblk3", "mixblk3s")

# group of cases: (worst device-against-model figure measured on the MI355X, its quantity and case, that case's bound by the rule
# above, the figure as a fraction of the bound).  No case came nearer to its bound than 0.043 of it, and no case found a kernel error;
# two mutated builds (k_cw's odd tail adding its second entry's coefficient; k_wsum stopping after two trips) failed 11 and 2 cases.
MEASURED = {
    "mixsz130, its three variants": (1.09e-15, "factors, default and LORADS_FUSE_CG0=0", 2.51e-14, 0.043),
    "bigsz200, by recurrence and LORADS_EXACT_REFRESH=1": (1.60e-15, "constraint sums, by recurrence", 4.73e-14, 0.034),
    "mixsz300 (SHORT), its three variants": (5.86e-15, "constraint sums, default", 4.99e-13, 0.012),
    "theta64x300, by recurrence and LORADS_EXACT_REFRESH=1": (1.55e-13, "pObj, by recurrence", 5.60e-12, 0.028),
    "mixblk3, its four variants": (1.61e-15, "factors, LORADS_FRONT_CW=0", 4.77e-14, 0.034),
    "mixblk3s, its four variants": (1.94e-15, "factors, merged", 4.77e-14, 0.041),
    "Gram form": (6.06e-14, "constraint sums and scalars, theta64x300 (0.011 of its bound; mixsz130 9.6e-16 is 0.038 of its own)", 5.60e-12, 0.011),
    "CSR forms of rand120 and hub16": (1.18e-14, "factors, hub16 LORADS_NO_SLOT_ELL", 2.99e-13, 0.039),
    "rank walk": (4.44e-15, "factors, r 66 (r 258: 6.2e-16, 0.022 of its bound 2.85e-14)", 1.27e-13, 0.035),
    "phase 1": (1.3e-14, "D/R/Grad, bigsz200 (both paths)", 6.29e-13, 0.020),
}


def _mixblk3s():
    return instances.block_diag([instances.randsparse_sizes(90, S1, 2207, 180),
                                 instances.randsparse_sizes(70, S1[:12] + [(0, 1)] * 6, 2208, 140), instances.maxcut(50, 60, 5)])


def _file(name):
    return common.generated_instance(name, make=_mixblk3s) if name == "mixblk3s" else _path(name)


def _assert_layout(name, facts):
    """the forms each instance is there for, from the library's read-outs; returns cone 0's front_cw"""
    kinds, im, lay = facts["kinds"], facts["images"], facts["layouts"]
    print(name, "kinds", kinds, "layouts", lay, "front_cw", [x["front_cw"] for x in im], "dense_c", [x["dense_c"] for x in im],
          "ranks", facts["ranks"])
    cw = [0, 1] if name in SEVERAL else [0]
    if name in SEVERAL:
        assert kinds == [CW, CW, "k_op_diag"], kinds
        assert lay[2] == dict(ca_ell=0, cs_w=0, cell_w=0, rows_over=0) and im[2]["use_cw"] == 0, (lay[2], im[2])
        assert im[2]["dense_c"] == (1 if name == "mixblk3" else 0), im[2]
    else:
        assert kinds == [CW], kinds
    for k in cw:
        assert im[k]["use_cw"] == 1 and lay[k]["ca_ell"] == 0 and lay[k]["cell_w"] == im[k]["slot_width"] > 0, (k, im[k], lay[k])
    if name in ("mixsz130", "mixsz300"):
        assert im[0]["front_cw"] == 1 and lay[0]["cs_w"] > 64 and im[0]["dense_c"] == 0, (im[0], lay[0])  # (three trips of k_wsum)
    if name in SEVERAL:  # (three trips and two)
        assert all(im[k]["front_cw"] == 1 and im[k]["dense_c"] == 0 for k in cw) and lay[0]["cs_w"] > 64 and lay[1]["cs_w"] > 32, (im, lay)
    if name == "bigsz200":
        assert im[0]["front_cw"] == 0 and lay[0]["cs_w"] == 0 and im[0]["dense_c"] == 0, (im[0], lay[0])
    if name == "theta64x300":
        assert im[0]["front_cw"] == 0 and lay[0]["cs_w"] == 0 and im[0]["dense_c"] == 1, (im[0], lay[0])
    if name in ("mixsz300", "theta64x300"):
        assert im[0]["nrow"] >= 256  # (kind 4 without a switch)
    if name in ("bigsz200", "mixsz300", "theta64x300"):
        assert lay[0]["rows_over"] > 0, lay[0]  # (rows whose tails run on the CSR slot list)
    return im[0]["front_cw"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixsz130", "bigsz200", "mixsz300", "theta64x300", "mixblk3", "mixblk3s"])
def test_constraint_wise_forms_on_unequal_constraints(built, name):
    env, schedule = FORCED[name.rstrip("s")], SIZES[name.rstrip("s")][1]
    facts, worst = run_case(name, env, schedule=schedule, path=_file(name), spread=True)
    front = _assert_layout(name, facts)
    _check("%s %s" % (name, env), worst)
    assert front == (0 if name in ("bigsz200", "theta64x300") else 1)
    variants = [{"LORADS_FUSE_CG0": "0"}, {"LORADS_FRONT_CW": "0"}] if front else [{"LORADS_EXACT_REFRESH": "1"}]
    if name in SEVERAL:
        variants.append({"LORADS_NO_MERGE": "1"})
    for extra in variants:
        f2, w2 = run_case(name, dict(env, **extra), schedule=schedule, path=_file(name), spread=True)
        assert _assert_layout(name, f2) == front
        print(name, extra, "launches", f2["launches"], "default", facts["launches"])
        # the default case really ran the CG0 form / the one-kernel front (one cone) and the merged view (mixblk3s): each of
        # these switches costs launches
        if (name not in SEVERAL and "LORADS_EXACT_REFRESH" not in extra) or (name == "mixblk3s" and "LORADS_NO_MERGE" in extra):
            assert facts["launches"] < f2["launches"], (extra, facts["launches"], f2["launches"])
        _check("%s %s" % (name, dict(env, **extra)), w2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixsz130", "bigsz200", "theta64x300"])
def test_gram_form_on_unequal_constraints(built, name):
    """LORADS_OP_CW=0: k_cv, k_sgram and k_spmm2 walk the constraint CSR of unequal rows (a sparse C, and theta64x300's dense C)"""
    facts, worst = run_case(name, {"LORADS_OP_CW": "0"}, path=_path(name), spread=True)
    im, lay = facts["images"][0], facts["layouts"][0]
    assert facts["kinds"] == [GRAM] and im["use_cw"] == 0 and im["has_gram"] == 1, (facts["kinds"], im)
    assert lay == dict(ca_ell=0, cs_w=0, cell_w=0, rows_over=0), lay
    assert im["dense_c"] == (1 if name == "theta64x300" else 0), im
    _check("%s Gram form" % name, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["LORADS_NO_ELL", "LORADS_NO_SLOT_ELL"])
@pytest.mark.parametrize("name", ["rand120", "hub16"])
def test_csr_forms_of_equal_size_instances(built, name, switch):
    """k_cw on the constraint CSR / k_spmm<CW> on the CSR slot list, on instances whose default layout is the fixed-width one"""
    base, _ = run_case(name, {"LORADS_OP_CW": "1"}, schedule=RANKS)
    assert base["layouts"][0]["ca_ell"] > 0 and base["layouts"][0]["cell_w"] > 0, base["layouts"]
    facts, worst = run_case(name, {"LORADS_OP_CW": "1", switch: "1"}, spread=True)
    im, lay = facts["images"][0], facts["layouts"][0]
    print(name, switch, "layout", lay, "front_cw", im["front_cw"])
    assert facts["kinds"] == [CW] and im["use_cw"] == 1, (facts["kinds"], im)
    if switch == "LORADS_NO_ELL":
        assert lay["ca_ell"] == 0 and lay["cell_w"] == base["layouts"][0]["cell_w"] and im["front_cw"] == 1, (lay, im)
    else:  # (no fixed-width slot list: no one-kernel front either, and every row with a slot counts as over the width)
        assert lay["cell_w"] == 0 and lay["cs_w"] == 0 and im["front_cw"] == 0 and lay["rows_over"] > 0, (lay, im)
        assert lay["ca_ell"] == base["layouts"][0]["ca_ell"], lay
    _check("%s %s" % (name, switch), worst)


# 8 lanes per entry up to rank 128 (even) and at 41 unpadded, 32 at 130 and 200, 64 at 258 (lg_for)
@pytest.mark.gpu
@pytest.mark.parametrize("r", [2, 8, 40, 41, 66, 130, 200, 258])
def test_rank_walk_on_the_constraint_csr(built, r):
    env = {"LORADS_OP_CW": "1"}
    for e in [env] + ([dict(env, LORADS_PAD_ODD_RANK="0")] if r % 2 else []):
        facts, worst = run_case("mixsz130", e, params=dict(timesLogRank=0.1), schedule=RANKS, ranks=r, path=_path("mixsz130"),
                                spread=True)
        assert facts["ranks"] == [r] and facts["kinds"] == [CW] and facts["layouts"][0]["ca_ell"] == 0, facts
        assert facts["layouts"][0]["cs_w"] > 64, facts["layouts"]
        _check("mixsz130 r %d %s" % (r, e), worst)


# ---- GPU: phase 1 (the bounds are that harness's own: the model's spread per case, nothing from the device)
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "slots"])
@pytest.mark.parametrize("name", ["mixsz130", "bigsz200", "theta64x300"])
def test_phase_1_on_unequal_constraints(built, name, path):
    facts, worst, bound, _ = alm.run_case(name, FORCED[name], path=path, file=_path(name))
    im, lay = facts["images"][0], facts["layouts"][0]
    print(name, path, "layout", lay, "bound %.2e" % bound, "used %.3f" % (max(worst.values()) / bound))
    assert facts["kinds"] == [CW] and im["use_cw"] == 1 and lay["ca_ell"] == 0, (facts["kinds"], im, lay)
    assert im["dense_c"] == (1 if name == "theta64x300" else 0), im
