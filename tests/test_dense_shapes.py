"""The dense-coefficient GEMM (k_dense_cx_b + k_sum_slabs: a dense objective, dense constraint matrices) at every tile shape, and the
products kept from it (Block::wj_for), against the extended-precision models (tests/admm_model.py, tests/alm_model.py).

The kernel has one instantiation per (NT column tiles of 16, REM single columns); ranks above 128 take several launches (col0 = 128,
256, 384); the K range is split over 1, 2, 4, 8 or 16 workgroups whose slabs k_sum_slabs adds; the cone's dimension is padded to 64,
so the last workgroups hold rows past n and the last k-rows lie beyond it.  Every case runs fixed-count sweeps (run_case of
tests/test_fixed_count_sweeps.py) or consecutive phase-1 iterations (run_case of tests/test_fixed_count_alm.py) from
timesLogRank = 0.1 grown to the wanted rank, and asserts what was launched from the library's own plan (Session.hip_dense_plan)
against the rule restated here (`rule`) and against the figures of SIZES: a case that silently runs another shape fails.

    name        n     npad  K split  k trips  what the size is for
    densec33    33    64    1        1        the second workgroup holds one real row
    densea32    32    64    1        1        the smallest cone that keeps a constraint dense; the second workgroup all past n
                                              (72 stored entries of C against a threshold of 52.8: its objective is stored dense too)
    densec65    65    128   2        1        slabs; the third workgroup one row, the fourth none
    densea65    65    128   2        1        the same with three dense constraints
    densec190   190   192   1        3        several trips of the k loop, n % 32 = 30
    denseac200  200   256   4        1        dense C and dense A_i together
    densec370   370   384   2        3        split and trips together
    densec500   500   512   8        1
    densec1000  1000  1024  16       1        the cap of the split, n % 32 = 8

Bounds: BOUNDS["default"] of tests/test_fixed_count_sweeps.py (1e-12, relative to the vector's largest entry) for the sweeps and the
kept-product sequences; CG counts and stopping iterations exact; phase 1 by the rule of tests/test_fixed_count_alm.py
(max(32 x the float64 model's distance from the longdouble model, 1e-14), never above 1e-11), which the single phase-1 front of the
kept-product sequences follows too.  Nothing is taken from the device.  MEASURED holds the worst figure seen on the MI355X per group."""
import contextlib

import numpy as np
import pytest

from lorads_amd import host, instances
from tests import common
from tests import test_fixed_count_alm as alm
from tests import test_fixed_count_sweeps as sweeps
from tests.admm_model import LD, AdmmModel
from tests.alm_model import BOUND_CEILING, BOUND_FACTOR, BOUND_FLOOR, AlmModel, record_errors

pytestmark = pytest.mark.gpu

BOUND = sweeps.BOUNDS["default"]
RHO = sweeps.RHO
# group of cases: (worst device-against-model figure measured on the MI355X, where, the bound)
MEASURED = {
    "rank walk, n = 65": (3.4e-15, "densea65", 1e-12),
    "size walk": (6.5e-14, "constraint sums, densec370 at rank 18; every other case <= 7.1e-15", 1e-12),
    "tolerance stops": (1.1e-14, "constraint sums, densec65 (stops at 4 and 2; densea65 at 3 and 6)", 1e-12),
    "switches, replay": (1.1e-15, "densea65", 1e-12),
    "phase 1": (2.0e-14, "0.03 of its case's bound at most (densea65, rank 66)", (9.5e-14, 1.1e-12)),
    "kept products, ADMM sequences": (6.6e-15, "denseac200 behind resize_rank", 1e-12),
    "kept products, phase-1 front": (3.5e-16, "denseac200; 2.7e-2 before lorads_hip_lbfgs_direction dropped the products", (4.1e-14, 6.4e-14)),
}
# The whole file: 83 cases, 47 s on the MI355X (the longest: denseac200 at rank 146, 7 s, nearly all of it the model).

_rs = instances.randsparse
INST = {
    "densec33": lambda: _rs(33, 8, 9033, n_diag=1, n_off=2, r0=2, dense_c=True),
    "densea32": lambda: instances.with_dense_constraints(_rs(32, 8, 9032, c_edges=40, n_diag=1, n_off=2, r0=2), 2, 9132),
    "densec65": lambda: _rs(65, 8, 9065, n_diag=1, n_off=2, r0=2, dense_c=True),
    "densea65": lambda: instances.with_dense_constraints(_rs(65, 8, 9066, c_edges=40, n_diag=1, n_off=2, r0=2), 3, 9166),
    "densec190": lambda: _rs(190, 8, 9190, n_diag=1, n_off=2, r0=2, dense_c=True),
    "denseac200": None,  # (instances.NAMED)
    "densec370": lambda: _rs(370, 8, 9370, n_diag=1, n_off=2, r0=2, dense_c=True),
    "densec500": lambda: _rs(500, 20, 9500, n_diag=1, n_off=2, r0=2, dense_c=True),
    "densec1000": lambda: _rs(1000, 20, 9999, n_diag=1, n_off=2, r0=2, dense_c=True),
}
# name: (n, npad, K split, trips of the k loop, objective stored dense, dense constraint matrices) -- the table above
SIZES = {
    "densec33": (33, 64, 1, 1, 1, 0), "densea32": (32, 64, 1, 1, 1, 2), "densec65": (65, 128, 2, 1, 1, 0), "densea65": (65, 128, 2, 1, 0, 3),
    "densec190": (190, 192, 1, 3, 1, 0), "denseac200": (200, 256, 4, 1, 1, 3), "densec370": (370, 384, 2, 3, 1, 0),
    "densec500": (500, 512, 8, 1, 1, 0), "densec1000": (1000, 1024, 16, 1, 1, 0),
}
RANK_LIST = [2, 17, 19, 22, 36, 50, 66, 80, 100, 116, 128, 146, 258]
RANKS_PAD = [(r, pad) for r in RANK_LIST for pad in ([True, False] if r % 2 else [True])]  # (an odd rank also unpadded)


def _file(name):
    return common.generated_instance(name) if INST[name] is None else common.generated_instance("shapes_" + name, make=INST[name])


def rule(n, r, rem_on=True):
    """(plan, trips of the k loop) of the dense GEMM for a cone of dimension n at device rank r: build_block's K split (doubled while
    the grid holds fewer than 512 workgroups, each half stays a multiple of 64 rows and the split is below 16) and dense_cx's tiles
    (cols = min(r - col0, 128), nt = ceil(cols / 16), a last tile of 1..4 columns becomes REM when nt >= 2 and LORADS_DENSE_REM is on)"""
    npad = -(-n // 64) * 64
    ks = 1
    while ks < 16 and (npad // 32) * ks < 512 and (npad // (2 * ks)) % 64 == 0:
        ks *= 2
    launches = []
    for col0 in range(0, r, 128):
        cols = min(r - col0, 128)
        nt, rem = -(-cols // 16), 0
        if 1 <= cols % 16 <= 4 and nt >= 2 and rem_on:
            nt, rem = nt - 1, cols % 16
        launches.append((col0, nt, rem))
    return dict(npad=npad, ksplit=ks, launches=launches), npad // ks // 64  # (four wavefronts on a quarter each, 16 k-rows per trip)


def _dev_rank(r, pad=True):
    return r + 1 if pad and r % 2 and r < 512 else r


def _env(env, pad):
    return dict(env or {}, **({} if pad else {"LORADS_PAD_ODD_RANK": "0"}))


def _shape(plan):
    """a plan without the word on the kept products"""
    return {k: v for k, v in plan.items() if k != "kept"}


def _ran_as_planned(name, facts, r, pad=True, rem_on=True, dense_a=None):
    """the case ran the shape it names: the library's plan is the rule's and the table's, the storage is what the table says"""
    n, npad, ks, trips, dense_c, nd = SIZES[name]
    nd = nd if dense_a is None else dense_a
    plan, want_trips = rule(n, _dev_rank(r, pad), rem_on)
    assert facts["ranks"] == [r], facts["ranks"]
    assert (plan["npad"], plan["ksplit"], want_trips) == (npad, ks, trips), (name, plan, want_trips)
    im = facts["images"][0]
    assert (im["n"], im["dense_c"], im["dense_a"]) == (n, dense_c, nd), im
    if dense_c or nd:
        assert [_shape(d) for d in facts["dense"]] == [plan], (name, r, pad, facts["dense"], plan)
    else:
        assert facts["dense"] == [dict(npad=0, ksplit=0, launches=[], kept="")], facts["dense"]
    assert ("dense A_i" in facts["kinds"][0]) == (nd > 0), facts["kinds"]
    return plan


def _admm(name, r, env=None, pad=True, schedule=sweeps.RANKS, rem_on=True, dense_a=None):
    facts, worst = sweeps.run_case(name, _env(env, pad), params=dict(timesLogRank=0.1), schedule=schedule, ranks=r, path=_file(name))
    plan = _ran_as_planned(name, facts, r, pad, rem_on, dense_a)
    sweeps._check(worst)
    return facts, worst, plan


# ---- what the lists cover, from the library's own plans
def test_rank_list_covers_every_instantiation(built):
    """every NT in 1..8, every REM in 0..4 and a launch at col0 > 0 with REM > 0 occur over the rank walk, by the plans the library
    gives at those ranks (grown in one session, padded and unpadded), each equal to the rule"""
    seen = []
    for pad in (True, False):
        s = sweeps._session(_file("densec65"), _env({}, pad), dict(timesLogRank=0.1))
        try:
            for r in RANK_LIST:
                if not pad and r % 2 == 0:
                    continue
                s.be.resize_rank([r])
                plan = _shape(s.hip_dense_plan(0))
                assert plan == rule(65, _dev_rank(r, pad))[0], (r, pad, plan)
                seen += plan["launches"]
            assert s.hip_dense_plan(0)["launches"][-1][0] == (256 if pad else 0), s.hip_dense_plan(0)
        finally:
            s.close()
    assert {nt for _, nt, _ in seen} == set(range(1, 9)), sorted(seen)
    assert {rem for _, _, rem in seen} == set(range(5)), sorted(seen)
    assert any(col0 > 0 and rem > 0 for col0, _, rem in seen), sorted(seen)
    assert {col0 for col0, _, _ in seen} == {0, 128, 256}, sorted(seen)


def test_size_table_covers_every_split():
    """K splits 1, 2, 4, 8, 16, one and several trips of the k loop, by the rule; every case asserts its row of the table against the
    library's plan (_ran_as_planned)"""
    for name, (n, npad, ks, trips, _, _) in SIZES.items():
        plan, t = rule(n, 18)
        assert (plan["npad"], plan["ksplit"], t) == (npad, ks, trips), (name, plan, t)
    assert {v[2] for v in SIZES.values()} == {1, 2, 4, 8, 16}
    assert {v[3] for v in SIZES.values()} == {1, 3}
    assert {(v[2] > 1, v[3] > 1) for v in SIZES.values()} == {(False, False), (True, False), (False, True), (True, True)}


def test_cone_without_dense_storage_has_no_plan(built):
    s = sweeps._session(common.instance_path("rand120"), {}, {})
    try:
        assert s.hip_dense_plan(0) == dict(npad=0, ksplit=0, launches=[], kept="") and s.hip_block_image(0)["dense_c"] == 0
    finally:
        s.close()


# ---- ADMM: the rank walk and the size walk
@pytest.mark.parametrize("r,pad", RANKS_PAD)
@pytest.mark.parametrize("name", ["densec65", "densea65"])
def test_rank_walk(built, name, r, pad):
    _admm(name, r, pad=pad)


SIZE_WALK = [(name, r) for name in SIZES for r in (18, 34) if (name, r) != ("densec1000", 34)] + [
    ("denseac200", 146), ("densec500", 66), ("densec370", 258)]  # (three crossings of a split with more tiles and more launches)


@pytest.mark.parametrize("name,r", SIZE_WALK)
def test_size_walk(built, name, r):
    _admm(name, r)


@pytest.mark.parametrize("name", ["densea65", "densec65"])
def test_tolerance_stops(built, name):
    """the FULL schedule: solves that a tolerance found from the model stops early, at two different iterations -- the kept products
    across solves that end early and across the speculation miss (which clears them)"""
    facts, _, _ = _admm(name, 34, schedule=sweeps.FULL)
    assert len(facts["stops"]) == 2 and all(facts["stops"]), facts["stops"]


# ---- the switches, each against the model
@pytest.mark.parametrize("r,want", [(18, [(0, 2, 0)]), (36, [(0, 3, 0)])])
def test_single_columns_on_a_tile_of_their_own(built, r, want):
    """LORADS_DENSE_REM=0: no single columns, one tile more (the default plans: [(0, 1, 2)] and [(0, 2, 4)])"""
    _, _, plan = _admm("densec65", r, {"LORADS_DENSE_REM": "0"}, rem_on=False)
    assert plan["launches"] == want and rule(65, r)[0]["launches"] == [(0, want[0][1] - 1, r % 16)], plan


def test_products_formed_per_application(built):
    """LORADS_DENSE_CACHE=0: nd + 1 GEMMs per operator application instead of nd per solve -- more launches for the same schedule"""
    kept, _, _ = _admm("densea65", 34)
    per, _, _ = _admm("densea65", 34, {"LORADS_DENSE_CACHE": "0"})
    assert per["launches"] > kept["launches"], (per["launches"], kept["launches"])


def test_dense_constraints_left_in_the_sparse_structures(built):
    """LORADS_NO_DENSE_A=1: the same constraints through the sparse kernels (no dense storage, no plan)"""
    facts, _, _ = _admm("densea65", 34, {"LORADS_NO_DENSE_A": "1"}, dense_a=0)
    assert "dense" not in facts["kinds"][0], facts["kinds"]


def test_replayed_steps_of_a_dense_constraint_cone(built):
    """LORADS_GRAPH=1: a step whose launch chain has been seen is replayed as a captured graph; the chain is keyed on the array the
    kept products belong to, and a replay puts that back"""
    facts, _, _ = _admm("densea65", 18, {"LORADS_GRAPH": "1"}, schedule=[("step", 2, 0.0)] * 8)
    assert facts["graph"]["enabled"] == 1 and facts["graph"]["replayed"] > 0, facts["graph"]


# ---- phase 1: the gradient's dense part and the (R, D) constraint values through the same GEMM, no kept products
@pytest.mark.parametrize("r,pad", [(18, True), (19, False), (66, True), (146, True)])
@pytest.mark.parametrize("name", ["densec65", "densea65", "denseac200"])
def test_phase_one(built, name, r, pad):
    for path in ("fused", "slots"):
        facts, _, _, _ = alm.run_case(name, _env({}, pad), params=dict(timesLogRank=0.1), schedule=alm.SHORT, ranks=r, path=path,
                                      file=_file(name))
        _ran_as_planned(name, facts, r, pad)
        assert facts["team"]["launches"] == 0, facts["team"]  # (the one-launch direction steps aside for dense storage)


# ---- the kept products W_j = A_j Y (and C Y): whoever overwrites Y has to drop them
class _Pair:
    """a session and the model in the same seeded ADMM state at rank r; every step runs on both and compares U, V and the constraint
    sums (the model's own: both sides have formed them by the same calls)"""

    def __init__(self, name, r, seed=5):
        self.file = _file(name)
        self.s = sweeps._session(self.file, {}, dict(timesLogRank=0.1))
        self.be, self.nb = self.s.be, self.s.nblk
        self.be.resize_rank([r] * self.nb)
        self.model = AdmmModel.from_file(self.file)
        U, V, lam = common.random_uv_state(self.s, seed)
        common.load_uv_state(self.be, U, V, lam)
        self.model.set_state(U, V, lam)
        self.worst = 0.0
        self.rng = np.random.default_rng(seed + 100)

    def check(self, what):
        errs = [common.rel_to_scale(self.be.get_vec(host.VEC_CONSTR_SUM), self.model.csum)]
        for k in range(self.nb):
            errs.append(common.rel_to_scale(self.be.get_mat(host.MAT_U, k), self.model.U[k]))
            errs.append(common.rel_to_scale(self.be.get_mat(host.MAT_V, k), self.model.V[k]))
        self.worst = max(self.worst, max(errs))
        assert max(errs) <= BOUND, (what, "constraint sums, then U and V per cone", errs)

    def sweep(self, what, kind="sweep", maxit=2):
        if kind == "sweep":
            its, mits = self.be.admm_update_var(RHO, 0.0, maxit), self.model.sweep(RHO, 0.0, maxit)[0]
        else:
            its, mits = self.be.admm_step(RHO, 0.0, maxit)[0], self.model.step(RHO, 0.0, maxit)[0]
        assert its == mits, (what, its, mits)
        self.check(what)

    def kept(self):
        return self.s.hip_dense_plan(0)["kept"]

    def settle(self, kind="sweep"):
        """sweeps until the kept products belong to the U array, the fixed factor of a sweep's last solve.  (A context's first sweep
        has no CG counts to speculate on: it misses, and the miss drops the products.)  A sequence that then overwrites U meets them."""
        for i in range(4):
            self.sweep("settling %s %d" % (kind, i), kind)
            if self.kept() == "U":
                return
        raise AssertionError("no sweep left the products of the U array kept: the sequence would test nothing (%r)" % self.kept())

    def init_constr(self, what):
        self.be.init_constr(host.PAIR_UV)
        self.model.init_constr()
        self.check(what)

    def fresh(self, k=0):
        n, r = self.s.block_shape(k)
        return self.rng.standard_normal((n, r)) / np.sqrt(r)


@contextlib.contextmanager
def _pair(name, r):
    p = _Pair(name, r)
    try:
        yield p
        print(name, "rank", r, "worst %.2e" % p.worst)
    finally:
        p.s.close()


@pytest.mark.parametrize("name", ["densea65", "denseac200"])
def test_kept_products_after_set_mat(built, name):
    """a new U while the products of the U array are kept (init_constr(PAIR_UV) would take <V, A_j U_old> from them), then a new V
    after a step"""
    with _pair(name, 18) as p:
        p.settle()
        for which, kind in ((host.MAT_U, "sweep"), (host.MAT_V, "step")):
            if kind == "step":
                p.sweep("step before set_mat", kind)
            assert which != host.MAT_U or p.kept() == "U", p.kept()
            for k in range(p.nb):
                F = p.fresh(k)
                p.be.set_mat(which, k, F)
                (p.model.U if which == host.MAT_U else p.model.V)[k] = F.astype(LD)
            p.init_constr("constraint values of the new factor")
            p.sweep("%s behind set_mat" % kind, kind)


@pytest.mark.parametrize("name", ["densea65", "denseac200"])
def test_kept_products_after_resize_rank(built, name):
    """18 -> 34 while the products of the U array are kept: the old columns stay, new column j holds 1 / sqrt(16) in row j
    (lorads_hip_resize_rank), and the products of the narrower U must not be met by its address"""
    with _pair(name, 18) as p:
        p.settle()
        p.be.resize_rank([34] * p.nb)
        for F in (p.model.U, p.model.V):
            for k in range(p.nb):
                n, aug = F[k].shape[0], 34 - 18
                G = np.zeros((n, 34), dtype=LD)
                G[:, :18] = F[k]
                for j in range(min(n, aug)):
                    G[j, 18 + j] = 1 / np.sqrt(LD(min(n, aug)))
                F[k] = G
        assert _shape(p.s.hip_dense_plan(0)) == rule(SIZES[name][0], 34)[0], p.s.hip_dense_plan(0)
        p.init_constr("constraint values at the new rank")
        p.sweep("sweep at the new rank")
        p.sweep("step at the new rank", "step")


def test_kept_products_after_scale_obj(built):
    """denseac200 keeps C Y beside the A_j Y: C and lambda times 0.5 between sweeps.  (Between whole sweeps the products kept are
    those of the U array and the next sweep's first solve forms those of V anew, so no order of whole calls meets a C Y of the
    old C: the sequence pins the results, it cannot show the clear of lorads_hip_scale_obj missing.)"""
    with _pair("denseac200", 18) as p:
        p.settle()
        p.be.scale_obj(0.5)
        p.model.scale_obj(0.5)
        p.sweep("sweep with the scaled objective")
        p.sweep("step with the scaled objective", "step")


@pytest.mark.parametrize("name", ["densea65", "denseac200"])
def test_kept_products_after_average_uv_to_v(built, name):
    with _pair(name, 18) as p:
        p.settle()
        p.be.average_uv_to_v()
        p.model.V = [(u + v) / 2 for u, v in zip(p.model.U, p.model.V)]
        p.init_constr("constraint values of (U, (U + V) / 2)")
        p.sweep("sweep behind the average")


def _front(mdl, R, lam, rho):
    mdl.set_r_state(R, lam)
    lag = mdl.cal_grad(rho)
    mdl.direction(0)
    p1, p2 = mdl.q12p12()
    coef, mags = mdl.linesearch_coeffs(rho)
    return dict(p1=p1, p2=p2, a=coef[0], b=coef[1], c=coef[2], d=coef[3], D=[x.copy() for x in mdl.D], q1=mdl.q1.copy(), q2=mdl.q2.copy(),
                lag0=lag, mags=dict(p1=mdl.p1_mag, p2=mdl.p2_mag, a=mags[0], b=mags[1], c=mags[2], d=mags[3]))


@pytest.mark.parametrize("state", ["loaded", "as_left"])
@pytest.mark.parametrize("name", ["densea65", "denseac200"])
def test_phase_one_front_behind_a_sweep(built, name, state):
    """After a sweep the kept products belong to the U array, and phase 1 writes its direction D into that array: q1 = 2 A(sym(R D^T))
    and q2 = A(D D^T) must come from D, not from the products of the U that stood there.  `loaded`: R and lambda set through set_mat /
    set_vec (load_r_state); set_mat drops the products of its cone whichever array it writes, so this order never met stale ones.
    `as_left`: no set_mat in between -- R and lambda are read from the device and the model starts from them; the direction
    itself (lorads_hip_lbfgs_direction) has to drop the products."""
    rho = 0.7
    with _pair(name, 18) as p:
        p.settle()
        be = p.be
        if state == "loaded":
            R, lam = common.random_r_state(p.s, 5, 0.1)
            common.load_r_state(be, R, lam)
            assert p.kept() == "", p.kept()
        else:
            R, lam = [be.get_mat(host.MAT_R, k) for k in range(p.nb)], be.get_vec(host.VEC_LAMBDA)
            assert all(np.all(np.isfinite(r)) and np.abs(r).max() > 0 for r in R)
            be.init_constr(host.PAIR_RR)
            assert p.kept() == "U", p.kept()
        want = _front(AlmModel.from_file(p.file), R, lam, rho)
        e64 = max(record_errors(_front(AlmModel.from_file(p.file, dtype=np.float64), R, lam, rho), want).values())
        bound = min(max(BOUND_FACTOR * e64, BOUND_FLOOR), BOUND_CEILING)
        got = dict(lag0=be.alm_cal_grad(rho))
        be.lbfgs_direction(0)
        got["D"] = [be.get_mat(host.MAT_U, k) for k in range(p.nb)]
        p1, p2 = be.alm_q12p12()
        coef = be.alm_linesearch_coeffs(rho, p1, p2)
        got.update(p1=p1, p2=p2, a=coef[0], b=coef[1], c=coef[2], d=coef[3], q1=be.get_vec(host.VEC_Q1), q2=be.get_vec(host.VEC_Q2))
        err = record_errors(got, want)
        print(name, state, "e64 %.1e" % e64, "bound %.1e" % bound, {k: "%.1e" % v for k, v in err.items()})
        assert max(err.values()) <= bound, (name, state, err, bound)
