"""Balanced partitions on the GPU (Session.round_bisection) against the numpy model (tests/bisect_model.py): the hyperplanes, the
imbalance, the signs of every trial after the repair and the swap search, f before and after the search, the best trials and the
rounds -- exactly on the unit-weight instances --, the invariants on every instance, the same bits from the dense and the sparse
store, from the LDS and the slab path and from call to call, the dual bound, the read-only continuation, the refusals and the
command line's --bisectTrials / --bisectFile.  The long-row cases (tests/bisect_cases.py): row lists longer than the workgroup in
either store of C, signed dyadic weights, t = 2 and a sum row with a != 1, exactly the model's on seeded factors."""
import os
import subprocess
import time

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.bisection import read_bisection
from tests import bisect_cases as bc
from tests import bisect_model as bm
from tests import common
from tests import rounding_model as rm

pytestmark = pytest.mark.gpu

L = 1000

# name -> (generator, environment at the context's creation).  C is stored dense above 0.1 n (n + 1) / 2 entries: s24, d40, odd65,
# dense40 and the clique pairs have a dense C; n300, w150, sparse64 and nodense64 a sparse one.
INST = {
    "s24": (lambda: instances.bisection(24, 80, 241), {}),                       # the sum row in the sparse structures (n < 32)
    "d40": (lambda: instances.bisection(40, 160, 401, diff=4), {}),              # the dense store
    "odd65": (lambda: instances.bisection(65, 300, 651, diff=1), {}),            # odd n
    "n300": (lambda: instances.bisection(300, 1200, 3001), {}),                  # several rows per thread, sparse C
    "dense40": (lambda: instances.bisection(40, 600, 402), {}),                  # a dense graph: dense C and dense sum row
    "full40": (lambda: instances.bisection(40, 160, 403, diff=40), {}),          # one side empty
    "near40": (lambda: instances.bisection(40, 160, 404, diff=38), {}),          # one side nearly empty
    "two": (lambda: instances.block_diag([instances.bisection(24, 80, 241), instances.bisection(40, 160, 401, diff=4)]), {}),
    "nodense40": (lambda: instances.bisection(40, 160, 401, diff=4), {"LORADS_NO_DENSE_A": "1"}),  # the sparse structures at n >= 32
    "nodense64": (lambda: instances.bisection(64, 100, 641), {"LORADS_NO_DENSE_A": "1"}),  # ... under a sparse C: every slot touched
    "sparse64": (lambda: instances.bisection(64, 100, 641), {}),                 # sparse C, dense store, the smallest such n
    "w150": (lambda: instances.bisection(150, 400, 1501, weights=lambda rng, k: rng.uniform(0.5, 2.0, k)), {}),  # inexact arithmetic
    "clq12": (lambda: instances.clique_pair(12, 121), {}),
    "clq16": (lambda: instances.clique_pair(16, 161), {}),
}
UNIT = [n for n in INST if n != "w150"]


def _path(name):
    if name in bc.LONG:
        return common.generated_instance("bis_long_" + name, bc.LONG[name][0])
    return common.generated_instance("bis_" + name.replace("nodense", "d"), INST[name][0]) if name in INST else (
        common.instance_path(name) if name in ("maxcut100", "theta30", "sdplp40", "blk4x60") else common.generated_instance(name))


def _phase2(path, env=None, steps=3):
    s = common.hip_session_with_env(path, env or {}, {})
    s.alm()
    s.alm_to_admm()
    s.be.init_constr(host.PAIR_UV)
    s.be.cal_obj(host.PAIR_UV)
    e0 = s.be.update_dimacs(host.PAIR_UV)
    res = s.results()
    rho = min(res["admm_rho"] if res["admm_rho"] > 0 else res["alm_rho"], 5000.0)
    if steps:
        s.admm_steps(steps, rho, e0)
    return s, rho, e0


_STATES = {}


def _state(name):
    """(session, model problem, R per cone) after phase 1 and three ADMM steps, kept for the module"""
    if name not in _STATES:
        s, _, _ = _phase2(_path(name), (INST.get(name) or bc.LONG[name])[1])
        P = bm.BisectProblem.read(_path(name))
        assert P.ok, P.why
        if name in UNIT or name in bc.LONG:
            assert s.results()["scale_obj_his"] == 1.0
        _STATES[name] = (s, P, [c.R for c in s.solution(tol=0).cones])
    return _STATES[name]


def teardown_module(module):
    for s, *_ in _STATES.values():
        s.close()
    _STATES.clear()


def _trial_signs(s, P, K):
    """every trial's signs of the last call, per cone n x K"""
    allt = np.stack([s.be.bisect_trial(t) for t in range(K)], axis=1)
    off = np.concatenate([[0], np.cumsum(P.dims)])
    return [allt[off[k]:off[k + 1]] for k in range(len(P.dims))]


def _model(P, R, r, K, rounds=L):
    """the model on the device's R and hyperplanes: per cone and trial bm.run's dict; `near`: trials with a projection
    |R_p.g| <= 1e-12 |R_p| |g|"""
    out, near = [], np.zeros(K, dtype=bool)
    for k, c in enumerate(r.cones):
        assert c.G.shape == (R[k].shape[1], K) == (c.rank, K)
        sig, proj = rm.signs(R[k], c.G)
        near |= np.any(np.abs(proj) <= 1e-12 * np.linalg.norm(R[k], axis=1)[:, None] * np.linalg.norm(c.G, axis=0)[None, :], axis=0)
        out.append([bm.run(P.C[k], P.t[k], P.d[k], sig[:, t], rounds) for t in range(K)])
    return out, near


@pytest.mark.parametrize("K", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("name", UNIT)
def test_exact_agreement_with_the_model(name, K):
    s, P, R = _state(name)
    seed = 1000 + K
    r = s.round_bisection(trials=K, seed=seed, local_search_rounds=L, tol=0, hyperplanes=True)
    for k, c in enumerate(r.cones):
        want = rm.hyperplanes(seed, k, c.rank, K)
        assert np.all(np.abs(c.G - want) <= 1e-14 * np.maximum(1.0, np.abs(want))), np.abs(c.G - want).max()
        assert c.t == P.t[k] and c.diff == P.d[k] and c.n == P.dims[k]
        assert {c.plus, c.minus} == {(c.n + c.diff) // 2, (c.n - c.diff) // 2}
    M, near = _model(P, R, r, K)
    keep = ~near
    print("%s K=%d: %d trials with a near-zero projection excluded" % (name, K, int(near.sum())))
    assert int(near.sum()) * 64 <= K
    got = _trial_signs(s, P, K)
    for k, c in enumerate(r.cones):
        assert np.array_equal(c.imbalance[keep], np.array([m["imbalance"] for m in M[k]])[keep])
        want = np.stack([m["sigma"] for m in M[k]], axis=1)
        bad = [t for t in range(K) if keep[t] and not np.array_equal(got[k][:, t], want[:, t])]
        assert not bad, (k, bad[:8])
    f0 = np.sum([[m["f0"] for m in Mk] for Mk in M], axis=0)
    f = np.sum([[m["f"] for m in Mk] for Mk in M], axis=0)
    assert np.array_equal(r.obj0[keep], f0[keep]), np.abs(r.obj0 - f0).max()
    assert np.array_equal(r.obj[keep], f[keep]), np.abs(r.obj - f).max()
    assert r.best == int(np.argmin(r.obj)) and r.best0 == int(np.argmin(r.obj0))
    assert r.f_best == r.obj[r.best] and r.f_best0 == r.obj0[r.best0]
    assert np.array_equal(r.sign, np.concatenate([g[:, r.best] for g in got]))
    if keep.all():
        assert r.best == int(np.argmin(f)) and r.best0 == int(np.argmin(f0))
        assert r.rounds == max(m["rounds"] for Mk in M for m in Mk)
        assert r.rounds < L


@pytest.mark.parametrize("name", list(INST))
def test_invariants(name):
    s, P, R = _state(name)
    K = 64
    r = s.round_bisection(trials=K, seed=7, local_search_rounds=L, tol=0)
    got = _trial_signs(s, P, K)
    for k, c in enumerate(r.cones):
        assert np.all(np.abs(got[k].sum(axis=0)) == P.d[k]), (k, got[k].sum(axis=0))
        assert np.all(np.abs(got[k]) == 1)
    assert np.all(r.obj <= r.obj0 + 1e-13 * np.maximum(1.0, np.abs(r.obj0)))
    f = sum(bm.objective(P.C[k], P.t[k], c.sigma) for k, c in enumerate(r.cones))
    assert abs(f - r.f_best) <= 1e-13 * max(1.0, abs(f)), (f, r.f_best)
    assert r.rounds >= 1
    if r.rounds < L:
        for k in range(len(r.cones)):
            tv = bm.tau(P.C[k], P.t[k])
            for t in range(K):
                pick = bm.swap_round(P.C[k], P.t[k], got[k][:, t].astype(np.int64))
                assert pick is None or pick[2] >= -1.01 * 2.0 ** -40 * (tv[pick[0]] + tv[pick[1]]), (k, t, pick)
    # no search: obj is obj0, and the repair alone balances
    r0 = s.round_bisection(trials=K, seed=7, local_search_rounds=0, tol=0)
    assert r0.rounds == 0 and np.array_equal(r0.obj, r0.obj0) and np.array_equal(r0.obj0, r.obj0) and r0.best == r0.best0
    for k, g in enumerate(_trial_signs(s, P, K)):
        assert np.all(np.abs(g.sum(axis=0)) == P.d[k])


def test_the_repair_runs():
    """at least one tested trial starts off its target"""
    for name in ("s24", "d40", "n300", "full40"):
        s, P, R = _state(name)
        r = s.round_bisection(trials=64, seed=7, local_search_rounds=0, tol=0)
        D = r.cones[0].imbalance
        target = np.where(D >= 0, P.d[0], -P.d[0])
        print("%s: %d of 64 trials repaired, largest |D - target| %d" % (name, int(np.sum(D != target)), int(np.abs(D - target).max())))
        assert np.any(D != target)


def test_long_searches_rebuild_the_field_and_match_the_model():
    """a seeded factor far from a solution: trials that accept more than 64 swaps (h is rebuilt from the row lists on the way) and a
    search cut short by max_rounds, both exactly the model's"""
    path = common.generated_instance("bis_long600", lambda: instances.bisection(600, 2400, 6001))
    P = bm.BisectProblem.read(path)
    s = common.hip_session(path)
    try:
        assert s.results()["scale_obj_his"] == 1.0
        n, r = s.block_shape(0)
        R = np.random.default_rng(9).standard_normal((n, r)) / np.sqrt(r)
        s.be.set_mat(host.MAT_R, 0, R)
        for rounds in (L, 70):
            rc, o = s.be.round_bisect(host.PAIR_RR, 8, 5, rounds, want_hyperplanes=True)
            assert rc == 0
            sig, proj = rm.signs(R, o["hyperplanes"][0])
            assert np.all(np.abs(proj) > 1e-12 * np.linalg.norm(R, axis=1)[:, None] * np.linalg.norm(o["hyperplanes"][0], axis=0)[None, :])
            M = [bm.run(P.C[0], P.t[0], P.d[0], sig[:, t], rounds) for t in range(8)]
            got = np.stack([s.be.bisect_trial(t) for t in range(8)], axis=1)
            print("n = 600, seeded factor, max_rounds %d: rounds per trial %s" % (rounds, [m["rounds"] for m in M]))
            assert min(m["rounds"] for m in M) > 66 if rounds == L else all(m["rounds"] == 70 for m in M)  # (the test's own inputs)
            assert np.array_equal(got, np.stack([m["sigma"] for m in M], axis=1))
            assert np.array_equal(o["obj"], [m["f"] for m in M]) and np.array_equal(o["obj0"], [m["f0"] for m in M])
            assert o["rounds"] == max(m["rounds"] for m in M)
            assert np.all(o["obj"] < o["obj0"])
    finally:
        s.close()


_PROBLEMS = {}


def _long_context(name, env=None):
    """a fresh context of bc.LONG[name] (`env` on top of its own), no solve: (session, model problem, (n, rank) per cone).  Its
    size facts are asserted from the rules restated here: C is stored dense where its nc stored entries exceed 0.1 n (n + 1) / 2;
    the sum row sits in the dense store from n = 32 up unless LORADS_NO_DENSE_A is set; the union pattern holds the diagonal (the
    diagonal rows) and what is not stored dense -- C's positions, every position under the sum row --; the dense stores pad n to
    a multiple of 64 (read from the dense plan the context reports); the longest row list bis_row deals outgrows the workgroup."""
    if name not in _PROBLEMS:
        _PROBLEMS[name] = bm.BisectProblem.read(_path(name))
    P = _PROBLEMS[name]
    assert P.ok and bc.c64_is_integral(P), P.why
    own = bc.LONG[name][1]
    s = common.hip_session_with_env(_path(name), dict(own, **(env or {})), {})
    try:
        assert s.results()["scale_obj_his"] == 1.0
        shapes = [s.block_shape(k) for k in range(s.nblk)]
        assert shapes == [(n, bc.RANKS[n]) for n in P.dims]
        longest = 0
        for k, C_ in enumerate(P.C):
            n, im = len(C_), s.hip_block_image(k)
            nc = int(np.count_nonzero(np.tril(C_)))
            sparse_row = n < 32 or "LORADS_NO_DENSE_A" in own
            assert im["n"] == n and im["nc"] == nc
            assert bool(im["dense_c"]) == (nc > 0.1 * n * (n + 1) / 2)
            assert im["dense_a"] == (0 if sparse_row else 1)
            held = np.ones((n, n), dtype=bool) if sparse_row else np.eye(n, dtype=bool) | ((C_ != 0) & (not im["dense_c"]))
            assert im["pattern_union"] == np.count_nonzero(np.tril(held))
            assert s.hip_dense_plan(k)["npad"] == ((n + 63) // 64 * 64 if im["dense_c"] or im["dense_a"] else 0)
            longest = max(longest, int(bc.row_lists(C_, bool(im["dense_c"]), sparse_row).max()))
        assert longest == 300 > bc.TPB
        if name == "densec300":
            assert s.hip_block_image(0)["dense_c"] == 1 and s.hip_dense_plan(0)["npad"] == 320 != P.dims[0]
        else:
            assert s.hip_block_image(0)["dense_c"] == 0
    except BaseException:
        s.close()
        raise
    return s, P, shapes


def _against_the_model(s, P, R, seed, rounds):
    """one call of bc.K trials on the factors R (set already) against the model fed the device's hyperplanes, no trial excluded
    (model_trials asserts that no projection is near zero): t and d, the imbalance, every trial's signs, obj0 and obj bit for bit,
    best, best0 and rounds.  Returns (the call's dict, the model's (dict, log) per cone and trial)."""
    rc, o = s.be.round_bisect(host.PAIR_RR, bc.K, seed, rounds, want_hyperplanes=True)
    assert rc == 0
    assert list(o["t"]) == P.t and list(o["diff"]) == P.d
    M = bc.model_trials(P, R, o["hyperplanes"], rounds)
    got = _trial_signs(s, P, bc.K)
    for k in range(len(P.dims)):
        assert np.array_equal(o["imbalance"][k], [m["imbalance"] for m, _ in M[k]]), k
        want = np.stack([m["sigma"] for m, _ in M[k]], axis=1)
        bad = [t for t in range(bc.K) if not np.array_equal(got[k][:, t], want[:, t])]
        assert not bad, (k, bad)
    f0 = np.sum([[m["f0"] for m, _ in Mk] for Mk in M], axis=0)
    f = np.sum([[m["f"] for m, _ in Mk] for Mk in M], axis=0)
    assert np.array_equal(o["obj0"], f0), (o["obj0"], f0)
    assert np.array_equal(o["obj"], f), (o["obj"], f)
    assert o["best"] == int(np.argmin(f)) and o["best0"] == int(np.argmin(f0))
    assert o["rounds"] == max(m["rounds"] for Mk in M for m, _ in Mk)
    assert np.array_equal(o["sign"], np.concatenate([g[:, o["best"]] for g in got]))
    return o, M


@pytest.mark.parametrize("name", list(bc.LONG))
def test_long_rows_weights_and_scaled_rows_match_the_model_exactly(name):
    """Row lists of 300 slots -- a second trip of bis_row's stride over the adjacency or over a row of Cfull, with a remainder --,
    signed dyadic weights, t = 2 and a = -3.  The premise of tests/bisect_cases.py makes every sum exact (C * 64 is integral, t in
    {1, 2}, n <= 300), so the comparison is bit for bit whatever the order of summation.  Seeded factors, no solve; the full search
    and a search cut short at 5 rounds.  On the hub graphs the model's log shows the hub as a swap's p and as a swap's q."""
    t0 = time.perf_counter()
    s, P, shapes = _long_context(name)
    try:
        R = bc.case_factors(name, P, shapes)
        for k, Rk in enumerate(R):
            s.be.set_mat(host.MAT_R, k, Rk)
        for rounds in (L, 5):
            o, M = _against_the_model(s, P, R, bc.SEEDS[name], rounds)
            per = [m["rounds"] for m, _ in M[0]]
            print("%s, max_rounds %d: rounds per trial %s" % (name, rounds, per) +
                  (", the hub a swap's (p, q) in %s trials" % (bc.hub_roles(M[0]),) if name.startswith("hub") else ""))
            if rounds == L:   # (the test's own inputs)
                assert 20 < o["rounds"] < L
                if name.startswith("hub"):
                    p, q = bc.hub_roles(M[0])
                    assert p >= 1 and q >= 1
            else:
                assert o["rounds"] == 5 and sum(r == 5 for r in per) >= 4
    finally:
        s.close()
    print("%s: %.2f s" % (name, time.perf_counter() - t0))


def test_the_repair_flips_the_hub_from_either_side():
    """hubneg300 with factors whose rows are all equal: every trial starts from D = +-n, the hub's Delta = -4 t^2 sum_q C_hq = -598
    is the least, so the first of the 149 flips of every trial is the hub -- bis_flip over a list of 300 slots -- and the other 148
    update h_hub through their own short lists"""
    t0 = time.perf_counter()
    s, P, shapes = _long_context("hubneg300")
    try:
        R = bc.planted(bc.PLANT, shapes)
        s.be.set_mat(host.MAT_R, 0, R[0])
        for rounds in (L, 0):
            o, M = _against_the_model(s, P, R, bc.PLANT, rounds)
            D = [m["imbalance"] for m, _ in M[0]]
            print("planted hubneg300, max_rounds %d: D %s, rounds %s" % (rounds, D, [m["rounds"] for m, _ in M[0]]))
            assert set(D) == {300, -300} and np.array_equal(o["imbalance"][0], D)
            for m, log in M[0]:
                flips = [e for e in log if e[0] == "flip"]
                assert len(flips) == 149 and flips[0][1] == bc.HUB and flips[0][2] == -598.0
    finally:
        s.close()
    print("planted hubneg300: %.2f s" % (time.perf_counter() - t0))


@pytest.mark.parametrize("name", ["hubneg300", "densec300", "mixed"])
def test_long_rows_same_bits_on_the_slab_path(name):
    """LORADS_BISECT_LDS=0: h on the slab at hs + blockIdx.x * n with n above the workgroup's 256 threads, the sign bytes in the
    trial's place of the store; against the LDS context that the exact test pins to the model, same factors and seed"""
    t0 = time.perf_counter()
    runs = []
    for env in ({}, {"LORADS_BISECT_LDS": "0"}):
        s, P, shapes = _long_context(name, env)
        try:
            assert shapes[0][0] > bc.TPB
            for k, Rk in enumerate(bc.case_factors(name, P, shapes)):
                s.be.set_mat(host.MAT_R, k, Rk)
            rc, o = s.be.round_bisect(host.PAIR_RR, bc.K, bc.SEEDS[name], L, want_hyperplanes=True)
            assert rc == 0
            runs.append((o, np.stack([s.be.bisect_trial(t) for t in range(bc.K)], axis=1)))
        finally:
            s.close()
    (a, sa), (b, sb) = runs
    for key in ("obj", "obj0", "best", "best0", "sign", "imbalance", "rounds", "t", "diff"):
        assert np.array_equal(a[key], b[key]), key
    assert all(np.array_equal(x, y) for x, y in zip(a["hyperplanes"], b["hyperplanes"]))
    assert np.array_equal(sa, sb) and a["rounds"] > 20 and np.all(a["obj"] < a["obj0"])
    print("%s, slab against LDS: %.2f s" % (name, time.perf_counter() - t0))


def _raw(s, K, seed, rounds=L):
    rc, o = s.be.round_bisect(host.PAIR_RR, K, seed, rounds)
    assert rc == 0
    return o, np.stack([s.be.bisect_trial(t) for t in range(K)], axis=1)


@pytest.mark.parametrize("name,env", [("d40", {"LORADS_NO_DENSE_A": "1"}), ("d40", {"LORADS_BISECT_LDS": "0"}),
                                      ("w150", {"LORADS_BISECT_LDS": "0"}), ("n300", {"LORADS_BISECT_LDS": "0"}),
                                      ("two", {"LORADS_BISECT_LDS": "0"})])
def test_same_bits_from_either_store_and_either_state_path(name, env):
    """the same factor in a context that keeps the sum row in the sparse structures / a trial's state in device memory"""
    s, P, R = _state(name)
    K = 64
    a = s.round_bisection(trials=K, seed=21, local_search_rounds=L, tol=0)
    sa = np.concatenate(_trial_signs(s, P, K), axis=0)
    s2 = common.hip_session_with_env(_path(name), env, {})
    try:
        for k, Rk in enumerate(R):
            s2.be.set_mat(host.MAT_R, k, Rk)
        o, sb = _raw(s2, K, 21)
    finally:
        s2.close()
    scale = s.results()["scale_obj_his"]
    assert np.array_equal(o["obj"] / scale, a.obj) and np.array_equal(o["obj0"] / scale, a.obj0)
    assert np.array_equal(sa, sb) and o["rounds"] == a.rounds and o["best"] == a.best and o["best0"] == a.best0
    assert np.array_equal(o["imbalance"], np.stack([c.imbalance for c in a.cones]))


def test_determinism_and_trial_independence():
    s, P, R = _state("two")
    a = s.round_bisection(trials=200, seed=77, local_search_rounds=L, tol=0, hyperplanes=True)
    sa = _trial_signs(s, P, 200)
    b = s.round_bisection(trials=200, seed=77, local_search_rounds=L, tol=0, hyperplanes=True)
    sb = _trial_signs(s, P, 200)
    assert np.array_equal(a.obj, b.obj) and np.array_equal(a.obj0, b.obj0) and a.best == b.best and a.rounds == b.rounds
    assert np.array_equal(a.sign, b.sign) and all(np.array_equal(x, y) for x, y in zip(sa, sb))
    c = s.round_bisection(trials=64, seed=77, local_search_rounds=L, tol=0, hyperplanes=True)
    sc = _trial_signs(s, P, 64)
    for k in range(2):
        assert np.array_equal(c.cones[k].G, a.cones[k].G[:, :64]) and np.array_equal(sc[k], sa[k][:, :64])
        assert np.array_equal(c.cones[k].imbalance, a.cones[k].imbalance[:64])
    assert np.array_equal(c.obj, a.obj[:64]) and np.array_equal(c.obj0, a.obj0[:64])
    d = s.round_bisection(trials=64, seed=78, local_search_rounds=0, tol=0, hyperplanes=True)
    assert not np.array_equal(d.cones[0].G, c.cones[0].G)


@pytest.mark.parametrize("name", ["d40", "two", "mixed"])
def test_dual_bound(name):
    """mixed: T_k = n_k t_k^2 is 1200 for the first cone (t = 2) and 24 for the second"""
    s, P, R = _state(name)
    if name == "mixed":
        assert [P.T(k) for k in range(2)] == [1200.0, 24.0]
    r = s.round_bisection(trials=64, seed=1, local_search_rounds=10, tol=1e-8)
    sol = s.solution(tol=1e-8)
    lam = []
    for k, c in enumerate(sol.cones):
        row, col, val = sol.slack(k)
        S = np.zeros((c.n, c.n))
        S[row, col] = val
        S[col, row] = val
        lam.append(float(np.linalg.eigvalsh(S)[0]))
    d = rm.dual_bound(P.b, sol.y, [P.T(k) for k in range(len(P.dims))], lam)
    assert abs(r.bound - d) <= 1e-8 * max(1.0, abs(d)), (r.bound, d)
    assert abs(r.by - float(P.b @ sol.y)) <= 1e-12 * max(1.0, abs(r.by))
    assert r.bound <= r.f_best
    assert r.gap == pytest.approx((r.f_best - r.bound) / max(1.0, abs(r.bound)), rel=1e-15)


def test_whole_solve_proves_the_bisection_of_a_clique_pair_optimal():
    s = common.hip_session(_path("clq16"))
    try:
        s.solve()
        r = s.round_bisection(tol=1e-8)
    finally:
        s.close()
    print("clique_pair(16): f_best %.17g (after the repair %.17g), dual bound %.17g, rounds %d" % (r.f_best, r.f_best0, r.bound, r.rounds))
    assert r.f_best == 16.0
    assert r.bound > 15 and int(np.ceil(r.bound)) == 16
    assert r.cones[0].plus == r.cones[0].minus == 16


def _snap(s):
    nb = s.nblk
    return [s.be.get_mat(w, k) for w in (host.MAT_U, host.MAT_V) for k in range(nb)] + [s.be.get_vec(host.VEC_LAMBDA)]


@pytest.mark.parametrize("name", ["s24", "d40"])
def test_read_only_continuation(name):
    runs = []
    for rnd in (True, False):
        s, rho, e0 = _phase2(_path(name), steps=0)
        try:
            a = s.admm_steps(5, rho, e0)
            if rnd:
                s.round_bisection(trials=200, seed=3, local_search_rounds=L, tol=1e-8)
            b = s.admm_steps(5, rho, a[0])
            runs.append((a, b, _snap(s)))
        finally:
            s.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for x, y in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(x, y)


def _deviating(n, e, seed, diff=0):
    prob = instances.bisection(n, e, seed, diff=diff)
    ent = list(prob["entries"])
    i = max(j for j, x in enumerate(ent) if x[0] == n + 1 and x[2] != x[3]) - 7
    ent[i] = ent[i][:4] + (1.0 + 2.0 ** -52,)
    return dict(prob, entries=ent)


def _two_sum_rows(n):
    prob = instances.bisection(n, 3 * n, 5)
    return dict(prob, m=n + 2, b=np.append(prob["b"], 0.0), entries=prob["entries"] + [(n + 2,) + e[1:] for e in prob["entries"] if e[0] == n + 1])


def _with_b(n, b_last):
    prob = instances.bisection(n, 3 * n, 6)
    b = prob["b"].copy()
    b[-1] = b_last
    return dict(prob, b=b)


REFUSED = {
    "maxcut100": (None, "cone 1 has no sum row"),
    "bis_dev24": (lambda: _deviating(24, 80, 241), "constraint 25 is neither a diagonal row nor a sum row of cone 1"),
    "bis_dev40": (lambda: _deviating(40, 160, 401, 4), "constraint 41 is neither a diagonal row nor a sum row of cone 1"),
    "bis_two24": (lambda: _two_sum_rows(24), r"cone 1 has two sum rows \(constraints 25 and 26\)"),
    "bis_two40": (lambda: _two_sum_rows(40), r"cone 1 has two sum rows \(constraints 41 and 42\)"),
    "bis_q3": (lambda: _with_b(24, 3.0), r"the sum row of cone 1 \(constraint 25\) has b / \(a t\^2\) = 3:"),
    "bis_q3d": (lambda: _with_b(40, 3.0), r"the sum row of cone 1 \(constraint 41\) has b / \(a t\^2\) = 3:"),
    "bis_odd_d": (lambda: _with_b(24, 1.0), r"the sum row of cone 1 \(constraint 25\) has b / \(a t\^2\) = 1: .* n = 24 with d = n \(mod 2\)"),
    "bis_scaled": (lambda: instances._with_sum_row(instances.scaled_pm1(40, 100, 3), 0), "cone 1 has unequal diagonal values"),
    "sdplp40": (None, "block 2 is an LP block"),
    "theta30": (None, "constraint 1 is neither a diagonal row nor a sum row of cone 1"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(name):
    make, why = REFUSED[name]
    path = common.generated_instance(name, make) if make else common.instance_path(name)
    s = common.hip_session(path)
    try:
        assert s.be.round_bisect(host.PAIR_RR, 0)[0] == 2 and s.be.round_bisect(host.PAIR_RR, 8)[0] == 2
        with pytest.raises(NotImplementedError, match="not bisection-structured: " + why):
            s.round_bisection(trials=0)
        with pytest.raises(NotImplementedError, match="not bisection-structured"):
            s.round_bisection(trials=8)
    finally:
        s.close()


def test_bad_arguments_leave_the_context_usable():
    s, P, R = _state("s24")
    for args in ((host.PAIR_RR, -1), (host.PAIR_RR, 65537), (7, 8), (host.PAIR_RR, 8, 0, -1)):
        assert s.be.round_bisect(*args)[0] == 1
    rc, o = s.be.round_bisect(host.PAIR_UV, 0)
    assert rc == 0 and o["t"][0] == 1.0 and o["diff"][0] == 0
    assert s.round_bisection(trials=0) is None
    assert s.round_bisection(trials=8, tol=0).trials == 8


def test_sharded_refusal():
    s = common.hip_session(common.instance_path("blk4x60"), world=2, rank=0, separable=True)
    try:
        assert s.be.round_bisect(host.PAIR_RR, 0)[0] == 3
        with pytest.raises(NotImplementedError, match="sharded"):
            s.round_bisection(trials=16)
    finally:
        s.close()


@pytest.mark.parametrize("name", ["s24", "d40", "nodense40"])
def test_the_other_roundings_still_refuse(name):
    s, P, R = _state(name)
    with pytest.raises(NotImplementedError, match="not \\+-1-structured"):
        s.round_pm1(trials=0)
    with pytest.raises(NotImplementedError):
        s.round_kcut(3, trials=0)
    with pytest.raises(NotImplementedError):
        s.triangle_cuts()
    assert s.be.round_kcut(host.PAIR_UV, 3, 0)[0] == 2
    assert s.be.triangle_cuts(host.PAIR_UV, 0, 1e-3, 10)[0] == 2


def test_cli(tmp_path):
    exe = os.path.join(host.LIB_DIR, "lorads")
    path = _path("clq12")
    out = tmp_path / "bisect.txt"
    p = subprocess.run([exe, path, "--bisectTrials", "64", "--bisectFile", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert "Bisection (64 trials, seed 0, %s): parts 12+12, best f" % out in p.stdout and "dual bound d" in p.stdout, p.stdout
    s = common.hip_session(path)
    try:
        s.solve()
        s.write_bisection(tmp_path / "py.txt", trials=64)
        mine = s.round_bisection(trials=64)
    finally:
        s.close()
    assert (tmp_path / "py.txt").read_bytes() == out.read_bytes()
    got = read_bisection(out)
    assert got.best == mine.best and got.f_best == mine.f_best == 12.0 and got.bound == mine.bound
    assert np.array_equal(got.sign, mine.sign) and np.array_equal(got.obj, mine.obj) and np.array_equal(got.obj0, mine.obj0)
    bad = subprocess.run([exe, common.instance_path("maxcut100"), "--bisectTrials", "8"], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 2 and "End Program" not in bad.stdout and "bisection-structured" in bad.stderr
