"""Stable sets read off the factors on the GPU (lorads_hip_round_stable, Session.round_stable) against the numpy model
(tests/stable_model.py): the priorities within their derived bound, then -- the model fed the device's own priorities -- exactly the
device's sets, sizes, best trials and rounds for every trial, f within its derived bound; the shapes and graphs that reach each edge of
the kernels on seeded factors; read-only continuation, memory, refusals, and real solves end to end (C5, the Hamming graph's theta',
the theta30 golden, the command line)."""
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.stable import read_stable
from tests import common
from tests import stable_model as sm
from tests.test_rounding import _phase2, _snap
from tests.test_stable_model import _cycle_theta
from tests.test_triangle_cuts import _last_error, _mem

pytestmark = pytest.mark.gpu

RR, UV = host.PAIR_RR, host.PAIR_UV


def _graph_problem(cones, seed, dense_c=False):
    """cones: [(n, edges)], one trace row 2 tr(X_k) = 3 (T = 1.5) and one edge row per edge; C random symmetric, a diagonal and about
    2 n off-diagonal entries (dense_c: every entry, so that the solver stores C dense)"""
    rng = np.random.default_rng(seed)
    ent, con, b = [], 0, []
    for k, (n, edges) in enumerate(cones):
        if dense_c:
            cpos = [(i, j) for i in range(n) for j in range(i, n)]
        else:
            cpos = [(i, i) for i in range(n)] + [tuple(sorted(rng.choice(n, 2, replace=False).tolist())) for _ in range(2 * n if n > 1 else 0)]
        for i, j in sorted(set(cpos)):
            ent.append((0, k + 1, i + 1, j + 1, float(np.round(rng.standard_normal() * 64) / 64 or 0.25)))
    for k, (n, edges) in enumerate(cones):
        con += 1
        b.append(3.0)
        ent += [(con, k + 1, i + 1, i + 1, 2.0) for i in range(n)]
        for p, q in edges:
            con += 1
            b.append(0.0)
            ent.append((con, k + 1, min(p, q) + 1, max(p, q) + 1, 1.0))
    ent.sort(key=lambda e: (e[0], e[1]))
    return dict(m=con, blocks=[n for n, _ in cones], b=np.array(b), entries=ent)


def _random_edges(rng, n, count):
    out = set()
    while len(out) < min(count, n * (n - 1) // 2):
        p, q = sorted(rng.choice(n, 2, replace=False).tolist())
        out.add((p, q))
    return sorted(out)


def _named(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("rand"):     # rand<n>
        n = int(name[4:])
        return [(n, _random_edges(rng, n, 2 * n) if n > 1 else [])]
    if name == "c5":
        return [(5, [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4)])]
    if name == "empty33":
        return [(33, [])]
    if name == "complete33":
        return [(33, [(p, q) for p in range(33) for q in range(p + 1, 33)])]
    if name == "star301":           # the hub (vertex 7) has 300 neighbours: more than a workgroup has threads
        return [(301, [(min(7, q), max(7, q)) for q in range(301) if q != 7])]
    if name == "cliques35":
        return [(35, [(5 * c + i, 5 * c + j) for c in range(7) for i in range(5) for j in range(i + 1, 5)])]
    if name == "path600":
        return [(600, [(p, p + 1) for p in range(599)])]
    if name == "three":             # three cones of unequal n
        return [(5, [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4)]), (33, _random_edges(rng, 33, 50)), (17, _random_edges(rng, 17, 30))]
    raise KeyError(name)


_SESS = {}


def _session(name, dense_c=False):
    """(session at device rank 1, model problem) of a named graph problem, kept for the module"""
    key = (name, dense_c)
    if key not in _SESS:
        tag = "stable_%s%s" % (name, "_dc" if dense_c else "")
        path = common.generated_instance(tag, lambda: _graph_problem(_named(name), len(tag), dense_c))
        s = common.hip_session(path, timesLogRank=1e-3)
        P = sm.StableProblem.read(path)
        assert P.ok, P.why
        _SESS[key] = (s, P)
    return _SESS[key]


def teardown_module(module):
    for s, _ in _SESS.values():
        s.close()
    _SESS.clear()


def _load(s, ranks, src, seed, factors=None):
    """seeded factors at the given ranks; returns F per cone as the device forms it"""
    if [s.block_shape(k)[1] for k in range(s.nblk)] != list(ranks):
        s.be.resize_rank(list(ranks))
    rng = np.random.default_rng(seed)
    shapes = [s.block_shape(k) for k in range(s.nblk)]
    assert [r for _, r in shapes] == list(ranks)
    if factors is not None:
        A = B = [np.asarray(f, dtype=np.float64) for f in factors]
    else:
        A = [rng.standard_normal(sh) for sh in shapes]
        B = [rng.standard_normal(sh) for sh in shapes]
    if src == RR:
        common.load_r_state(s.be, A, np.zeros(s.m))
        return A
    common.load_uv_state(s.be, A, B, np.zeros(s.m))
    return [(a + b) / 2 for a, b in zip(A, B)]


def _check(s, P, F, K, seed, L, src):
    """one call against the model: priorities, then every trial's sets, sizes and rounds, f, the best trials"""
    rc, d = s.be.round_stable(src, K, seed, L, want_scores=True)
    assert rc == 0, _last_error(s)
    ncone = len(P.cones)
    worst = 0.0
    for kc, k in enumerate(P.cones):
        G = sm.directions(seed, k, F[kc].shape[1], K)
        exact, bound = sm.priorities(F[kc], G), sm.priority_bound(F[kc], G)
        err = np.abs(d["scores"][kc] - exact).astype(np.float64)
        assert d["scores"][kc].shape == exact.shape and np.all(err <= bound), (k, float((err - bound).max()))
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.array_equal(d["T"], [P.T[k] for k in P.cones])
    rounds, fmax = 0, 0.0
    for t in range(K):
        got = s.be.stable_trial(t)
        at, f, f0, fb, fb0 = 0, np.longdouble(0), np.longdouble(0), 0.0, 0.0
        for kc, k in enumerate(P.cones):
            n = P.dims[k]
            S0, S1, r = sm.run_trial(P.adj[k], d["scores"][kc][:, t], L)
            assert np.array_equal(got[at:at + n].astype(bool), S1), (t, k)
            assert d["sizes"][kc, t] == S1.sum() and sm.is_stable(P.adj[k], S1) and sm.is_maximal(P.adj[k], S1)
            rounds = max(rounds, r)
            f += sm.value(P.C[k], P.T[k], S1)[0]
            f0 += sm.value(P.C[k], P.T[k], S0)[0]
            fb += sm.f_bound(P.C[k], P.T[k], S1, ncone)
            fb0 += sm.f_bound(P.C[k], P.T[k], S0, ncone)
            at += n
        assert abs(d["obj"][t] - f) <= fb and abs(d["obj0"][t] - f0) <= fb0, (t, float(d["obj"][t] - f), fb)
        fmax = max(fmax, float(abs(d["obj"][t] - f)) / fb if fb else 0.0)
    assert d["rounds"] == rounds
    assert d["best"] == int(np.argmin(d["obj"])) and d["best0"] == int(np.argmin(d["obj0"]))
    assert np.array_equal(d["member"], s.be.stable_trial(d["best"]))
    if L == 0:
        assert np.array_equal(d["obj"], d["obj0"]) and d["best"] == d["best0"]
    print("K=%d L=%d: rounds %d, worst score error / bound %.3f, worst f error / bound %.3f" % (K, L, rounds, worst, fmax))
    return d


# n (not a multiple of 16 or 64; more vertices than a workgroup has threads), rank, K, src: every n, every rank and every K of the
# lists below at least once, the large n at the small K
SHAPES = [(1, 1, 1, RR), (1, 3, 3, UV), (5, 2, 3, RR), (5, 130, 3, UV), (33, 3, 64, RR), (33, 18, 3, UV), (64, 16, 257, RR), (64, 41, 3, UV),
          (600, 3, 3, UV), (2100, 2, 3, RR)]


@pytest.mark.parametrize("n,r,K,src", SHAPES)
def test_shapes(n, r, K, src):
    s, P = _session("rand%d" % n)
    F = _load(s, [r], src, 100 * n + r)
    _check(s, P, F, K, seed=n + K, L=100, src=src)


@pytest.mark.parametrize("name", ["empty33", "complete33", "c5", "cliques35", "three"])
@pytest.mark.parametrize("L", [0, 1, 100])
def test_graphs(name, L):
    s, P = _session(name)
    ranks = [3] * len(P.cones)
    F = _load(s, ranks, UV, 5)
    d = _check(s, P, F, 16, seed=9, L=L, src=UV)
    if name == "empty33":
        assert np.all(d["sizes"] == 33) and d["member"].all() and d["rounds"] == min(L, 1)
    if name == "complete33":
        assert np.all(d["sizes"] == 1)
    if name == "c5":
        assert np.all(d["sizes"] == 2)
    if name == "cliques35":
        assert np.all(d["sizes"] == 7)


def test_dense_objective():
    """C stored dense: the value pass walks the full row"""
    s, P = _session("rand33", dense_c=True)
    F = _load(s, [4], RR, 8)
    _check(s, P, F, 16, seed=2, L=100, src=RR)


@pytest.mark.parametrize("L", [0, 100])
def test_star_with_a_hub_above_the_workgroup_size(L):
    """rank-1 factors that put the hub first in trial 0: the greedy set is the hub alone, and one swap with its completion takes all
    300 leaves"""
    s, P = _session("star301")
    f = np.ones((301, 1))
    f[7] = 2.0
    F = _load(s, [1], RR, 0, factors=[f])
    d = _check(s, P, F, 3, seed=1, L=L, src=RR)
    assert d["sizes"][0, 0] == (300 if L else 1) and d["rounds"] == (2 if L else 0)


def test_path_is_the_longest_dependency_chain():
    """F_p = n - p at rank 1: trial 0 decides one vertex per round of the fixed point, n / 2 rounds"""
    s, P = _session("path600")
    F = _load(s, [1], RR, 0, factors=[(600.0 - np.arange(600.0))[:, None]])
    d = _check(s, P, F, 2, seed=4, L=100, src=RR)
    assert np.array_equal(s.be.stable_trial(0), np.arange(600) % 2 == 0) and d["sizes"][0, 0] == 300


def test_duplicated_rows_tie_by_index():
    s, P = _session("rand33")
    rng = np.random.default_rng(12)
    f = np.repeat(rng.standard_normal((3, 18)), 11, axis=0)   # rows 0..10, 11..21, 22..32 equal: exact ties in every trial
    F = _load(s, [18], UV, 0, factors=[f])
    d = _check(s, P, F, 16, seed=6, L=100, src=UV)
    assert len(np.unique(d["scores"][0][:, 3])) == 3


def test_same_bits_twice_and_trial_independence():
    s, P = _session("three")
    _load(s, [3, 3, 3], UV, 5)
    a = s.be.round_stable(UV, 100, 77, 100, want_scores=True)[1]
    b = s.be.round_stable(UV, 100, 77, 100, want_scores=True)[1]
    for key in ("obj", "obj0", "member", "sizes"):
        assert np.array_equal(a[key], b[key])
    assert (a["best"], a["best0"], a["rounds"]) == (b["best"], b["best0"], b["rounds"])
    c = s.be.round_stable(UV, 17, 77, 100, want_scores=True)[1]
    assert np.array_equal(c["obj"], a["obj"][:17]) and np.array_equal(c["sizes"], a["sizes"][:, :17])
    assert all(np.array_equal(x, y[:, :17]) for x, y in zip(c["scores"], a["scores"]))


def test_read_only_and_memory():
    """lambda, U, V and the next ADMM steps are what they are without the call, a dual update waiting inside the backend stays
    waiting; the scratch grows once and goes with the context"""
    path = common.instance_path("theta30")
    held = _mem()
    runs = []
    for rnd in (True, False):
        s, rho, e0 = _phase2(path, steps=0)
        try:
            a = s.admm_steps(5, rho, e0)   # (leaves a dual update waiting inside the backend)
            if rnd:
                before = _mem()
                x = s.round_stable(trials=300, seed=3, local_search_rounds=100, tol=1e-8)
                grown = _mem()
                y = s.round_stable(trials=300, seed=3, local_search_rounds=100, tol=1e-8)
                assert _mem() == grown and grown[1] > before[1]
                assert np.array_equal(x.obj, y.obj) and np.array_equal(x.members[0], y.members[0]) and x.bound == y.bound
            b = s.admm_steps(5, rho, a[0])
            runs.append((a, b, _snap(s)))
        finally:
            s.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for x, y in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(x, y)
    assert _mem() == held


def _refused(s, code, why, call):
    snap = [s.be.get_mat(host.MAT_R, 0), s.be.get_vec(host.VEC_LAMBDA)]
    held, launches = _mem(), s.hip_launch_count()
    assert call()[0] == code
    assert why in _last_error(s), (why, _last_error(s))
    assert _mem() == held and s.hip_launch_count() == launches
    assert all(np.array_equal(x, y) for x, y in zip(snap, [s.be.get_mat(host.MAT_R, 0), s.be.get_vec(host.VEC_LAMBDA)]))


def _broken_theta(kind):
    prob = instances.theta(30, 40, 1)
    if kind == "edge_b":
        b = prob["b"].copy()
        b[7] = 0.5
        return dict(prob, b=b)
    return dict(prob, m=prob["m"] + 1, b=np.append(prob["b"], 2.0),
                entries=prob["entries"] + [(prob["m"] + 1, 1, i + 1, i + 1, 2.0) for i in range(30)])


@pytest.mark.parametrize("name", ["maxcut100", "sdplp40", "rand120", "edge_b", "two_trace"])
def test_refused_structures(name):
    if name in ("edge_b", "two_trace"):
        path = common.generated_instance("stable_theta_" + name, lambda: _broken_theta(name))
    else:
        path = common.instance_path(name)
    why = sm.StableProblem.read(path).why   # (the model walks the constraints as the library does: the same first reason, word for word)
    assert why
    s = common.hip_session(path)
    try:
        _refused(s, 2, "not theta-structured: " + why, lambda: s.be.round_stable(RR, 0))
        _refused(s, 2, "not theta-structured: " + why, lambda: s.be.round_stable(RR, 8))
    finally:
        s.close()


def test_bad_arguments_sharded_and_unsolved():
    s, P = _session("c5")
    _refused(s, 1, "trials -1 is outside [0, 65536]", lambda: s.be.round_stable(RR, -1))
    _refused(s, 1, "trials 65537 is outside [0, 65536]", lambda: s.be.round_stable(RR, 65537))
    _refused(s, 1, "bad argument", lambda: s.be.round_stable(7, 8))
    _refused(s, 1, "bad argument", lambda: s.be.round_stable(RR, 8, max_rounds=-1))
    with pytest.raises(ValueError, match="trials 65537"):
        s.round_stable(trials=65537)
    sh = common.hip_session(common.instance_path("blk4x60"), world=2, rank=0, separable=True)
    try:
        _refused(sh, 3, "sharded", lambda: sh.be.round_stable(RR, 16))
        with pytest.raises(NotImplementedError, match="sharded"):
            sh.round_stable(trials=16)
    finally:
        sh.close()
    t = common.hip_session(common.instance_path("maxcut100"))
    try:
        with pytest.raises(NotImplementedError, match="theta-structured"):
            t.round_stable(trials=0)
    finally:
        t.close()


def _stable_in(prob, S):
    P = sm.StableProblem(prob["m"], prob["b"], prob["blocks"], prob["entries"])
    mask = np.zeros(P.dims[0], dtype=bool)
    mask[S] = True
    return P, mask


def test_c5_theta_end_to_end(tmp_path):
    """every maximal stable set of the 5-cycle has 2 vertices: the size is certain, and theta = sqrt(5) bounds it from above"""
    prob = _cycle_theta(5)
    path = str(tmp_path / "c5theta.dat-s")
    instances.write_sdpa(prob, path)
    s = common.hip_session(path)
    try:
        r = s.solve()
        x = s.round_stable(trials=64, seed=0)
    finally:
        s.close()
    P, mask = _stable_in(prob, x.members[0])
    print("C5 theta: pObj %.9f, size %s, f_best %.12f, bound %.9f, gap %.3e, rounds %d" % (r["pObj"], x.sizes, x.f_best, x.bound, x.gap, x.rounds))
    assert x.sizes == [2] and sm.is_stable(P.adj[0], mask) and sm.is_maximal(P.adj[0], mask)
    assert abs(x.f_best + 2.0) <= 1e-12 and -x.bound >= 2.0 - 1e-4 and abs(-x.bound - np.sqrt(5.0)) <= 1e-3
    assert x.bound <= x.f_best and x.gap == pytest.approx((x.f_best - x.bound) / max(1.0, abs(x.bound)), rel=1e-15)


def test_hamming_theta_prime_exhibits_the_code_of_size_4(tmp_path):
    """theta' = 4 of the graph on {0,1}^5 with an edge at distance 1 or 2 (solve, entry_bounds(lower=0), write_bounded, solve), and a
    stable set of size 4 -- a binary code of length 5 and minimum distance 3 -- read off the bounded solve's factors: alpha = 4"""
    prob = instances.hamming_theta(5, 2)
    path, tight = str(tmp_path / "ham5.dat-s"), str(tmp_path / "ham5_b.dat-s")
    instances.write_sdpa(prob, path)
    s = common.hip_session(path)
    try:
        s.solve()
        x0 = s.round_stable(trials=64, seed=0)
        s.write_bounded(tight, s.entry_bounds(lower=0.0))
    finally:
        s.close()
    p2tol = 1e-4
    s2 = common.hip_session(tight, phase2Tol=p2tol)
    try:
        s2.solve()
        x = s2.round_stable(trials=64, seed=0)
    finally:
        s2.close()
    P, mask = _stable_in(prob, x.members[0])
    print("hamming theta: unbounded solve size %s (trial 0: %d), bound %.6f; bounded solve size %s (trial 0: %d), bound %.6f, "
          "lp columns %d (negative slacks %d)" % (x0.sizes, x0.cones[0].trial_sizes[0], x0.bound, x.sizes, x.cones[0].trial_sizes[0],
                                                  x.bound, x.lp_columns, x.lp_negative))
    assert sm.is_stable(P.adj[0], mask) and sm.is_maximal(P.adj[0], mask)
    assert x.sizes == [4] and abs(x.f_best + 4.0) <= 1e-12
    code = [int(v) for v in x.members[0]]
    assert all(bin(a ^ b).count("1") >= 3 for i, a in enumerate(code) for b in code[i + 1:])
    assert x.lp_columns == 16 and np.all(x.lp_upper == 0.5)
    assert abs(-x.bound - 4.0) <= 5 * p2tol * (1 + 4), x.bound


def test_theta30_golden_and_cli(tmp_path):
    """the theta30 golden: a stable, maximal set no larger than the bound allows, beside brute-force alpha; the command line writes
    the same bytes as write_stable for the same seed"""
    path = common.instance_path("theta30")
    P = sm.StableProblem.read(path)
    s = common.hip_session(path)
    try:
        s.solve()
        x = s.round_stable(trials=128, seed=0)
        s.write_stable(tmp_path / "py.txt", trials=128, seed=0, local_search_rounds=100, tol=1e-8)
    finally:
        s.close()
    mask = np.zeros(30, dtype=bool)
    mask[x.members[0]] = True
    a = sm.alpha(P.adj[0])
    print("theta30: size %d (greedy only: %d), alpha %d, bound %.6f, gap %.3e, rounds %d" % (x.sizes[0], round(-x.f_best0), a, x.bound, x.gap, x.rounds))
    assert sm.is_stable(P.adj[0], mask) and sm.is_maximal(P.adj[0], mask)
    assert x.sizes[0] <= a <= int(np.floor(-x.bound + 1e-3)) and abs(x.f_best + x.sizes[0]) <= 1e-12 * x.sizes[0]
    exe = os.path.join(host.LIB_DIR, "lorads")
    out = tmp_path / "cli.txt"
    p = subprocess.run([exe, path, "--stableTrials", "128", "--stableFile", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert "Stable sets (128 trials, seed 0, %s): size %d, best f" % (out, x.sizes[0]) in p.stdout and "dual bound d" in p.stdout, p.stdout
    assert (tmp_path / "py.txt").read_bytes() == out.read_bytes()
    got = read_stable(out)
    assert got.best == x.best and got.f_best == x.f_best and got.bound == x.bound and np.array_equal(got.members[0], x.members[0])
    bad = subprocess.run([exe, common.instance_path("maxcut100"), "--stableTrials", "8"], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 2 and "End Program" not in bad.stdout and "theta-structured" in bad.stderr
    alone = subprocess.run([exe, path, "--stableSeed", "3"], capture_output=True, text=True, timeout=600)
    assert alone.returncode == 2 and "--stableSeed needs --stableTrials" in alone.stderr
