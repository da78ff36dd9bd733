"""The numpy model of the stable-set rounding (tests/stable_model.py) against first principles -- the greedy sets, the swap search,
brute-force alpha, the parallel fixed point -- the structure check on the generators and on what write_bounded makes of them, and the
stable-set file (lrd_stable_write against read_stable, byte for byte).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.stable import StableCone, StableSet, StableStruct, read_stable
from tests import common
from tests import stable_model as sm
from tests.test_bounds_model import _bounds


def _random_adj(rng, n, n_edges):
    nb = [set() for _ in range(n)]
    for _ in range(n_edges):
        p, q = rng.choice(n, 2, replace=False).tolist() if n > 1 else (0, 0)
        if p != q:
            nb[p].add(q)
            nb[q].add(p)
    return [np.array(sorted(x), dtype=np.int64) for x in nb]


def _path_adj(n):
    return [np.array([q for q in (p - 1, p + 1) if 0 <= q < n], dtype=np.int64) for p in range(n)]


def _problem(name):
    prob = {"c5": lambda: _cycle_theta(5), "theta30x100": lambda: instances.theta(30, 100, 1),
            "hamming5_2": lambda: instances.hamming_theta(5, 2)}[name]()
    return sm.StableProblem(prob["m"], prob["b"], prob["blocks"], prob["entries"])


def _cycle_theta(n):
    ent = [(0, 1, i + 1, j + 1, 1.0) for i in range(n) for j in range(i, n)]
    ent += [(1, 1, i + 1, i + 1, 1.0) for i in range(n)]
    for k in range(n):
        i, j = sorted((k, (k + 1) % n))
        ent.append((k + 2, 1, i + 1, j + 1, 1.0))
    b = np.zeros(n + 1)
    b[0] = 1.0
    return dict(m=n + 1, blocks=[n], b=b, entries=ent)


@pytest.mark.parametrize("n,e", [(1, 0), (2, 1), (17, 30), (40, 60), (40, 300), (64, 0)])
def test_greedy_sets_are_stable_and_maximal_and_swaps_never_shrink(n, e):
    rng = np.random.default_rng(n * 1000 + e)
    adj = _random_adj(rng, n, e)
    for trial in range(8):
        pi = rng.standard_normal(n) if trial else np.round(rng.standard_normal(n))   # (trial 0: many exact ties)
        S0 = sm.greedy(adj, pi)
        assert sm.is_stable(adj, S0) and sm.is_maximal(adj, S0)
        first = sm.order(pi)[0]
        assert S0[first]
        prev = S0
        for L in range(1, 6):
            S, r = sm.swap_search(adj, pi, S0, L)
            assert sm.is_stable(adj, S) and sm.is_maximal(adj, S)
            assert S.sum() >= prev.sum() and 1 <= r <= L
            assert S.sum() >= S0.sum() + r - 1   # (every round but the last one that finds nothing adds a vertex or more)
            prev = S
        S, r = sm.swap_search(adj, pi, S0, 1000)
        assert r < 1000 and S.sum() <= sm.alpha(adj)
        assert sm.swap_search(adj, pi, S, 5)[1] == 1   # (a fixed point of the search: the next search stops in its first round)


def _max_stable(adj):
    """a maximum stable set by exhaustive branching (a witness of alpha)"""
    n = len(adj)
    best = [np.zeros(n, dtype=bool)]

    def rec(p, S, blocked):
        if p == n:
            if S.sum() > best[0].sum():
                best[0] = S.copy()
            return
        if S.sum() + (n - p) <= best[0].sum():
            return
        if not blocked[p]:
            S[p] = True
            b2 = blocked.copy()
            b2[adj[p]] = True
            rec(p + 1, S, b2)
            S[p] = False
        rec(p + 1, S, blocked)

    rec(0, np.zeros(n, dtype=bool), np.zeros(n, dtype=bool))
    return best[0]


@pytest.mark.parametrize("name,want", [("c5", 2), ("theta30x100", None), ("hamming5_2", 4)])
def test_model_reaches_alpha_from_an_exact_feasible_point(name, want):
    """X = X(S*) = T 1 1^T / |S*| on a maximum stable set S* is feasible and of rank one; its factor's trial-0 priorities X_pp put S*
    first, so the greedy set is S* and the search leaves it alone"""
    P = _problem(name)
    assert P.ok, P.why
    adj, T = P.adj[0], P.T[0]
    a = sm.alpha(adj)
    if want is not None:
        assert a == want
    star = _max_stable(adj)
    assert star.sum() == a and sm.is_stable(adj, star)
    F = (np.sqrt(T / a) * star.astype(np.float64))[:, None]
    G = sm.directions(0, 0, 1, 4)
    pi = sm.priorities(F, G)
    S0, S1, r = sm.run_trial(adj, pi[:, 0], 100)
    assert np.array_equal(S0, star) and np.array_equal(S1, star) and r == 1
    f, mag = sm.value(P.C[0], T, S1)
    assert float(f) == -float(a) and mag == float(a)   # (C = -J: f = -|S|)
    for t in range(1, 4):   # (the projections are +- the same indicator: every trial's set is stable, maximal and at most alpha)
        S0, S1, _ = sm.run_trial(adj, pi[:, t], 100)
        assert sm.is_stable(adj, S1) and sm.is_maximal(adj, S1) and S0.sum() <= S1.sum() <= a


@pytest.mark.parametrize("n,e", [(1, 0), (9, 12), (33, 40), (60, 200), (100, 150)])
def test_fixed_point_is_the_sequential_greedy(n, e):
    rng = np.random.default_rng(7 * n + e)
    adj = _random_adj(rng, n, e)
    for trial in range(6):
        pi = rng.standard_normal(n) if trial else np.round(2 * rng.standard_normal(n))
        S, rounds = sm.fixed_point(adj, pi)
        assert np.array_equal(S, sm.greedy(adj, pi)) and rounds <= n + 1


def test_fixed_point_on_a_path_takes_half_as_many_rounds_as_vertices():
    n = 60
    adj = _path_adj(n)
    pi = (n - np.arange(n)).astype(np.float64)
    S, rounds = sm.fixed_point(adj, pi)
    assert np.array_equal(S, np.arange(n) % 2 == 0) and np.array_equal(S, sm.greedy(adj, pi)) and rounds == n // 2


def _check_prob(prob):
    return sm.StableProblem(prob["m"], prob["b"], prob["blocks"], prob["entries"])


def test_structure_check_accepts():
    for prob in (instances.theta(30, 40, 1), instances.theta(50, 103, 1), instances.hamming_theta(5, 2), _cycle_theta(5)):
        P = _check_prob(prob)
        assert P.ok and P.T[0] == 1.0 and len(P.edges[0]) == prob["m"] - 1
    P = _check_prob(instances.block_diag([instances.theta(30, 40, 1), _cycle_theta(5), instances.theta(17, 20, 3)]))
    assert P.ok and P.cones == [0, 1, 2] and [len(P.edges[k]) for k in P.cones] == [40, 5, 20]


def test_structure_check_accepts_what_write_bounded_writes(tmp_path):
    path = common.instance_path("theta30")
    out = str(tmp_path / "bounded.dat-s")
    s = host.Session.open(path, lib=common.load_oracle())
    try:
        s.write_bounded(out, _bounds([(0, 0, 5, 0, 0.0), (0, 2, 29, 0, 0.0), (0, 3, 4, 1, 0.25)]))
    finally:
        s.close()
    P = sm.StableProblem.read(out)
    assert P.ok, P.why
    assert P.lp == [1] and len(P.rows) == 3 and len(P.edges[0]) == 40
    # 2 (1/2) X_pq -+ x_j = bound with T = 1: u = 1/2 + |bound|
    assert np.array_equal(P.u, [0.5, 0.5, 0.75])


@pytest.mark.parametrize("name,why", [("maxcut100", "constraint 1 is neither a trace row nor an edge row of cone 1"),
                                      ("sdplp40", "constraint 1 has 3 LP entries"),
                                      ("rand120", "neither a trace row nor an edge row")])
def test_structure_check_rejects_goldens(name, why):
    P = sm.StableProblem.read(common.instance_path(name))
    assert not P.ok and why in P.why, P.why


def test_structure_check_rejects_broken_thetas():
    prob = instances.theta(30, 40, 1)
    b = prob["b"].copy()
    b[7] = 0.5
    P = _check_prob(dict(prob, b=b))
    assert P.why == "constraint 8 is an edge row with b = 0.5 (not 0)"
    two = dict(prob, m=prob["m"] + 1, b=np.append(prob["b"], 2.0), entries=prob["entries"] + [(prob["m"] + 1, 1, i + 1, i + 1, 2.0) for i in range(30)])
    assert _check_prob(two).why == "cone 1 has two trace rows (constraints 1 and 42)"
    none = dict(prob, m=prob["m"] - 1, b=prob["b"][1:], entries=[(e[0] - (e[0] > 0), ) + tuple(e[1:]) for e in prob["entries"] if e[0] != 1])
    assert _check_prob(none).why == "cone 1 has no trace row"
    neg = dict(prob, b=-prob["b"])
    assert _check_prob(neg).why.startswith("constraint 1 is a trace row with a = 1, b = -1")


def test_priorities_and_their_bound():
    rng = np.random.default_rng(3)
    F = rng.standard_normal((13, 5))
    G = sm.directions(11, 2, 5, 7)
    pi = sm.priorities(F, G)
    assert np.allclose(pi[:, 0].astype(np.float64), (F * F).sum(axis=1)) and np.allclose(pi[:, 1:].astype(np.float64), (F @ G)[:, 1:])
    B = sm.priority_bound(F, G)
    assert B.shape == pi.shape and np.all(B > 0)
    assert np.all(np.abs((F @ G)[:, 1:] - pi[:, 1:]) <= B[:, 1:])


def test_value_and_lp_bounds():
    C = np.array([[1.0, -2.0, 0.0], [-2.0, 3.0, 0.5], [0.0, 0.5, -1.0]])
    S = np.array([True, False, True])
    f, mag = sm.value(C, 4.0, S)
    assert float(f) == 2.0 * (1.0 - 1.0) and mag == 2.0 * 2.0
    assert sm.f_bound(C, 4.0, S, 1) == (2 + 1 + 8 + 4 + 1) * 2.0 ** -53 * 4.0
    assert sm.dual_bound([1.0, 0.0], [-3.0, 9.0], [2.0], [-0.25], [0.5], [-1.0]) == -3.0 - 0.5 - 0.5


def _stable_set():
    cones = [StableCone(0, 7, 3, np.array([0, 2, 6])), StableCone(2, 1, 1, np.array([0])), StableCone(3, 4, 2, np.zeros(0, dtype=np.int64))]
    return StableSet(cones, trials=5, seed=2 ** 63 + 11, max_rounds=100, rounds=3, src=1, best=4, best0=0, lp_columns=2, lp_negative=1,
                     scale=0.1, f_best=-3.0000000000000004, f_best0=-2.0, by=-3.3333333333333335, bound=-3.4, gap=1.0 / 3.0, tol=1e-8)


def test_stable_file_round_trips_byte_for_byte(tmp_path):
    """lrd_stable_write is a pure function of the struct: written from a struct built here, read back, written again"""
    lib = host.host_lib()
    lib.lrd_stable_write.argtypes = [C.c_char_p, C.POINTER(StableStruct)]
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    x = _stable_set()
    assert lib.lrd_stable_write(os.fsencode(str(a)), C.byref(x.to_struct())) == 0
    text = a.read_text().split("\n")
    assert text[0] == "lorads-stableset 1" and text[1] == "trials 5" and text[2] == "seed %d" % (2 ** 63 + 11)
    assert "f_best -3.0000000000000004" in text and "gap 0.33333333333333331" in text
    assert text[text.index("cone 1 7 3"):][:4] == ["cone 1 7 3", "1", "3", "7"] and "cone 3 1 1" in text and text[-2] == "cone 4 4 0"
    y = read_stable(str(a))
    for k in ("trials", "seed", "max_rounds", "rounds", "src", "best", "best0", "lp_columns", "lp_negative", "scale", "f_best",
              "f_best0", "by", "bound", "gap", "tol"):
        assert getattr(y, k) == getattr(x, k), k
    assert [c.blk for c in y.cones] == [0, 2, 3] and y.sizes == [3, 1, 0]
    assert all(np.array_equal(c.member, d.member) for c, d in zip(x.cones, y.cones))
    assert lib.lrd_stable_write(os.fsencode(str(b)), C.byref(y.to_struct())) == 0
    assert a.read_bytes() == b.read_bytes()
    assert lib.lrd_stable_write(os.fsencode(str(tmp_path / "no" / "dir.txt")), C.byref(x.to_struct())) == 2


def test_read_stable_refuses_malformed_files(tmp_path):
    lib = host.host_lib()
    lib.lrd_stable_write.argtypes = [C.c_char_p, C.POINTER(StableStruct)]
    a = tmp_path / "a.txt"
    assert lib.lrd_stable_write(os.fsencode(str(a)), C.byref(_stable_set().to_struct())) == 0
    good = a.read_text()
    for bad in (good.replace("lorads-stableset 1", "lorads-kcut 1"), good.replace("cone 1 7 3\n1\n3\n7", "cone 1 7 3\n3\n1\n7"),
                good.replace("cone 1 7 3\n1\n3\n7", "cone 1 7 3\n1\n3\n8"), good.replace("rounds 3\n", "")):
        p = tmp_path / "bad.txt"
        p.write_text(bad)
        with pytest.raises(ValueError):
            read_stable(str(p))


def test_oracle_backend_has_no_slot_and_the_table_mirror_places_it():
    s = common.oracle_session(common.instance_path("theta30"))
    try:
        assert not s.be.has_round_stable()
        with pytest.raises(NotImplementedError):
            s.round_stable(trials=8)
    finally:
        s.close()
    names = [f[0] for f in host.BackendStruct._fields_]
    assert names.index("get_slack") + 1 == names.index("round_stable") == names.index("round_pm1") - 1
    lib = host.host_lib()
    lib.lrd_backend_sizeof.restype = C.c_size_t
    assert lib.lrd_backend_sizeof() == C.sizeof(host.BackendStruct)
    hdr = open(os.path.join(common.ROOT, "include", "lorads_hip.h")).read()
    assert "int lorads_hip_round_stable(lorads_hip_ctx *ctx, int32_t src, int32_t trials, uint64_t seed, int32_t max_rounds" in hdr
