"""The model of the rounding into k parts (tests/kcut_model.py) against definitions written out a second time -- big-integer generator,
dense X(l), brute force -- and the parts of the feature that need no GPU: the planted partitions of the complete k-partite graphs,
weak duality of the bound with and without bound rows, the file writer, the table's slot and the refusals of the host and the command
line."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.kcut import KCut, KCutCone, KCutStruct, read_kcut
from tests import bounds_model as bm
from tests import common
from tests import kcut_model as km
from tests import rounding_model as rm


def test_vectors_against_hyperplanes_and_big_integers():
    G = km.vectors(12345, 3, 5, 7, 40)
    assert np.array_equal(G[0], rm.hyperplanes(12345, 3, 7, 40))
    for a, t, j in [(1, 0, 0), (4, 39, 6), (2, 17, 3), (3, 1, 5)]:
        assert G[a, j, t] == km.vector_int(12345, 3, a, t, j)
    for seed in (0, (1 << 64) - 1):
        g = km.vectors(seed, 2, 64, 1, 1)
        assert g[63, 0, 0] == km.vector_int(seed, 2, 63, 0, 0)
    # the counter's fields do not collide at their largest values
    top = km.counter(5, 63, 65535, 1023)
    assert top == (5 << 32) | (63 << 26) | (65535 << 10) | 1023
    assert (top >> 32, (top >> 26) & 63, (top >> 10) & 65535, top & 1023) == (5, 63, 65535, 1023)
    assert len({km.counter(c, a, t, j) for c in (0, 1) for a in (0, 1, 63) for t in (0, 1, 65535) for j in (0, 1, 1023)}) == 54


def _random_problem(rng, n):
    C_ = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.5)
    C_ = np.triu(C_) + np.triu(C_, 1).T
    return C_, 0.5 + rng.random(n)


@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 5, 12])
def test_objective_against_dense_point(n, k):
    rng = np.random.default_rng(10 * n + k)
    C_, t = _random_problem(rng, n)
    lab = rng.integers(0, k, size=(n, 30)).astype(np.uint8)
    f = km.objective(C_, t, lab, k)
    for i in range(lab.shape[1]):
        X = km.point(t, lab[:, i], k)
        want = float(np.sum(C_ * X))
        assert abs(float(f[i]) - want) <= 1e-13 * max(1.0, np.sum(np.abs(C_) * np.outer(t, t)))
        assert np.allclose(np.diag(X), t * t, rtol=1e-15)
        assert np.linalg.eigvalsh(X)[0] >= -1e-12 * float(t @ t)
    if k == 2:   # the +-1 rounding's x^T C x at sigma = +-1
        sig = np.where(lab == 0, 1, -1).astype(np.int8)
        want = rm.objective(C_, t, sig)
        assert np.all(np.abs(f.astype(np.float64) - want) <= 1e-13 * max(1.0, np.sum(np.abs(C_) * np.outer(t, t))))


@pytest.mark.parametrize("k", [2, 3, 4])
def test_brute_force_minimum_and_local_search(k):
    """n = 7: the search never rises, every accepted move lowers f by |Delta|, it ends 1-move-optimal up to tau, and no trial ends
    below the brute-force minimum"""
    rng = np.random.default_rng(k)
    n = 7
    C_, t = _random_problem(rng, n)
    allab = np.array(list(itertools.product(range(k), repeat=n)), dtype=np.uint8).T
    fmin = float(km.objective(C_, t, allab, k).min())
    adj = [np.nonzero((C_[p] != 0) & (np.arange(n) != p))[0] for p in range(n)]
    lab0 = rng.integers(0, k, size=(n, 50)).astype(np.uint8)
    # one move at a time: f drops by |Delta|
    for tr in range(10):
        lab = lab0[:, tr:tr + 1].copy()
        for _ in range(100):
            rec = []
            f0 = float(km.objective(C_, t, lab, k)[0])
            nxt, _, _ = km.local_search(C_, t, adj, lab, k, 1, record=rec)
            if not rec:
                break
            f1 = float(km.objective(C_, t, nxt, k)[0])
            assert abs((f1 - f0) - sum(d for _, _, d in rec)) <= 1e-12 * max(1.0, abs(f0))
            assert all(d < 0 for _, _, d in rec) and f1 < f0
            lab = nxt
    lab1, rounds, _ = km.local_search(C_, t, adj, lab0, k, 100)
    f0, f1 = km.objective(C_, t, lab0, k), km.objective(C_, t, lab1, k)
    assert 1 <= rounds < 100 and np.all(f1 <= f0) and float(f1.min()) >= fmin - 1e-12
    d, tau = km.move_deltas(C_, t, lab1, k)
    assert np.all(d >= -1.01 * tau[:, None] - 1e-300)


@pytest.mark.parametrize("name,k,m,fstar,need", [("kpartite3x10", 3, 10, -75.0, 64), ("kpartite4x6", 4, 6, -36.0, 60)])
def test_planted_partition(name, k, m, fstar, need):
    """R = the simplex arrangement plus 1e-2 Gaussian noise at rank 8: the rounding and the search find the planted partition"""
    P = km.KCutProblem(*_prob(instances.NAMED[name]()))
    assert P.ok and P.cones == [0]
    n = k * m
    W4 = P.C[0] - np.diag(np.diag(P.C[0]))     # C = -L/4 = (W - D) / 4: the off-diagonal part is W/4
    assert W4.sum() == k * (k - 1) * m * m / 4.0
    rng = np.random.default_rng(7)
    V = np.zeros((k, 8))
    V[:, :k] = np.eye(k) - 1.0 / k
    V /= np.linalg.norm(V, axis=1)[:, None]
    R = V[np.arange(n) // m] + 1e-2 * rng.standard_normal((n, 8))
    lab, _ = km.labels(R, km.vectors(0, 0, k, 8, 64))
    adj = P.adj[0]
    lab1, _, _ = km.local_search(W4, P.t[0], adj, lab, k, 100)
    f = km.objective(W4, P.t[0], lab1, k).astype(np.float64)
    planted = (np.arange(n) // m).astype(np.uint8)[:, None]
    assert float(km.objective(W4, P.t[0], planted, k)[0]) == fstar
    hits = int(np.sum(f == fstar))
    print("%s: %d of 64 trials end at f(planted) = %g" % (name, hits, fstar))
    assert hits >= need and np.all(f >= fstar)
    # in the problem's own terms (C = -L/4): f = -E k / (2 (k - 1)) and the cut weight is -2 f (k - 1) / k = E
    E = k * (k - 1) * m * m // 2
    fp = float(km.objective(P.C[0], P.t[0], planted, k)[0])
    assert fp == -E * k / (2.0 * (k - 1)) and -2 * fp * (k - 1) / k == E


def _prob(prob):
    return prob["m"], prob["b"], prob["blocks"], prob["entries"]


@pytest.mark.parametrize("bounded", [False, True])
def test_dual_bound_is_below_every_feasible_point(tmp_path, bounded):
    """weak duality written out: for any y, d(y) <= <C, X> for every feasible (X, x) -- sampled ones, every X(l) that meets the
    bound rows (brute force, n = 8, k = 3) -- and so <= the optimum, which the oracle's solve approaches from its tolerance"""
    k, n = 3, 8
    prob = instances.maxcut(n, 14, 5)
    cuts = [(0, 0, 3, 0, -0.5), (0, 1, 2, 0, -0.5), (0, 2, 7, 0, -0.625), (0, 4, 5, 0, -0.75)] if bounded else []
    if bounded:
        prob = bm.bounded(prob, cuts)
    path = str(tmp_path / "p.dat-s")
    instances.write_sdpa(prob, path)
    P = km.KCutProblem.read(path)
    assert P.ok and len(P.rows) == len(cuts)
    Cm, t = P.C[0], P.t[0]
    assert np.array_equal(t, np.ones(n))
    if bounded:
        assert np.array_equal(P.u, [(abs(c[4]) + 1.0) / 1.0 for c in cuts])
    rng = np.random.default_rng(3)
    allab = np.array(list(itertools.product(range(k), repeat=n)), dtype=np.uint8).T
    fall = km.objective(Cm, t, allab, k).astype(np.float64)
    # feasible points: X(l) (x_j = X_pq - lower >= 0 holds as lower <= -1/2) and random correlation matrices that meet the rows
    feas = []
    for i in rng.choice(allab.shape[1], 40, replace=False):
        feas.append(km.point(t, allab[:, i], k))
    while len(feas) < 80:
        F = rng.standard_normal((n, 3))
        X = F @ F.T
        dd = np.sqrt(np.diag(X))
        X = X / np.outer(dd, dd) * 0.4 + 0.6 * np.eye(n)
        if all(X[p, q] >= lo for _, p, q, _, lo in cuts):
            feas.append(X)
    s_o = common.oracle_session(path, phase2Tol=1e-5)
    try:
        popt = s_o.solve()["pObj"]
    finally:
        s_o.close()
    assert popt <= fall.min() + 1e-6
    for trial in range(6):
        y = np.zeros(P.m) if trial == 0 else rng.standard_normal(P.m) * (0.1 if trial < 3 else 1.0)
        if trial == 5:   # a good y: the degrees (S = the Laplacian's off-diagonal part shifted), zero on the bound rows
            y[:n] = -np.abs(np.diag(Cm)) - 0.3
            y[n:] = 0.0
        S = Cm - np.diag(y[:n])
        s = np.zeros(len(cuts))
        for i, kk, p, q, a, j, c in P.rows:
            S[p, q] -= y[i] * a
            S[q, p] -= y[i] * a
            s[j] = -c * y[i]
        d = km.dual_bound(P.b, y, [P.T(0)], [float(np.linalg.eigvalsh(S)[0])], P.u if bounded else (), s)
        for X in feas:
            x = np.array([(P.b[i] - 2 * a * X[p, q]) / c for i, kk, p, q, a, j, c in P.rows])
            assert np.all(x >= -1e-15) and np.all(x <= (P.u if bounded else x) + 1e-15)
            val = float(np.sum(Cm * X))
            # the identity <C, X> = b.y + <S, X> + s.x at a feasible point, and the bound below it
            assert abs(val - (float(P.b @ y) + float(np.sum(S * X)) + float(s @ x))) <= 1e-11 * (1 + np.abs(y).sum())
            assert d <= val + 1e-11 * (1 + np.abs(y).sum())
        assert d <= fall.min() + 1e-11 * (1 + np.abs(y).sum())
        assert d <= popt + 1e-3 * (1 + abs(popt))


def _example():
    rng = np.random.default_rng(1)
    cones = []
    for blk, n in ((0, 5), (2, 3)):
        lab = rng.integers(0, 3, n).astype(np.uint8)
        cones.append(KCutCone(blk, n, 4, lab, np.bincount(lab, minlength=3)))
    return KCut(cones, parts=3, trials=64, seed=(1 << 64) - 5, max_rounds=100, rounds=4, src=1, best=17, best0=3, lp_columns=7,
                lp_negative=2, scale=0.125, f_best=-1.0 / 3.0, f_best0=-0.3, by=-0.4, bound=-0.41, gap=0.07666666666666666, tol=1e-8)


def test_writer_round_trip(tmp_path):
    lib = host.host_lib()
    lib.lrd_kcut_write.argtypes = [C.c_char_p, C.POINTER(KCutStruct)]
    r = _example()
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    assert lib.lrd_kcut_write(os.fsencode(a), C.byref(r.to_struct())) == 0
    back = read_kcut(a)
    for key in ("parts", "trials", "seed", "max_rounds", "rounds", "src", "best", "best0", "lp_columns", "lp_negative", "scale", "f_best",
                "f_best0", "by", "bound", "gap", "tol"):
        assert getattr(back, key) == getattr(r, key), key
    assert [c.blk for c in back.cones] == [0, 2] and np.array_equal(back.label, r.label)
    assert all(np.array_equal(x.sizes, y.sizes) for x, y in zip(back.cones, r.cones))
    back.cones[0].rank = back.cones[1].rank = 4
    assert lib.lrd_kcut_write(os.fsencode(b), C.byref(back.to_struct())) == 0
    assert open(a, "rb").read() == open(b, "rb").read()
    assert open(a).readline() == "lorads-kcut 1\n"
    with pytest.raises(ValueError):
        read_kcut(common.instance_path("maxcut100"))
    assert lib.lrd_kcut_write(os.fsencode(str(tmp_path / "no" / "dir.txt")), C.byref(r.to_struct())) == 2


def test_oracle_backend_refuses_and_table_mirror():
    s = common.oracle_session(common.instance_path("maxcut100"))
    try:
        assert not s.be.has_round_kcut()
        with pytest.raises(NotImplementedError):
            s.round_kcut(3, trials=0)
        with pytest.raises(NotImplementedError):
            s.round_kcut(3, trials=16)
    finally:
        s.close()
    names = [f[0] for f in host.BackendStruct._fields_]
    assert names.index("round_pm1") + 1 == names.index("round_kcut") == names.index("primal_entries") - 1
    lib = host.host_lib()
    lib.lrd_backend_sizeof.restype = C.c_size_t
    assert lib.lrd_backend_sizeof() == C.sizeof(host.BackendStruct)
    assert C.sizeof(KCutStruct) == 136
    hip = C.CDLL(os.path.join(host.LIB_DIR, "liblorads_hip.so"))
    assert hasattr(hip, "lorads_hip_round_kcut")


@pytest.mark.parametrize("name,why", [("maxcut100", None), ("theta30", "entries"), ("maxcut_uncovered60", "diagonal 60 of cone 1 is fixed by 0"),
                                      ("maxcut_negratio60", "constraint 1 has b / a = -1"), ("sdplp40", "constraint 1 has"),
                                      ("mix4", "entries")])
def test_model_check(name, why):
    golden = {"maxcut100", "theta30", "sdplp40", "mix4"}
    P = km.KCutProblem.read(common.instance_path(name) if name in golden else common.generated_instance(name))
    if why is None:
        assert P.ok and P.why is None
    else:
        assert not P.ok and why in P.why, P.why


@pytest.mark.parametrize("args", [["--kcutParts", "1"], ["--kcutParts", "65"], ["--kcutParts", "-3"], ["--kcutParts", "3x"],
                                  ["--kcutParts", "3", "--kcutTrials", "0"], ["--kcutParts", "3", "--kcutTrials", "65537"],
                                  ["--kcutParts", "64", "--kcutTrials", "16385"], ["--kcutParts", "3", "--kcutSeed", "-1"],
                                  ["--kcutParts", "3", "--kcutLocalSearch", "-2"], ["--kcutParts", "3", "--kcutLocalSearch", "1e3"],
                                  ["--kcutTrials", "64"], ["--kcutSeed", "1"], ["--kcutLocalSearch", "10"], ["--kcutFile", "out.txt"]])
def test_cli_refuses_bad_values_before_the_backend(tmp_path, args):
    host.host_lib()
    exe = os.path.join(host.LIB_DIR, "lorads")
    # (no GPU and no HIP library in reach: whatever passes the options would fail with another code and message)
    r = subprocess.run([exe, common.instance_path("maxcut100")] + args, cwd=tmp_path, capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "bad value" in r.stderr or "needs --kcutParts" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.txt")
