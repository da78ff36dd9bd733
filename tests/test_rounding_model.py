"""The rounding's numpy model against first principles, and the rounding file written by the C writer (lrd_rounding_write) read
back bit for bit (no GPU)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.rounding import RoundingConeStruct, RoundingStruct, read_rounding
from tests import rounding_model as rm


@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEFCAFEF00D, (1 << 64) - 1])
def test_generator_matches_big_integer_splitmix(seed):
    rng = np.random.default_rng(seed % 1000)
    for cone, rank, K in ((0, 7, 70), (3, 40, 9), (15, 512, 3)):
        G = rm.hyperplanes(seed, cone, rank, K)
        for t, j in zip(rng.integers(0, K, 12), rng.integers(0, rank, 12)):
            assert G[j, t] == rm.hyperplane_int(seed, cone, int(t), int(j)), (cone, t, j)
    # one splitmix64 step from a known state (the generator's published first outputs for state 0)
    assert rm.sm_int(0) == 0xE220A8397B1DCDAF
    assert int(rm.sm(np.uint64(0))) == 0xE220A8397B1DCDAF
    # trial t's hyperplane does not depend on K; other seeds and cones give other values
    assert np.array_equal(rm.hyperplanes(seed, 2, 5, 64), rm.hyperplanes(seed, 2, 5, 1024)[:, :64])
    assert not np.array_equal(rm.hyperplanes(seed, 2, 5, 8), rm.hyperplanes(seed ^ 1, 2, 5, 8))
    assert not np.array_equal(rm.hyperplanes(seed, 2, 5, 8), rm.hyperplanes(seed, 3, 5, 8))


def _random_problem(rng, n, unit):
    """single cone, +-1 structure with random a, b (b / a > 0) and C with a diagonal"""
    C_ = np.zeros((n, n))
    for p, q in itertools.combinations(range(n), 2):
        if rng.random() < 0.5:
            C_[p, q] = C_[q, p] = (rng.integers(-2, 3) / 4.0) if unit else rng.uniform(-1, 1)
    C_[np.diag_indices(n)] = rng.uniform(-1, 1, n)
    s = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    a = np.ones(n) if unit else s * rng.uniform(0.5, 2, n)
    b = np.ones(n) if unit else s * rng.uniform(0.5, 2, n)
    ent = [(0, 1, p + 1, q + 1, -C_[p, q]) for p in range(n) for q in range(p, n) if C_[p, q] != 0]
    ent += [(i + 1, 1, i + 1, i + 1, a[i]) for i in range(n)]
    return rm.Pm1Problem(n, b, [n], ent), a


@pytest.mark.parametrize("seed", range(12))
def test_objective_and_local_search_on_small_instances(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 13))
    P, _ = _random_problem(rng, n, unit=seed % 2 == 0)
    assert P.ok
    C_, t = P.C[0], P.t[0]
    R = rng.standard_normal((n, 3))
    sigma, _ = rm.signs(R, rm.hyperplanes(seed, 0, 3, 40))
    f0 = rm.objective(C_, t, sigma)
    for k in range(sigma.shape[1]):
        x = sigma[:, k] * t
        assert abs(f0[k] - x @ C_ @ x) <= 1e-12 * max(1.0, abs(f0[k]))
    s1, rounds = rm.local_search(C_, t, P.adj[0], sigma, 100)
    f1 = rm.objective(C_, t, s1)
    assert np.all(f1 <= f0 + 1e-12 * np.maximum(1.0, np.abs(f0)))
    assert 1 <= rounds < 100
    d, tau = rm.deltas(C_, t, s1)
    assert np.all(d >= -tau[:, None])  # 1-opt up to tau
    # no two vertices of a colour class are adjacent
    col = rm.colouring(P.adj[0])
    for p in range(n):
        assert all(col[q] != col[p] for q in P.adj[0][p])
        assert all(col[p] == 0 or any(col[q] == c for q in P.adj[0][p] if q < p) for c in range(col[p]))
    # brute force: the best +-1 point is 1-opt, and every local-search result is no better than it
    allx = np.array(list(itertools.product([-1, 1], repeat=n)), dtype=np.int8).T
    fall = rm.objective(C_, t, allx)
    assert f1.min() >= fall.min() - 1e-12 * max(1.0, abs(fall.min()))


@pytest.mark.parametrize("seed", range(8))
def test_dual_bound_below_the_pm1_optimum(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(2, 11))
    P, a = _random_problem(rng, n, unit=False)
    C_, t = P.C[0], P.t[0]
    allx = np.array(list(itertools.product([-1, 1], repeat=n)), dtype=np.int8).T
    fmin = rm.objective(C_, t, allx).min()
    for _ in range(5):
        y = rng.standard_normal(n) * 2
        S = C_ - np.diag(y * a)  # S = C - sum_i y_i A_i, A_i = a_i e_p e_p^T
        d = rm.dual_bound(P.b, y, [P.T(0)], [np.linalg.eigvalsh(S)[0]])
        assert d <= fmin + 1e-10 * max(1.0, abs(fmin))


def test_near_misses_do_not_qualify():
    for prob in (instances.maxcut_uncovered(30, 50, 1), instances.maxcut_negative_ratio(30, 50, 2)):
        assert not rm.Pm1Problem(prob["m"], prob["b"], prob["blocks"], prob["entries"]).ok
    for prob in (instances.maxcut(30, 50, 3), instances.scaled_pm1(30, 60, 4), instances.weighted_maxcut(30, 60, 5),
                 instances.dense_maxcut(40, 300, 6)):
        assert rm.Pm1Problem(prob["m"], prob["b"], prob["blocks"], prob["entries"]).ok


def _ptr(a, ct=C.c_double):
    return a.ctypes.data_as(C.POINTER(ct))


@pytest.mark.parametrize("dims", [[5], [6, 3, 9], [1]])
def test_roundtrip_bit_equal(tmp_path, dims):
    rng = np.random.default_rng(len(dims))
    keep = []
    arr = (RoundingConeStruct * len(dims))()
    sig_want = []
    for k, n in enumerate(dims):
        s = np.where(rng.random(n) < 0.5, -1, 1).astype(np.int8)
        keep.append(s)
        arr[k].n, arr[k].rank = n, 3
        arr[k].sigma = _ptr(s, C.c_int8)
        sig_want.append(s)
    st = RoundingStruct()
    h = st.head   # (the scalars sit in the struct's lrd_round_head)
    st.nblk, h.trials, h.max_rounds, h.rounds, h.src = len(dims), 1000, 100, 7, 1
    h.seed, h.best, h.best0 = (1 << 64) - 5, 917, 3
    vals = dict(scale=5.0, f_best=-123.45678901234567, f_best0=1e-310, by=1.0 / 3.0, bound=float("nan"), gap=2.5e-17, tol=1e-8)
    for k, v in vals.items():
        setattr(h, k, v)
    st.cone = arr
    lib = host.host_lib()
    lib.lrd_rounding_write.argtypes = [C.c_char_p, C.POINTER(RoundingStruct)]
    path = tmp_path / "r.txt"
    assert lib.lrd_rounding_write(str(path).encode(), C.byref(st)) == 0
    got = read_rounding(path)
    assert path.read_text().startswith("lorads-rounding 1\n")
    for k in ("trials", "seed", "max_rounds", "rounds", "src", "best", "best0"):
        assert getattr(got, k) == getattr(h, k), k
    for k, v in vals.items():
        g = getattr(got, k)
        assert (np.isnan(g) and np.isnan(v)) or np.float64(g).tobytes() == np.float64(v).tobytes(), k
    assert len(got.cones) == len(dims)
    for c, s in zip(got.cones, sig_want):
        assert np.array_equal(c.sigma, s)
    assert np.array_equal(got.sign, np.concatenate(sig_want))
