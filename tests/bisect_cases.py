"""The long-row instances of the bisection rounding ("Long rows, weights and t != 1"), shared by
tests/test_bisect_model.py (CPU: the generator, the model on such data, the seeds), tests/test_bisection.py and
tests/test_trial_chunks.py (GPU).

Premise of every exact comparison on them: all edge weights are multiples of 1/16, so C = L / 4 holds multiples of 1/64 only
(`c64_is_integral`), t is 1 or 2 and n <= 300.  Every product and every partial sum in h, Delta, tau and f is then a multiple of
1/64 far below 2^53 / 64 in size, i.e. exact in double, whatever the order of summation: device and model must agree bit for bit."""
import numpy as np

from lorads_amd import instances
from tests import bisect_model as bm
from tests import rounding_model as rm

N = 300     # = 256 + 44: the smallest size at which a row list dealt over 256 threads takes a second trip with a remainder
HUB = 7     # the vertex adjacent to every other one
TPB = 256   # the workgroup of k_bis_search


def dyadic(rng, k):
    """k weights drawn from the nonzero j / 16, j in [-8, 32]"""
    j = rng.integers(-8, 32, k)
    return np.where(j >= 0, j + 1, j) / 16.0


def hub_graph(weighted):
    """N vertices: HUB adjacent to every other vertex, plus those of 300 seeded random edges that do not touch it.  Unit weights, or
    -1/2 on the hub's edges and dyadic weights elsewhere."""
    rng = np.random.default_rng(3007)
    e = instances._rand_edges(N, 300, rng)
    e = e[(e != HUB).all(axis=1)]
    edges = np.concatenate([np.array([(min(HUB, v), max(HUB, v)) for v in range(N) if v != HUB]), e])
    edges = edges[np.lexsort((edges[:, 1], edges[:, 0]))]
    w = np.where((edges == HUB).any(axis=1), -0.5, dyadic(rng, len(edges))) if weighted else np.ones(len(edges))
    return edges, w


def hub300():
    return instances.bisection_graph(N, *hub_graph(False), diff=2)


def hubneg300():
    """0.5 X_pp = 2 (t = 2) and -3 <11^T, X> = -12 d^2 with d = 2"""
    return instances.bisection_graph(N, *hub_graph(True), diff=2, t=2.0, a=-3.0)


def densec300():
    """6000 edges + 300 diagonal entries > 0.1 * 300 * 301 / 2 = 4515: C is stored dense (npad = 320 != n)"""
    rng = np.random.default_rng(3008)
    edges = instances._rand_edges(N, 6000, rng)
    return instances.bisection_graph(N, edges, dyadic(rng, len(edges)), diff=0, t=2.0)


def mixed():
    """hubneg300 (t = 2, d = 2, the sum row in the dense store) beside a 24-row cone with t = 1, d = 4 and its sum row in the sparse
    structures (n < 32)"""
    return instances.block_diag([hubneg300(), instances.bisection(24, 80, 243, diff=4, weights=dyadic)])


# name -> (generator, environment at the context's creation)
LONG = {
    "hub300": (hub300, {}),                 # 300 slots in the hub's row list, sparse C, dense sum row
    "hubneg300": (hubneg300, {}),           # ... with negative and non-unit weights, t = 2, a = -3
    "densec300": (densec300, {}),           # a row of Cfull past one trip, npad != n
    "nodense300": (lambda: instances.bisection(300, 1200, 3001), {"LORADS_NO_DENSE_A": "1"}),  # n300's file: every row list has 300 slots
    "mixed": (mixed, {}),                   # unlike cones: t, d, store of the sum row
}

K = 8
RANKS = {300: 12, 24: 7}   # the ranks the contexts give cones of these sizes (asserted where a context is at hand)
# name -> seed of the factors and of the call: chosen so that no projection is near zero and, on the hub graphs, the hub is a
# swap's p in some trial and a swap's q in some trial (tests/test_bisect_model.py::test_seeds_of_the_long_row_cases checks both at
# these ranks).  hubneg300 takes `near_solution` factors: under -1/2 on the hub's edges Delta_hub = 2 - 2 sigma_hub sum(sigma) is -2
# or 6 whatever the state, and from i.i.d. factors a side's least Delta is far below that while swaps are still accepted -- over 30
# graph seeds, 24 factor seeds and 8 trials each (5760 trials) the hub was a swap's q in 1194 trials and its p in none.
SEEDS = {"hub300": 7, "hubneg300": 19, "densec300": 5, "nodense300": 5, "mixed": 5}
NEAR = {"hubneg300": 0.5}
# the planted factor of hubneg300 (all rows equal, so every trial starts from D = +-n): seed of the factors and of the call
PLANT = 5


def c64_is_integral(P):
    return all(np.array_equal(C * 64.0, np.rint(C * 64.0)) for C in P.C)


def factors(seed, shapes):
    """seeded factors far from a solution, one (n, r) array per cone"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, r)) / np.sqrt(r) for n, r in shapes]


def near_solution(P, seed, eps, shapes):
    """what a solve leaves: per cone a rank-one factor on a partition that the model's search ends in (from seeded signs), plus
    eps times a seeded Gaussian factor"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (n, r) in enumerate(shapes):
        star = bm.run(P.C[k], P.t[k], P.d[k], np.where(rng.random(n) < 0.5, 1, -1), 1000)["sigma"]
        u = rng.standard_normal(r) / np.sqrt(r)
        out.append(np.outer(star, u) + eps * rng.standard_normal((n, r)) / np.sqrt(r))
    return out


def case_factors(name, P, shapes):
    """the factors of LONG[name]'s exact cases"""
    return near_solution(P, SEEDS[name], NEAR[name], shapes) if name in NEAR else factors(SEEDS[name], shapes)


def planted(seed, shapes):
    """factors whose rows are all equal: every vertex falls on the same side of every hyperplane"""
    rng = np.random.default_rng(seed)
    return [np.tile(rng.standard_normal(r) / np.sqrt(r), (n, 1)) for n, r in shapes]


def model_trials(P, R, G, rounds):
    """the model on the factors R and the hyperplanes G (per cone, rank x K): per cone and trial (bm.run's dict, its log).  No
    trial is excluded: every projection must be away from zero, |R_p.g| > 1e-12 |R_p| |g|."""
    out = []
    for k in range(len(P.dims)):
        assert G[k].shape[0] == R[k].shape[1]
        sig, proj = rm.signs(R[k], G[k])
        assert np.all(np.abs(proj) > 1e-12 * np.linalg.norm(R[k], axis=1)[:, None] * np.linalg.norm(G[k], axis=0)[None, :]), k
        cone = []
        for t in range(G[k].shape[1]):
            log = []
            cone.append((bm.run(P.C[k], P.t[k], P.d[k], sig[:, t], rounds, log), log))
        out.append(cone)
    return out


def hub_roles(trials):
    """(trials in which HUB is some swap's p, ... some swap's q) from one cone's (dict, log) pairs"""
    p = sum(any(e[0] == "swap" and e[1] == HUB for e in log) for _, log in trials)
    q = sum(any(e[0] == "swap" and e[2] == HUB for e in log) for _, log in trials)
    return p, q


def row_lists(C, dense_c, sum_row_sparse):
    """the lengths of the lists bis_row deals over the workgroup, from the rules of DESIGN.md sections 3 and 19: a dense-C cone
    walks the n positions of its row of Cfull; a sparse-C cone walks the union pattern's adjacency -- the positions C stores, the
    diagonal (the diagonal rows), and every position where the sum row sits in the sparse structures"""
    n = len(C)
    if dense_c or sum_row_sparse:
        return np.full(n, n)
    return ((C != 0) | np.eye(n, dtype=bool)).sum(axis=1)
