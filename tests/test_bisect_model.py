"""The bisection rounding without a GPU: the numpy model (tests/bisect_model.py) against brute force, the generators and the structure
check, the bisection file through the C writer, the command line's refusals, the oracle table and the table's layout; the model on
signed dyadic weights with t = 2 and a != 1, and the seeds of the long-row cases (tests/bisect_cases.py)."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.bisection import Bisection, BisectionCone, BisectionConeStruct, BisectionStruct, read_bisection
from tests import bisect_cases as bc
from tests import bisect_model as bm
from tests import common
from tests import rounding_model as rm


def _graph_c(rng, n, quarter_weights):
    """C = L / 4 of a seeded random graph on n vertices with weights in units of 1/4 (unit weights: w = 1)"""
    C_ = np.zeros((n, n))
    for p in range(n):
        for q in range(p + 1, n):
            if rng.random() < 0.5:
                w = float(rng.integers(1, 8)) / 4.0 if quarter_weights else 1.0
                C_[p, q] = C_[q, p] = -w / 4.0
    C_ -= np.diag(C_.sum(axis=1))
    return C_


@pytest.mark.parametrize("n", range(2, 15))
def test_model_is_balanced_never_below_brute_force_and_every_step_is_exact(n):
    """every n <= 14 and every admissible d: sum(sigma) = +-d, f >= the optimum, and every flip and swap changes f by exactly its
    Delta (weights in units of 1/4 and t = 1: the arithmetic is exact)"""
    rng = np.random.default_rng(100 + n)
    for d in range(n % 2, n + 1, 2):
        C_ = _graph_c(rng, n, quarter_weights=d % 4 == 0)
        opt = bm.brute_force(C_, 1.0, d)
        for trial in range(4):
            s0 = np.where(rng.random(n) < 0.5, 1, -1)
            log = []
            r = bm.run(C_, 1.0, d, s0, 1000, log)
            assert abs(int(r["sigma0"].sum())) == d and abs(int(r["sigma"].sum())) == d
            assert r["imbalance"] == int(s0.sum())
            assert int(r["sigma"].sum()) == int(r["sigma0"].sum())
            assert r["f"] >= opt and r["f"] <= r["f0"]
            assert r["rounds"] == sum(1 for e in log if e[0] == "swap") + 1 <= 1000
            sig = s0.astype(np.int64).copy()
            f = bm.objective(C_, 1.0, sig)
            for e in log:
                if e[0] == "flip":
                    sig[e[1]] = -sig[e[1]]
                else:
                    assert sig[e[1]] == -sig[e[2]] and e[3] < 0
                    sig[e[1]], sig[e[2]] = -sig[e[1]], -sig[e[2]]
                g = bm.objective(C_, 1.0, sig)
                assert g - f == e[-1], (e, g - f)
                f = g
            assert np.array_equal(sig, r["sigma"]) and f == r["f"]
            # the final point admits no improving swap of the round's kind
            pick = bm.swap_round(C_, 1.0, r["sigma"])
            assert pick is None or not pick[2] < 0


def test_repair_direction_and_empty_sides():
    C_ = _graph_c(np.random.default_rng(5), 8, False)
    s, D = bm.repair(C_, 1.0, 8, np.array([1, 1, -1, 1, -1, 1, 1, -1]))
    assert D == 2 and np.array_equal(s, np.ones(8))
    s, D = bm.repair(C_, 1.0, 8, np.array([-1, -1, -1, 1, -1, 1, 1, -1]))
    assert D == -2 and np.array_equal(s, -np.ones(8))
    assert bm.swap_round(C_, 1.0, s) is None and bm.swap_search(C_, 1.0, s, 10)[1] == 1
    s, D = bm.repair(C_, 1.0, 0, np.array([1, 1, 1, 1, 1, 1, -1, -1]))
    assert D == 4 and int(s.sum()) == 0 and np.array_equal(s[6:], [-1, -1])
    s, D = bm.repair(C_, 1.0, 4, np.array([-1, 1, 1, -1, -1, 1, 1, -1]))
    assert D == 0 and int(s.sum()) == 4


@pytest.mark.parametrize("m", [2, 3, 12, 16, 20])
def test_clique_pair_is_tight(m):
    """n lambda_2(L) / 4 = m = the smallest bisection"""
    prob = instances.clique_pair(m, 7 * m)
    P = bm.BisectProblem.from_instance(prob)
    assert P.ok and P.d == [0] and P.t == [1.0] and P.dims == [2 * m]
    L = 4.0 * P.C[0]
    assert np.array_equal(np.diag(L), np.full(2 * m, float(m))) and np.all(L.sum(axis=1) == 0)
    lam = np.linalg.eigvalsh(L)
    assert abs(2 * m * lam[1] / 4.0 - m) <= 1e-12 * m
    if m <= 3:
        assert bm.brute_force(P.C[0], 1.0, 0) == m
    # the planted bisection cuts the matching
    comp = np.linalg.eigh(L)[1][:, 1] > 0
    assert bm.objective(P.C[0], 1.0, np.where(comp, 1, -1)) == m
    assert not np.array_equal(instances.clique_pair(m, 1)["entries"], instances.clique_pair(m, 2)["entries"]) or m == 2


def test_generators_qualify_and_one_changed_entry_is_refused():
    for prob, d in ((instances.bisection(24, 80, 241), 0), (instances.bisection(40, 160, 401, diff=4), 4),
                    (instances.bisection(65, 300, 3, diff=1), 1), (instances.bisection(9, 12, 4, diff=9), 9),
                    (instances.bisection(30, 60, 5, weights=lambda rng, k: rng.uniform(0.5, 2.0, k)), 0)):
        P = bm.BisectProblem.from_instance(prob)
        assert P.ok and P.d == [d] and P.t == [1.0], P.why
        n = prob["blocks"][0]
        assert prob["m"] == n + 1 and prob["b"][-1] == d * d
        assert np.all(P.C[0].sum(axis=1) == 0) or d == 0 and n == 30
    P = bm.BisectProblem.from_instance(instances.block_diag([instances.bisection(24, 80, 241), instances.bisection(40, 160, 401, diff=4)]))
    assert P.ok and P.d == [0, 4] and P.dims == [24, 40]
    for name in ("bisect24", "bisect40d4", "cliquepair12", "cliquepair16"):
        assert bm.BisectProblem.from_instance(instances.NAMED[name]()).ok
    prob = instances.bisection(24, 80, 241)
    rows = [i for i, e in enumerate(prob["entries"]) if e[0] == 25]
    assert len(rows) == 24 * 25 // 2
    rng = np.random.default_rng(1)
    for i in rng.choice(rows, 12, replace=False).tolist() + [rows[0], rows[-1]]:
        ent = list(prob["entries"])
        ent[i] = ent[i][:4] + (1.0 + 2.0 ** -52,)
        assert "neither a diagonal row nor a sum row" in bm.BisectProblem.from_instance(dict(prob, entries=ent)).why
        assert not bm.BisectProblem.from_instance(dict(prob, entries=ent[:i] + ent[i + 1:])).ok
    with pytest.raises(ValueError):
        instances.bisection(24, 80, 1, diff=1)


@pytest.mark.parametrize("name,why", [("maxcut100", "cone 1 has 0 sum rows"), ("sdplp40", "LP block"), ("theta30", "neither a diagonal row"),
                                      ("rand120", "")])
def test_structure_check_rejects_goldens(name, why):
    P = bm.BisectProblem.read(common.instance_path(name))
    assert not P.ok and why in P.why, P.why


def test_structure_check_rejects_near_misses():
    prob = instances.bisection(24, 80, 241)
    n = 24
    b = prob["b"].copy()
    b[-1] = 3.0
    assert "b / (a t^2) = 3.0" in bm.BisectProblem.from_instance(dict(prob, b=b)).why
    b[-1] = 1.0
    assert "b / (a t^2) = 1.0" in bm.BisectProblem.from_instance(dict(prob, b=b)).why  # d = 1 on an even n
    b[-1] = 26.0 ** 2
    assert not bm.BisectProblem.from_instance(dict(prob, b=b)).ok                      # d > n
    two = dict(prob, m=n + 2, b=np.append(prob["b"], 4.0), entries=prob["entries"] + [(n + 2,) + e[1:] for e in prob["entries"] if e[0] == n + 1])
    assert bm.BisectProblem.from_instance(two).why == "cone 1 has 2 sum rows"
    sp = instances.scaled_pm1(24, 60, 3)
    sp = instances._with_sum_row(sp, 0)
    assert "unequal diagonal values" in bm.BisectProblem.from_instance(sp).why
    # a scaled form qualifies: a_i X_pp = b_i with b_i / a_i = 4 everywhere, the sum row 3 <11^T, X> = 3 * 4 * 2^2
    ent = [(e[0], e[1], e[2], e[3], 0.5 * e[4]) if 0 < e[0] <= n else ((e[0], e[1], e[2], e[3], 3.0) if e[0] == n + 1 else e) for e in prob["entries"]]
    P = bm.BisectProblem.from_instance(dict(prob, b=np.append(np.full(n, 2.0), 48.0), entries=ent))
    assert P.ok and P.t == [2.0] and P.d == [2]


def _bisection():
    cones = [BisectionCone(5, 3, 1, 3, 2, np.array([1, -1, 1, -1, 1], dtype=np.int8), 1.0),
             BisectionCone(4, 2, 0, 2, 2, np.array([-1, -1, 1, 1], dtype=np.int8), 0.70710678118654757)]
    return Bisection(cones, np.array([3.0000000000000004, 2.5, 7.0]), np.array([4.0, 2.5, 1.0 / 3.0]), trials=3, seed=2 ** 63 + 11,
                     max_rounds=1000, rounds=4, src=1, best=1, best0=2, scale=0.1, f_best=2.5, f_best0=1.0 / 3.0, by=2.25, bound=2.2,
                     gap=0.3, tol=1e-8)


def _to_struct(x, keep):
    st = BisectionStruct()
    for k in ("trials", "seed", "max_rounds", "rounds", "src", "best", "best0", "scale", "f_best", "f_best0", "by", "bound", "gap", "tol"):
        setattr(st.head, k, getattr(x, k))   # (the scalars sit in the struct's lrd_round_head)
    st.nblk = len(x.cones)
    obj, obj0 = (C.c_double * x.trials)(*x.obj), (C.c_double * x.trials)(*x.obj0)
    arr = (BisectionConeStruct * len(x.cones))()
    keep += [obj, obj0, arr]
    st.head.obj, st.head.obj0 = C.cast(obj, C.POINTER(C.c_double)), C.cast(obj0, C.POINTER(C.c_double))
    for q, c in zip(arr, x.cones):
        sig = (C.c_int8 * c.n)(*[int(v) for v in c.sigma])
        keep.append(sig)
        q.n, q.rank, q.diff, q.plus, q.minus, q.t = c.n, c.rank or 0, c.diff, c.plus, c.minus, c.t
        q.sigma = C.cast(sig, C.POINTER(C.c_int8))
    st.cone = C.cast(arr, C.POINTER(BisectionConeStruct))
    return st


def test_bisection_file_round_trips_byte_for_byte(tmp_path):
    """lrd_bisection_write is a pure function of the struct: written from a struct built here, read back, written again"""
    lib = host.host_lib()
    lib.lrd_bisection_write.argtypes = [C.c_char_p, C.POINTER(BisectionStruct)]
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    x, keep = _bisection(), []
    assert lib.lrd_bisection_write(os.fsencode(str(a)), C.byref(_to_struct(x, keep))) == 0
    text = a.read_text().split("\n")
    assert text[0] == "lorads-bisection 1" and text[1] == "trials 3" and text[2] == "seed %d" % (2 ** 63 + 11)
    assert "f_best 2.5" in text and "f_best0 0.33333333333333331" in text
    assert text[text.index("cone 1 5 1 3 2 1"):][:6] == ["cone 1 5 1 3 2 1", "+1", "-1", "+1", "-1", "+1"]
    assert "cone 2 4 0 2 2 0.70710678118654757" in text
    assert text[-5:] == ["objectives 3", "4 3.0000000000000004", "2.5 2.5", "0.33333333333333331 7", ""]
    y = read_bisection(str(a))
    for k in ("trials", "seed", "max_rounds", "rounds", "src", "best", "best0", "scale", "f_best", "f_best0", "by", "bound", "gap", "tol"):
        assert getattr(y, k) == getattr(x, k), k
    assert np.array_equal(y.obj, x.obj) and np.array_equal(y.obj0, x.obj0) and np.array_equal(y.sign, x.sign)
    assert [(c.n, c.diff, c.plus, c.minus, c.t) for c in y.cones] == [(c.n, c.diff, c.plus, c.minus, c.t) for c in x.cones]
    assert lib.lrd_bisection_write(os.fsencode(str(b)), C.byref(_to_struct(y, keep))) == 0
    assert a.read_bytes() == b.read_bytes()
    assert lib.lrd_bisection_write(os.fsencode(str(tmp_path / "no" / "dir.txt")), C.byref(_to_struct(x, keep))) == 2
    good = a.read_text()
    for bad in (good.replace("lorads-bisection 1", "lorads-rounding 1"), good.replace("cone 1 5 1 3 2 1", "cone 1 5 1 2 3 1"),
                good.replace("+1\n-1\n+1\n-1\n+1", "+1\n-1\n+1\n-1\n0"), good.replace("rounds 4\n", ""), good.replace("objectives 3", "objectives 2"),
                good.replace("2.5 2.5\n", "")):
        p = tmp_path / "bad.txt"
        p.write_text(bad)
        with pytest.raises(ValueError):
            read_bisection(str(p))


@pytest.mark.parametrize("args,say", [
    (["--bisectTrials", "0"], "bad value 0 of --bisectTrials"), (["--bisectTrials", "65537"], "bad value 65537 of --bisectTrials"),
    (["--bisectTrials", "-4"], "bad value -4 of --bisectTrials"), (["--bisectTrials", "x"], "bad value x of --bisectTrials"),
    (["--bisectTrials", "8", "--bisectLocalSearch", "65537"], "bad value 65537 of --bisectLocalSearch"),
    (["--bisectTrials", "8", "--bisectSeed", "1.5"], "bad value 1.5 of --bisectSeed"),
    (["--bisectFile", "x.txt"], "--bisectFile needs --bisectTrials"), (["--bisectSeed", "3"], "--bisectSeed needs --bisectTrials"),
    (["--bisectLocalSearch", "3"], "--bisectLocalSearch needs --bisectTrials")])
def test_cli_refuses_bad_values_before_the_backend(tmp_path, args, say):
    host.host_lib()
    exe = os.path.join(host.LIB_DIR, "lorads")
    # (no GPU in reach: whatever passes the options would fail with another code and message)
    r = subprocess.run([exe, common.instance_path("maxcut100")] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert say in r.stderr, r.stderr
    assert not (tmp_path / "x.txt").exists()


def test_oracle_backend_has_no_slot_and_the_table_mirror_places_it():
    path = common.generated_instance("bisect24")
    s = common.oracle_session(path)
    try:
        assert not s.be.has_round_bisect()
        with pytest.raises(NotImplementedError):
            s.round_bisection(trials=8)
        with pytest.raises(NotImplementedError):
            s.round_bisection(trials=0)
        with pytest.raises(ValueError):
            s.round_bisection(trials=65537)
        with pytest.raises(ValueError):
            s.round_bisection(trials=8, local_search_rounds=-1)
    finally:
        s.close()
    names = [f[0] for f in host.BackendStruct._fields_]
    assert names.index("certificate") + 1 == names.index("round_bisect") == names.index("get_slack") - 1
    lib = host.host_lib()
    lib.lrd_backend_sizeof.restype = C.c_size_t
    assert lib.lrd_backend_sizeof() == C.sizeof(host.BackendStruct)
    hip = C.CDLL(os.path.join(host.LIB_DIR, "liblorads_hip.so"))
    assert hasattr(hip, "lorads_hip_round_bisect") and hasattr(hip, "lorads_hip_bisect_trial")
    hdr = open(os.path.join(common.ROOT, "include", "lorads_hip.h")).read()
    assert "int lorads_hip_round_bisect(lorads_hip_ctx *ctx, int32_t src, int32_t trials, uint64_t seed, int32_t max_rounds" in hdr


# ---- the model on the data of the long-row cases (tests/bisect_cases.py): signed dyadic weights, t = 2, a != 1 ----

def test_bisection_graph_generalises_bisection():
    """bisection() is bisection_graph with t = a = 1 on the seeded graph: the entries and b of the construction it replaced (Max-Cut
    with F0 negated plus _with_sum_row), value for value and in the same order; and the scaled form's rows"""
    for args, kw in (((24, 80, 241), {}), ((40, 160, 401), dict(diff=4)), ((65, 300, 651), dict(diff=1)), ((300, 1200, 3001), {}),
                     ((150, 400, 1501), dict(weights=lambda rng, k: rng.uniform(0.5, 2.0, k)))):
        n, diff = args[0], kw.get("diff", 0)
        p = instances.maxcut(*args, weights=kw.get("weights"))
        old = instances._with_sum_row(dict(m=n, blocks=[n], b=p["b"], entries=[e[:4] + (-e[4] if e[0] == 0 else e[4],) for e in p["entries"]]), diff)
        new = instances.bisection(*args, **kw)
        assert new["m"] == old["m"] and new["blocks"] == old["blocks"] and np.array_equal(new["b"], old["b"])
        assert [tuple(float(v) for v in e) for e in new["entries"]] == [tuple(float(v) for v in e) for e in old["entries"]]
    prob = instances.bisection_graph(4, [(0, 1), (1, 3)], [0.5, -0.25], diff=2, t=2.0, a=-3.0)
    assert prob["m"] == 5 and np.array_equal(prob["b"], [2.0, 2.0, 2.0, 2.0, -48.0])
    assert [e for e in prob["entries"] if e[0] == 0] == [(0, 1, 1, 1, -0.125), (0, 1, 2, 2, -0.0625), (0, 1, 4, 4, 0.0625),
                                                        (0, 1, 1, 2, 0.125), (0, 1, 2, 4, -0.0625)]
    assert [e for e in prob["entries"] if 0 < e[0] < 5] == [(i, 1, i, i, 0.5) for i in range(1, 5)]
    assert [e for e in prob["entries"] if e[0] == 5] == [(5, 1, i, j, -3.0) for i in range(1, 5) for j in range(i, 5)]
    with pytest.raises(ValueError):
        instances.bisection_graph(4, [(0, 1)], [1.0], diff=1)


def _exact_f(Cq, t, sig):
    x = [Fraction(t) * int(s) for s in sig]
    return sum(x[p] * Cq[p][q] * x[q] for p in range(len(x)) for q in range(len(x)))


@pytest.mark.parametrize("n", range(2, 13))
def test_model_with_t2_and_signed_dyadic_weights(n):
    """t = 2, a = -3, weights from the nonzero j / 16 with j in [-8, 32] and every admissible d: the structure check finds t and d, C
    holds multiples of 1/64, the model's result is balanced and never below the brute-force optimum, `objective` is x^T C x in
    rational arithmetic, and every logged Delta is the exact change of f"""
    rng = np.random.default_rng(200 + n)
    edges = [(p, q) for p in range(n) for q in range(p + 1, n) if rng.random() < 0.6]
    w = bc.dyadic(rng, len(edges))
    assert np.all(w != 0) and np.array_equal(w * 16, np.rint(w * 16)) and w.min(initial=0) >= -0.5 and w.max(initial=0) <= 2.0
    for d in range(n % 2, n + 1, 2):
        P = bm.BisectProblem.from_instance(instances.bisection_graph(n, edges, w, diff=d, t=2.0, a=-3.0))
        assert P.ok and P.t == [2.0] and P.d == [d], P.why
        assert bc.c64_is_integral(P)
        C_ = P.C[0]
        Cq = [[Fraction(float(v)) for v in row] for row in C_]
        opt = bm.brute_force(C_, 2.0, d)
        for trial in range(3):
            s0 = np.where(rng.random(n) < 0.5, 1, -1)
            log = []
            r = bm.run(C_, 2.0, d, s0, 1000, log)
            assert abs(int(r["sigma0"].sum())) == d and int(r["sigma"].sum()) == int(r["sigma0"].sum())
            assert r["f"] >= opt and r["f"] <= r["f0"]
            assert Fraction(r["f"]) == _exact_f(Cq, 2.0, r["sigma"]) and Fraction(r["f0"]) == _exact_f(Cq, 2.0, r["sigma0"])
            sig = s0.astype(np.int64).copy()
            f = _exact_f(Cq, 2.0, sig)
            for e in log:
                for v in e[1:-1]:
                    sig[v] = -sig[v]
                g = _exact_f(Cq, 2.0, sig)
                assert g - f == Fraction(e[-1]), (e, g - f)
                f = g
            assert np.array_equal(sig, r["sigma"])


def test_structure_check_on_a_scaled_sum_row():
    """-3 <11^T, X> = -12 d^2 beside 0.5 X_pp = 2: t = 2 and d from b / (a t^2); the same problem with b off a square is refused"""
    rng = np.random.default_rng(7)
    edges = instances._rand_edges(10, 20, rng)
    for d in (0, 2, 10):
        prob = instances.bisection_graph(10, edges, bc.dyadic(rng, 20), diff=d, t=2.0, a=-3.0)
        assert prob["b"][-1] == -12.0 * d * d and all(e[4] == -3.0 for e in prob["entries"] if e[0] == 11)
        P = bm.BisectProblem.from_instance(prob)
        assert P.ok and P.t == [2.0] and P.d == [d] and P.T(0) == 40.0
        b = prob["b"].copy()
        b[-1] -= 12.0    # b / (a t^2) = d^2 + 1: no square but for d = 0, where d = 1 has the wrong parity
        Q = bm.BisectProblem.from_instance(dict(prob, b=b))
        assert not Q.ok and "b / (a t^2) = %r" % float(d * d + 1) in Q.why, Q.why
        b[-1] = 12.0 * d * d + (12.0 if d == 0 else 0.0)   # the sign of a forgotten: b / (a t^2) < 0
        assert not bm.BisectProblem.from_instance(dict(prob, b=b)).ok


@pytest.mark.parametrize("name", list(bc.LONG))
def test_seeds_of_the_long_row_cases(name):
    """what tests/test_bisection.py relies on in its long-row cases, checked here with the model's own hyperplanes at the ranks the
    contexts have: the storage rules give the row lists their length, no projection is anywhere near zero, the searches run for
    tens of rounds and are cut at 5, the hub is a swap's p and a swap's q, and the planted factor makes the hub the first flip from
    an excess on either side"""
    P = bm.BisectProblem.read(common.generated_instance("bis_long_" + name, bc.LONG[name][0]))
    assert P.ok and bc.c64_is_integral(P), P.why
    s = host.Session.open(common.generated_instance("bis_long_" + name))
    try:
        s.set_params(verbose=0)
        s.prepare(1, 0, separable=False)
        shapes = [s.block_shape(k) for k in range(s.nblk)]
    finally:
        s.close()
    assert shapes == [(n, bc.RANKS[n]) for n in P.dims]
    want = {"hub300": ([1.0], [2], [False]), "hubneg300": ([2.0], [2], [False]), "densec300": ([2.0], [0], [True]),
            "nodense300": ([1.0], [0], [False]), "mixed": ([2.0, 1.0], [2, 4], [False, True])}[name]
    dense_c = [np.count_nonzero(np.tril(C_)) > 0.1 * len(C_) * (len(C_) + 1) / 2 for C_ in P.C]
    assert (P.t, P.d, dense_c) == want
    sparse_row = [n < 32 or "LORADS_NO_DENSE_A" in bc.LONG[name][1] for n in P.dims]
    assert bc.row_lists(P.C[0], dense_c[0], sparse_row[0]).max() == 300 > bc.TPB
    if name.startswith("hub"):
        rows = bc.row_lists(P.C[0], False, False)
        assert rows[bc.HUB] == 300 and np.delete(rows, bc.HUB).max() < 16
    R = bc.case_factors(name, P, shapes)
    G = [rm.hyperplanes(bc.SEEDS[name], k, r, bc.K) for k, (_, r) in enumerate(shapes)]
    margin = min(float((np.abs(R[k] @ G[k]) / (np.linalg.norm(R[k], axis=1)[:, None] * np.linalg.norm(G[k], axis=0)[None, :])).min())
                 for k in range(len(shapes)))
    assert margin > 1e-6    # (the device's hyperplanes are the model's within 1e-14)
    M = bc.model_trials(P, R, G, 1000)
    cut = bc.model_trials(P, R, G, 5)
    rounds = [m["rounds"] for m, _ in M[0]]
    print("%s: margin %.1e, rounds %s, hub (p, q) in %s trials" % (name, margin, rounds, bc.hub_roles(M[0])))
    assert max(rounds) < 1000 and max(rounds) > 20
    assert [m["rounds"] for m, _ in cut[0]] == [min(r, 5) for r in rounds] and sum(r > 5 for r in rounds) >= 4
    if name.startswith("hub"):
        p, q = bc.hub_roles(M[0])
        assert p >= 1 and q >= 1
    if name == "hubneg300":
        R = bc.planted(bc.PLANT, shapes)
        G = [rm.hyperplanes(bc.PLANT, 0, shapes[0][1], bc.K)]
        M = bc.model_trials(P, R, G, 1000)
        D = [m["imbalance"] for m, _ in M[0]]
        assert set(D) == {300, -300}
        for m, log in M[0]:
            flips = [e for e in log if e[0] == "flip"]
            assert len(flips) == 149 and flips[0][1] == bc.HUB and flips[0][2] == -4.0 * 4.0 * 299 / 8.0
