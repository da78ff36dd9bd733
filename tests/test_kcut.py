"""Rounding into k parts and the 1-move local search on the GPU (Session.round_kcut) against the numpy model
(tests/kcut_model.py): vectors, labels, f before and after the search, the best trial, cones past 1024 rows on a seeded factor,
bounded contexts, the dual bound, determinism, read-only continuation, refusals and the command line's --kcutParts /
--kcutFile."""
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.kcut import read_kcut
from tests import common
from tests import kcut_model as km
from tests.test_rounding import BIG, _odd_rank_params, _phase2, _snap, big_facts, seeded_session
from tests.test_triangle_cuts import _last_error

pytestmark = pytest.mark.gpu

GOLDEN = {"maxcut100", "maxcut800", "blk4x60", "theta30", "rand120", "sdplp40", "mix4"}
SMALL = {"rank1_17": (17, 0.2), "n15": (15, 2.0), "n16": (16, 2.0), "n17": (17, 2.0), "n33": (33, 2.0)}   # n, timesLogRank


def _path(name):
    if name == "maxcut100odd":
        name = "maxcut100"
    if name in SMALL:
        n = SMALL[name][0]
        return common.generated_instance("kcut_n%d" % n, make=lambda: instances.maxcut(n, 2 * n, 900 + n))
    if name in BIG:
        return common.generated_instance(name, BIG[name])
    return common.instance_path(name) if name in GOLDEN else common.generated_instance(name)


_STATES = {}
_TMP = []


def _bounded_path():
    """maxcut100 solved, the entries below -1/2 separated and written as bound rows"""
    if not _TMP:
        import tempfile
        d = tempfile.mkdtemp(prefix="lorads_kcut_")
        s = common.hip_session(_path("maxcut100"))
        try:
            s.solve()
            b = s.entry_bounds(max_cuts=50, lower=-0.5)
            assert len(b.p) == 50
            s.write_bounded(os.path.join(d, "bounded.dat-s"), b)
        finally:
            s.close()
        _TMP.append(d)
    return os.path.join(_TMP[0], "bounded.dat-s")


SIGMA = (0.5, 1.0, 2.0, 4.0, 0.25)


def _bounded_scaled_path():
    """the bounded file with its LP columns in reverse order and column j in units of 1 / sigma_j (x_j' = sigma_j x_j, coefficient
    c / sigma_j): the same problem with unequal u_j = 1.5 sigma_j, and rows whose column is not their own number"""
    path = os.path.join(os.path.dirname(_bounded_path()), "bounded_scaled.dat-s")
    if not os.path.exists(path):
        m, b, dims, ent = km.read_sdpa(_bounded_path())
        lp = [k + 1 for k, d in enumerate(dims) if d < 0]
        assert len(lp) == 1 and dims[lp[0] - 1] == -50
        out = []
        for mat, blk, i, j, v in ent:
            if blk == lp[0]:
                assert mat > 0 and i == j
                i = j = 51 - i
                v = v / SIGMA[(i - 1) % 5]
            out.append((mat, blk, i, j, v))
        instances.write_sdpa(dict(m=m, blocks=dims, b=b, entries=out), path)
    return path


def _state(name):
    """(session, model problem, R per block, scale) after phase 1 and three ADMM steps -- a name of test_rounding's BIG: in the
    phase-1 state with a seeded R -- kept for the module"""
    if name not in _STATES and name in BIG:
        s, R = seeded_session(name)
        P = km.KCutProblem.read(_path(name))
        assert P.ok, P.why
        _STATES[name] = (s, P, R, s.results()["scale_obj_his"])
    if name not in _STATES:
        kw = _odd_rank_params() if name == "maxcut100odd" else {"timesLogRank": SMALL[name][1]} if name in SMALL else {}
        path = _bounded_path() if name == "bounded" else _bounded_scaled_path() if name == "bounded_scaled" else _path(name)
        s, _, _ = _phase2(path, **kw)
        P = km.KCutProblem.read(path)
        assert P.ok, P.why
        sol = s.solution(tol=0)
        _STATES[name] = (s, P, [c.R for c in sol.cones], s.results()["scale_obj_his"])
    return _STATES[name]


def teardown_module(module):
    import shutil
    for s, *_ in _STATES.values():
        s.close()
    _STATES.clear()
    for d in _TMP:
        shutil.rmtree(d, True)
    del _TMP[:]


def _fbound(P):
    return km.f_bound([P.C[k] for k in P.cones], [P.t[k] for k in P.cones], [P.adj[k] for k in P.cones])


def _model_start(P, R, r, parts, K):
    """model labels per cone from the device's R and G, and the trials that hold a near row"""
    lab, near = [], np.zeros(K, dtype=bool)
    for c in r.cones:
        assert c.G.shape == (parts, R[c.blk].shape[1], K) and c.rank == R[c.blk].shape[1]
        l, nr = km.labels(R[c.blk], c.G)
        near |= np.any(nr, axis=0)
        lab.append(l)
    return lab, near


def _f(P, lab, parts):
    return sum(km.objective(P.C[k], P.t[k], l, parts) for k, l in zip(P.cones, lab)).astype(np.float64)


def _cap(name, what, bad, K, none=False):
    """at most 2 % of the trials may be excluded (none: not one, so that every trial and the rounds are compared)"""
    print("%s: %d of %d trials excluded (%s)" % (name, int(bad.sum()), K, what))
    assert bad.sum() <= (0 if none else 0.02 * K), (name, what, int(bad.sum()), K)


@pytest.mark.parametrize("name", ["maxcut100", "blk4x60", "scaledpm1_120"])
def test_vectors_match_model(name):
    s, P, R, _ = _state(name)
    r = s.round_kcut(3, trials=100, seed=12345, local_search_rounds=0, tol=0, vectors=True)
    assert [c.blk for c in r.cones] == P.cones
    for c in r.cones:
        want = km.vectors(12345, c.blk, 3, c.rank, 100)
        assert np.all(np.abs(c.G - want) <= 1e-14 * np.maximum(1.0, np.abs(want))), np.abs(c.G - want).max()
    h = s.round_pm1(trials=100, seed=12345, local_search_rounds=0, tol=0, hyperplanes=True)
    for c, ch in zip(r.cones, h.cones):
        assert np.array_equal(c.G[0], ch.G)   # part 0 is the +-1 rounding's hyperplane


def _check_start(name, parts, K, seed, none_excluded=False):
    s, P, R, scale = _state(name)
    r = s.round_kcut(parts, trials=K, seed=seed, local_search_rounds=0, tol=0, vectors=True)
    assert r.rounds == 0 and np.array_equal(r.obj, r.obj0) and r.best == r.best0
    lab, near = _model_start(P, R, r, parts, K)
    _cap("%s parts=%d K=%d" % (name, parts, K), "near rows", near, K, none_excluded)
    keep = ~near
    want = _f(P, lab, parts)
    bound = _fbound(P)
    err = np.abs(r.obj0 - want)[keep]
    print("%s parts=%d K=%d: max |f - model| %.3e, bound %.3e" % (name, parts, K, err.max() if err.size else 0.0, bound))
    assert np.all(err <= bound)
    assert r.best0 == int(np.argmin(r.obj0)) and r.f_best0 == r.obj0[r.best0]
    for c, l in zip(r.cones, lab):
        assert np.array_equal(c.t, P.t[c.blk])
        assert np.array_equal(c.sizes, np.bincount(c.label, minlength=parts)) and c.label.max() < parts
        if keep[r.best]:
            assert np.array_equal(c.label, l[:, r.best])
    return r


@pytest.mark.parametrize("K", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("parts", [2, 3, 5, 16, 64])
def test_labels_and_f_maxcut100(parts, K):
    _check_start("maxcut100", parts, K, seed=K + parts)


NAMES = ["blk4x60", "blkmix5", "wmaxcut150", "scaledpm1_120", "densemaxcut120", "maxcut100odd", "rank1_17", "n15", "n16", "n17", "n33"]


@pytest.mark.parametrize("parts", [3, 4])
@pytest.mark.parametrize("name", NAMES)
def test_labels_and_f(name, parts):
    s, P, R, _ = _state(name)
    if name == "maxcut100odd":
        assert R[0].shape[1] % 2 == 1
    if name == "rank1_17":
        assert R[0].shape == (17, 1)
    _check_start(name, parts, 200, seed=7 + parts)


def _check_search(name, parts, K, seed, none_excluded=False):
    s, P, R, scale = _state(name)
    r = s.round_kcut(parts, trials=K, seed=seed, local_search_rounds=100, tol=0, vectors=True)
    lab0, near = _model_start(P, R, r, parts, K)
    bound = _fbound(P)
    assert np.all(r.obj <= r.obj0 + bound)   # f never rises
    assert r.best == int(np.argmin(r.obj)) and r.f_best == r.obj[r.best] and r.best0 == int(np.argmin(r.obj0))
    res = [km.local_search(P.C[k], P.t[k], P.adj[k], l, parts, 100) for k, l in zip(P.cones, lab0)]
    bad = near.copy()
    for _, _, fl in res:
        bad |= fl
    _cap("%s parts=%d K=%d" % (name, parts, K), "near rows or flagged moves", bad, K, none_excluded)
    keep = ~bad
    lab1 = [x[0] for x in res]
    err = np.abs(r.obj - _f(P, lab1, parts))[keep]
    print("%s parts=%d: rounds %d, max |f - model| %.3e, bound %.3e" % (name, parts, r.rounds, err.max() if err.size else 0.0, bound))
    assert np.all(err <= bound)
    # rounds: the longest of the kept trials (a model run on them alone); with nothing excluded, exactly the model's
    kept_rounds = max(km.local_search(P.C[k], P.t[k], P.adj[k], l[:, keep], parts, 100)[1] for k, l in zip(P.cones, lab0))
    assert r.rounds >= kept_rounds >= 1
    if keep.all():
        assert r.rounds == max(x[1] for x in res)
    if keep[r.best]:
        for c, l in zip(r.cones, lab1):
            assert np.array_equal(c.label, l[:, r.best])
    # the best trial is 1-move-optimal under the model's Delta and tau
    for c in r.cones:
        d, tau = km.move_deltas(P.C[c.blk], P.t[c.blk], c.label[:, None], parts)
        assert np.all(d[:, 0] >= -1.01 * tau - 1e-300), (c.blk, d[:, 0].min())
    return r


@pytest.mark.parametrize("parts", [3, 4])
@pytest.mark.parametrize("name", ["maxcut100", "blk4x60", "blkmix5", "wmaxcut150", "scaledpm1_120", "densemaxcut120", "maxcut100odd"])
def test_local_search(name, parts):
    _check_search(name, parts, 200, seed=99)


@pytest.mark.parametrize("name,parts", [("maxcut100", 17), ("maxcut100", 64), ("densemaxcut120", 17)])
def test_local_search_many_parts(name, parts):
    """more parts than one walk of the row list holds sums for (16): the second and later walks, their argmin across walks and the
    current part's sum found in a later walk"""
    _check_search(name, parts, 200, seed=31)


# Cones past 1024 rows on a seeded factor (test_rounding's BIG: the field pass's second trip over the rows of a cone and over the row
# list of a colour class).  K = 65: two label blocks per row, the second with one live lane; K = 20: a second, ragged 16-trial label
# tile.  The bound on |f - model| is f_bound, as everywhere.
BIG_CASES = [("big2100", 3, 65), ("big2100", 17, 20), ("densebig1100", 3, 20), ("mixbig", 4, 20)]


def _big_facts(name):
    s, P, R, scale = _state(name)
    big_facts(name, s, scale, [(P.C[k], P.t[k], P.adj[k], R[k]) for k in P.cones])


@pytest.mark.parametrize("name,parts,K", [c for c in BIG_CASES if c[1] != 17])
def test_big_cones_labels_and_f(name, parts, K):
    """the evaluation's row loop carries its partial sum over a second trip (and a third on 2100 rows)"""
    _big_facts(name)
    _check_start(name, parts, K, seed=7 + parts, none_excluded=True)


@pytest.mark.parametrize("name,parts,K", BIG_CASES)
def test_big_cones_local_search(name, parts, K):
    """the search on the same cones: on the sparse ones the first colour class is a row list of more than 1024 entries, read on a
    second trip; with 17 parts every row is walked twice (KCUT_CH = 16 sums per walk)"""
    _big_facts(name)
    _check_search(name, parts, K, seed=99, none_excluded=True)


def test_two_parts_is_the_flip_rule():
    """parts = 2: rounds and final f are the model's, whose move rule is the +-1 search's flip rule (coef 4, the same tau)"""
    r = _check_search("maxcut100", 2, 256, seed=5)
    s, P, R, _ = _state("maxcut100")
    from tests import rounding_model as rm
    sig = np.where(r.cones[0].label == 0, 1, -1).astype(np.int8)[:, None]
    d, tau = rm.deltas(P.C[0], P.t[0], sig)
    assert np.all(d[:, 0] >= -1.01 * tau - 1e-300)   # 1-flip-optimal in the +-1 rounding's own terms
    assert abs(float(rm.objective(P.C[0], P.t[0], sig)[0]) - r.f_best) <= _fbound(P)


def test_bounded_context():
    s, P, R, _ = _state("bounded")
    assert len(P.rows) == 50 and P.lp == [1] and P.cones == [0]
    _check_start("bounded", 3, 200, seed=11)
    r = _check_search("bounded", 3, 200, seed=12)
    assert r.lp_columns == 50 and np.array_equal(r.lp_upper, P.u) and np.all(P.u == 1.5)
    with pytest.raises(NotImplementedError, match="LP block"):
        s.round_pm1(trials=8)
    # X(l) of the best trial meets every bound row: lower = -1/2 = -t_p t_q / (k - 1)
    X = km.point(P.t[0], r.cones[0].label, 3)
    assert all(X[p, q] >= -0.5 for _, _, p, q, _, _, _ in P.rows)


def test_bounded_context_unequal_columns():
    """the same bound rows with the LP columns reversed and rescaled: u_j differs from column to column, so a wrong column of a row
    (in the check, or where the bound reads u of a slack entry) shows"""
    s, P, R, _ = _state("bounded_scaled")
    assert len(P.rows) == 50 and P.lp == [1] and P.cones == [0]
    assert [j for _, _, _, _, _, j, _ in P.rows] == list(range(49, -1, -1))
    assert np.array_equal(P.u, 1.5 * np.array([SIGMA[j % 5] for j in range(50)])) and not np.array_equal(P.u, P.u[::-1])
    _check_start("bounded_scaled", 3, 200, seed=11)
    r = _check_search("bounded_scaled", 3, 200, seed=12)
    assert r.lp_columns == 50 and np.array_equal(r.lp_upper, P.u)


def _model_bound(name):
    """(result of a call at tol 1e-8, the model's d from the exported y and S, the LP slack per column (empty without an LP block),
    the exported y)"""
    s, P, R, _ = _state(name)
    r = s.round_kcut(3, trials=64, seed=1, local_search_rounds=10, tol=1e-8)
    sol = s.solution(tol=1e-8)
    lam, slack = [], np.zeros(0)
    for k, c in enumerate(sol.cones):
        row, col, val = sol.slack(k)
        if c.is_lp:
            slack = np.zeros(c.n)
            slack[row] = val
            continue
        S = np.zeros((c.n, c.n))
        S[row, col] = val
        S[col, row] = val
        lam.append(float(np.linalg.eigvalsh(S)[0]))
    d = km.dual_bound(P.b, sol.y, [P.T(k) for k in P.cones], lam, P.u if P.lp else (), slack)
    return r, d, slack, sol.y


@pytest.mark.parametrize("name", ["maxcut100", "scaledpm1_120", "blk4x60", "bounded", "bounded_scaled"])
def test_dual_bound(name):
    s, P, R, _ = _state(name)
    r, d, slack, y = _model_bound(name)
    tol = 1e-8 * max(1.0, abs(d))
    assert abs(r.bound - d) <= tol, (r.bound, d)
    assert abs(r.by - float(P.b @ y)) <= 1e-12 * max(1.0, abs(r.by))
    assert r.bound <= r.f_best + tol
    assert r.gap == pytest.approx((r.f_best - r.bound) / max(1.0, abs(r.bound)), rel=1e-15)
    assert r.lp_negative == int(np.sum(slack < 0))
    if P.lp:
        print("%s: %d of %d LP slacks negative, sum u_j min(0, s_j) = %.6e" % (name, r.lp_negative, len(P.u), P.u @ np.minimum(0.0, slack)))
    for c in r.cones:
        assert c.T == pytest.approx(P.T(c.blk), rel=1e-15)


def test_dual_bound_uses_the_lp_term():
    """the LP term of d is not idle in test_dual_bound: on the column-scaled context some s_j < 0, and the u_j of the mirrored
    column in their place would move d by more than the tolerance d is compared to there"""
    u = _state("bounded_scaled")[1].u
    r, d, slack, _ = _model_bound("bounded_scaled")
    smin, tol = np.minimum(0.0, slack), 1e-8 * max(1.0, abs(d))
    print("bounded_scaled: LP term %.6e, with mirrored u %.6e, tolerance %.3e" % (u @ smin, u[::-1] @ smin, tol))
    assert r.lp_negative > 0 and u @ smin < 0
    assert abs(u @ smin - u[::-1] @ smin) > 2 * tol


def test_kpartite_finds_the_planted_partition():
    path = _path("kpartite3x10")
    P = km.KCutProblem.read(path)
    s = common.hip_session(path, phase2Tol=1e-4)
    try:
        s.solve()
        r = s.round_kcut(3, trials=256, seed=0, local_search_rounds=100, tol=1e-8)
    finally:
        s.close()
    planted = (np.arange(30) // 10).astype(np.uint8)[:, None]
    fstar = float(km.objective(P.C[0], P.t[0], planted, 3)[0])
    assert fstar == -225.0
    print("kpartite3x10: f_best %.12f (before the search %.12f), bound %.9f, rounds %d" % (r.f_best, r.f_best0, r.bound, r.rounds))
    assert abs(r.f_best - fstar) <= _fbound(P)
    assert abs(-2.0 * r.f_best * 2 / 3 - 300.0) <= 1e-9
    lab = r.cones[0].label.reshape(3, 10)
    assert np.all(lab == lab[:, :1]) and sorted(lab[:, 0].tolist()) == [0, 1, 2]
    assert r.bound <= r.f_best + 1e-8 * 225


def test_determinism_and_trial_independence():
    s, P, R, _ = _state("blk4x60")
    a = s.round_kcut(3, trials=1000, seed=77, local_search_rounds=100, tol=0, vectors=True)
    b = s.round_kcut(3, trials=1000, seed=77, local_search_rounds=100, tol=0, vectors=True)
    assert np.array_equal(a.obj, b.obj) and np.array_equal(a.obj0, b.obj0) and a.best == b.best and a.rounds == b.rounds
    assert np.array_equal(a.label, b.label)
    for K in (64, 65):
        c = s.round_kcut(3, trials=K, seed=77, local_search_rounds=100, tol=0, vectors=True)
        for k in range(len(a.cones)):
            assert np.array_equal(c.cones[k].G, a.cones[k].G[:, :, :K])
        assert np.array_equal(c.obj0, a.obj0[:K]) and np.array_equal(c.obj, a.obj[:K])
        if c.best == a.best:
            assert np.array_equal(c.label, a.label)
    c65, c64 = s.round_kcut(3, trials=65, seed=77, tol=0), s.round_kcut(3, trials=64, seed=77, tol=0)
    if c65.best == c64.best:
        assert np.array_equal(c65.label, c64.label)
    d = s.round_kcut(3, trials=64, seed=78, local_search_rounds=0, tol=0, vectors=True)
    assert not np.array_equal(d.cones[0].G, a.cones[0].G[:, :, :64])


@pytest.mark.parametrize("name", ["maxcut100", "blk4x60"])
def test_read_only_continuation(name):
    path = _path(name)
    held = host.Session.hip_memory_stats()   # (the module's sessions stay open: their memory is part of the level)
    runs = []
    for rnd in (True, False):
        s, rho, e0 = _phase2(path, steps=0)
        try:
            a = s.admm_steps(5, rho, e0)   # (leaves a dual update waiting inside the backend)
            if rnd:
                s.round_kcut(3, trials=300, seed=3, local_search_rounds=100, tol=1e-8)
            b = s.admm_steps(5, rho, a[0])
            runs.append((a, b, _snap(s)))
        finally:
            s.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for x, y in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(x, y)
    assert host.Session.hip_memory_stats() == held


def _refused(s, code, why, call):
    held, launches = host.Session.hip_memory_stats(), s.hip_launch_count()
    assert call()[0] == code
    assert why in _last_error(s), (why, _last_error(s))
    assert host.Session.hip_memory_stats() == held and s.hip_launch_count() == launches


def test_bad_arguments_and_sharded_refusal():
    s, P, R, _ = _state("maxcut100")
    be = s.be
    _refused(s, 1, "parts 1 is outside [2, 64]", lambda: be.round_kcut(host.PAIR_UV, 1, 16))
    _refused(s, 1, "parts 65 is outside [2, 64]", lambda: be.round_kcut(host.PAIR_UV, 65, 16))
    _refused(s, 1, "above 2^20", lambda: be.round_kcut(host.PAIR_UV, 17, 65536))
    _refused(s, 1, "trials 65537", lambda: be.round_kcut(host.PAIR_UV, 2, 65537))
    _refused(s, 1, "bad argument", lambda: be.round_kcut(7, 3, 16))
    _refused(s, 1, "bad argument", lambda: be.round_kcut(host.PAIR_UV, 3, 16, max_rounds=-1))
    with pytest.raises(ValueError, match="parts 65"):
        s.round_kcut(65, trials=16)
    sh = common.hip_session(common.instance_path("blk4x60"), world=2, rank=0, separable=True)
    try:
        _refused(sh, 3, "sharded", lambda: sh.be.round_kcut(host.PAIR_RR, 3, 16))
        with pytest.raises(NotImplementedError, match="sharded"):
            sh.round_kcut(3, trials=16)
    finally:
        sh.close()


@pytest.mark.parametrize("name,why", [("theta30", "entries"), ("rand120", "entries"), ("mix4", "entries"),
                                      ("maxcut_uncovered60", "diagonal 60"), ("maxcut_negratio60", "b / a"), ("sdplp40", None)])
def test_refusals(name, why):
    path = _path(name)
    if why is None:   # the model's check walks the constraints as the library does: the same first reason, word for word
        why = km.KCutProblem.read(path).why
        assert why == "constraint 1 has an LP entry and a diagonal entry" or why.startswith("constraint 1 has")
    s = common.hip_session(path)
    try:
        _refused(s, 2, why, lambda: s.be.round_kcut(host.PAIR_RR, 3, 0))
        _refused(s, 2, why, lambda: s.be.round_kcut(host.PAIR_RR, 3, 8))
        with pytest.raises(NotImplementedError, match="k-cut-structured"):
            s.round_kcut(3, trials=0)
    finally:
        s.close()


def test_cli(tmp_path):
    exe = os.path.join(host.LIB_DIR, "lorads")
    path = common.instance_path("maxcut100")
    out = tmp_path / "kcut.txt"
    p = subprocess.run([exe, path, "--kcutParts", "3", "--kcutTrials", "128", "--kcutFile", str(out)], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr
    assert "Rounding into 3 parts (128 trials" in p.stdout and "dual bound d" in p.stdout and "gap" in p.stdout
    s = common.hip_session(path)
    try:
        s.solve()
        s.write_kcut(tmp_path / "py.txt", 3, trials=128, seed=0, local_search_rounds=100, tol=1e-8)
        mine = s.round_kcut(3, trials=128, seed=0, local_search_rounds=100, tol=1e-8)
    finally:
        s.close()
    assert (tmp_path / "py.txt").read_bytes() == out.read_bytes()
    got = read_kcut(out)
    assert got.best == mine.best and got.f_best == mine.f_best and got.bound == mine.bound and got.parts == 3
    assert np.array_equal(got.label, mine.label)
    bad = subprocess.run([exe, common.instance_path("theta30"), "--kcutParts", "3"], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 2
    assert "End Program" not in bad.stdout and "k-cut-structured" in bad.stderr
