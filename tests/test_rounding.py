"""Hyperplane rounding and 1-flip local search on the GPU (Session.round_pm1) against the numpy model (tests/rounding_model.py):
hyperplanes, signs, f before and after the search, the best trial, cones past 1024 rows on a seeded factor, the dual bound,
determinism, read-only continuation, refusals and the command line's --roundTrials / --roundFile."""
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.rounding import read_rounding
from tests import common
from tests import rounding_model as rm

pytestmark = pytest.mark.gpu

UNIT = {"maxcut100", "maxcut800", "blk4x60", "blkmix5", "densemaxcut120", "maxcut100odd", "big2100", "densebig1100", "mixbig"}
GOLDEN = {"maxcut100", "maxcut800", "blk4x60", "theta30", "rand120", "sdplp40", "mix4"}


# Cones past 1024 rows, rounded from a seeded factor in the phase-1 state (source R).  One trip of the field pass covers FIELD_TRIP
# rows: RND_STRIPS = 256 strips of TPB / 64 = 4 wavefronts, one row each (csrc/hip/rounding.inc).  The evaluation always launches the
# 256 strips; a colour-class pass of the search launches min(256, ceil(rows / 4)).  Unit weights: C holds multiples of 1/4.
BIG = {
    "big2100": lambda: instances.maxcut(2100, 2100, 3000),               # sparse C; the first colour class alone has more than 1024 rows
    "densebig1100": lambda: instances.dense_maxcut(1100, 70000, 1101),   # C kept dense (Cfull, stride npad)
    "mixbig": lambda: instances.block_diag([instances.maxcut(90, 140, 71), instances.maxcut(2100, 2100, 3000),
                                            instances.maxcut(120, 250, 72)]),   # a small cone before and after a large one
}
FIELD_TRIP = 1024
BIG_SEED = 20261


def field_trips(nrows, search):
    """trips of the field pass's row loop over nrows rows, from the launch rule restated: the evaluation launches 256 strips, a
    colour-class pass of the search min(256, ceil(nrows / 4)); a strip holds 4 wavefronts, each with one row per trip"""
    strips = max(1, min(256, -(-nrows // 4))) if search else 256
    return -(-nrows // (4 * strips))


def seeded_session(name):
    """(context of the generated instance `name` in its phase-1 state with R of every cone drawn from a fixed generator, R per cone
    as the device holds it)"""
    s = common.hip_session(_path(name))
    rng = np.random.default_rng(BIG_SEED)
    for k in range(s.nblk):
        s.be.set_mat(host.MAT_R, k, rng.standard_normal(s.block_shape(k)))
    return s, [s.be.get_mat(host.MAT_R, k) for k in range(s.nblk)]


def class_sizes(adj):
    """rows per colour class of one cone (the model's greedy colouring)"""
    return np.bincount(rm.colouring(adj))


def _path(name):
    if name == "maxcut100odd":
        name = "maxcut100"
    if name in BIG:
        return common.generated_instance(name, BIG[name])
    return common.instance_path(name) if name in GOLDEN else common.generated_instance(name)


def _odd_rank_params():
    """a timesLogRank that gives maxcut100 an odd rank (the device pads it with a zero column)"""
    for f in (1.5, 1.7, 1.9, 2.1, 2.3, 2.5, 1.3, 1.1):
        s = host.Session.open(common.instance_path("maxcut100"))
        try:
            s.set_params(verbose=0, timesLogRank=f)
            s.prepare()
            if s.block_info(0)["rank"] % 2 == 1:
                return {"timesLogRank": f}
        finally:
            s.close()
    raise AssertionError("no odd rank found")


def _phase2(path, steps=3, **kw):
    s = common.hip_session(path, **kw)
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
    """(session, model problem, R per cone, scale) after phase 1 and three ADMM steps -- a name of BIG: in the phase-1 state with a
    seeded R -- kept for the module"""
    if name not in _STATES and name in BIG:
        s, R = seeded_session(name)
        P = rm.Pm1Problem.read(_path(name))
        assert P.ok
        _STATES[name] = (s, P, R, s.results()["scale_obj_his"])
    if name not in _STATES:
        kw = _odd_rank_params() if name == "maxcut100odd" else {}
        s, _, _ = _phase2(_path(name), **kw)
        P = rm.Pm1Problem.read(_path(name))
        assert P.ok
        sol = s.solution(tol=0)
        _STATES[name] = (s, P, [c.R for c in sol.cones], s.results()["scale_obj_his"])
    return _STATES[name]


def teardown_module(module):
    for s, *_ in _STATES.values():
        s.close()
    _STATES.clear()


def _model_start(P, R, r, K):
    """model signs from the device's R and G; trials with a near-zero projection |R_p.g| <= 1e-12 |R_p| |g| are flagged"""
    sig, near = [], np.zeros(K, dtype=bool)
    for k, c in enumerate(r.cones):
        G = c.G
        assert G.shape == (R[k].shape[1], K) == (c.rank, K)
        s, proj = rm.signs(R[k], G)
        bound = 1e-12 * np.linalg.norm(R[k], axis=1)[:, None] * np.linalg.norm(G, axis=0)[None, :]
        near |= np.any(np.abs(proj) <= bound, axis=0)
        sig.append(s)
    return sig, near


def _f(P, sig):
    return sum(rm.objective(P.C[k], P.t[k], s) for k, s in enumerate(sig))


def _assert_f(got, want, exact):
    if exact:
        assert np.array_equal(got, want), np.abs(got - want).max()
    else:
        assert np.all(np.abs(got - want) <= 1e-13 * np.maximum(1.0, np.abs(want))), np.abs(got - want).max()


@pytest.mark.parametrize("name", ["maxcut100", "blk4x60", "scaledpm1_120"])
def test_hyperplanes_match_model(name):
    s, P, R, _ = _state(name)
    r = s.round_pm1(trials=100, seed=12345, local_search_rounds=0, tol=0, hyperplanes=True)
    for k, c in enumerate(r.cones):
        assert c.rank == R[k].shape[1]
        want = rm.hyperplanes(12345, k, c.rank, 100)
        assert np.all(np.abs(c.G - want) <= 1e-14 * np.maximum(1.0, np.abs(want))), np.abs(c.G - want).max()


NAMES = ["maxcut100", "maxcut800", "blk4x60", "blkmix5", "wmaxcut150", "scaledpm1_120", "densemaxcut120", "maxcut100odd"]


def _check_start(name, K, seed):
    s, P, R, scale = _state(name)
    r = s.round_pm1(trials=K, seed=seed, local_search_rounds=0, tol=0, hyperplanes=True)
    assert r.rounds == 0 and np.array_equal(r.obj, r.obj0) and r.best == r.best0
    sig, near = _model_start(P, R, r, K)
    keep = ~near
    print("%s K=%d: %d trials with a near-zero projection excluded" % (name, K, int(near.sum())))
    _assert_f(r.obj0[keep], _f(P, sig)[keep], exact=name in UNIT and scale == 1.0)
    # best trial: argmin with the lowest index on ties; its signs and x = sigma o t
    assert r.best0 == int(np.argmin(r.obj0)) and r.f_best0 == r.obj0[r.best0]
    for k, c in enumerate(r.cones):
        assert np.array_equal(c.t, P.t[k])
        assert np.array_equal(c.x, c.sigma * c.t)
        if keep[r.best]:
            assert np.array_equal(c.sigma, sig[k][:, r.best])
    return near


@pytest.mark.parametrize("K", [1, 63, 64, 1000])
@pytest.mark.parametrize("name", NAMES)
def test_rounding_without_local_search(name, K):
    if name == "maxcut100odd":
        assert _state(name)[2][0].shape[1] % 2 == 1
    _check_start(name, K, seed=K + 3)


def _check_search(name, K, seed):
    s, P, R, scale = _state(name)
    r = s.round_pm1(trials=K, seed=seed, local_search_rounds=100, tol=0, hyperplanes=True)
    sig0, near = _model_start(P, R, r, K)
    keep = ~near
    assert np.all(r.obj <= r.obj0 + 1e-13 * np.maximum(1.0, np.abs(r.obj0)))
    assert r.best == int(np.argmin(r.obj)) and r.f_best == r.obj[r.best] and r.best0 == int(np.argmin(r.obj0))
    if name in UNIT and scale == 1.0:
        res = [rm.local_search(P.C[k], P.t[k], P.adj[k], sg, 100) for k, sg in enumerate(sig0)]
        sig1 = [x[0] for x in res]
        assert np.array_equal(r.obj[keep], _f(P, sig1)[keep])
        if keep.all():
            assert r.rounds == max(x[1] for x in res)
        if keep[r.best]:
            for k, c in enumerate(r.cones):
                assert np.array_equal(c.sigma, sig1[k][:, r.best])
    # the best trial is 1-opt under the model's Delta and tau, and its f recomputed equals f_best
    f = 0.0
    for k, c in enumerate(r.cones):
        d, tau = rm.deltas(P.C[k], P.t[k], c.sigma[:, None].astype(np.int8))
        assert np.all(d[:, 0] >= -1.01 * tau - 1e-300), (k, d[:, 0].min())
        f += float(c.x @ P.C[k] @ c.x)
    assert abs(f - r.f_best) <= 1e-13 * max(1.0, abs(f))
    assert r.rounds >= 1
    return r, near


@pytest.mark.parametrize("name", ["maxcut100", "maxcut800", "blk4x60", "blkmix5", "densemaxcut120", "wmaxcut150", "scaledpm1_120"])
def test_local_search(name):
    _check_search(name, 256, seed=99)


def big_facts(name, s, scale, cones):
    """what a case past 1024 rows rests on, asserted from the model (cones: (C, t, adj, R) per cone) and the device's image of the
    cone: a cone whose evaluation takes a second trip; on the sparse ones a colour class whose search pass takes a second trip; on
    the dense one C kept dense; every product C_pq t_p t_q a multiple of 1/4 and the objective unscaled"""
    assert scale == 1.0
    dims = [len(t) for _, t, _, _ in cones]
    k = int(np.argmax(dims))
    n, cls = dims[k], class_sizes(cones[k][2])
    assert n > FIELD_TRIP and field_trips(n, search=False) >= 2
    if name == "densebig1100":
        assert s.hip_block_image(k)["dense_c"] == 1
    else:
        assert s.hip_block_image(k)["dense_c"] == 0
        assert cls.max() > FIELD_TRIP and field_trips(int(cls.max()), search=True) == 2
    if name == "mixbig":   # the large cone between two that leave most strips without a row
        assert dims == [90, 2100, 120] and k == 1
    assert all(np.array_equal(4 * C, np.round(4 * C)) and np.all(t == 1.0) for C, t, _, _ in cones)
    print("%s: cone %d of %d rows (rank %d), classes %s: trips %d (evaluation), %d (search, largest class)"
          % (name, k, n, cones[k][3].shape[1], cls.tolist() if len(cls) <= 8 else "%d of up to %d rows" % (len(cls), cls.max()),
             field_trips(n, search=False), field_trips(int(cls.max()), search=True)))


def _big_facts(name):
    s, P, R, scale = _state(name)
    big_facts(name, s, scale, [(P.C[k], P.t[k], P.adj[k], R[k]) for k in range(len(P.dims))])


BIG_K = 65   # two sign words per row, the second with one live lane


@pytest.mark.parametrize("name", sorted(BIG))
def test_big_cones_without_local_search(name):
    """cones past 1024 rows: the evaluation's row loop carries its partial sum over a second trip (and a third on 2100 rows)"""
    _big_facts(name)
    near = _check_start(name, BIG_K, seed=BIG_K + 3)
    assert not near.any()   # (every trial is compared, the best one's signs among them)


@pytest.mark.parametrize("name", sorted(BIG))
def test_big_cones_local_search(name):
    """the search on the same cones: on the sparse ones the first colour class is a row list of more than 1024 entries, read on a
    second trip; f after the search, the rounds and the best trial's signs are the model's"""
    _big_facts(name)
    r, near = _check_search(name, BIG_K, seed=99)
    assert not near.any()   # (so the rounds and the best trial's signs were compared)
    print("%s: %d rounds" % (name, r.rounds))


@pytest.mark.parametrize("name", ["maxcut100", "scaledpm1_120", "blk4x60"])
def test_dual_bound(name):
    s, P, R, _ = _state(name)
    r = s.round_pm1(trials=64, seed=1, local_search_rounds=10, tol=1e-8)
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
    for k, c in enumerate(r.cones):
        assert c.T == pytest.approx(P.T(k), rel=1e-15)


def test_maxcut800_ratio():
    s = common.hip_session(common.instance_path("maxcut800"))
    try:
        s.solve()
        r = s.round_pm1(trials=1024, seed=0, local_search_rounds=100, tol=1e-8)
    finally:
        s.close()
    print("maxcut800: cut %.6f (before the search %.6f), bound %.6f, rounds %d" % (-r.f_best, -r.f_best0, -r.bound, r.rounds))
    assert -r.f_best >= 0.878 * (-r.bound)
    assert r.f_best <= r.f_best0 and r.bound <= r.f_best


def test_phase1_state():
    path = common.instance_path("maxcut100")
    s = common.hip_session(path)
    try:
        s.alm()
        P = rm.Pm1Problem.read(path)
        R = s.be.get_mat(host.MAT_R, 0)
        r = s.round_pm1(trials=200, seed=5, local_search_rounds=0, tol=0, hyperplanes=True)
        sig, near = _model_start(P, [R], r, 200)
        _assert_f(r.obj0[~near], _f(P, sig)[~near], exact=s.results()["scale_obj_his"] == 1.0)
    finally:
        s.close()


def test_determinism_and_trial_independence():
    s, P, R, _ = _state("blk4x60")
    a = s.round_pm1(trials=1000, seed=77, local_search_rounds=100, tol=0, hyperplanes=True)
    b = s.round_pm1(trials=1000, seed=77, local_search_rounds=100, tol=0, hyperplanes=True)
    assert np.array_equal(a.obj, b.obj) and np.array_equal(a.obj0, b.obj0) and a.best == b.best and a.rounds == b.rounds
    assert np.array_equal(a.sign, b.sign)
    c = s.round_pm1(trials=64, seed=77, local_search_rounds=0, tol=0, hyperplanes=True)
    for k in range(len(a.cones)):
        assert np.array_equal(c.cones[k].G, a.cones[k].G[:, :64])
    assert np.array_equal(c.obj0, a.obj0[:64])
    d = s.round_pm1(trials=64, seed=78, local_search_rounds=0, tol=0, hyperplanes=True)
    assert not np.array_equal(d.cones[0].G, c.cones[0].G)


def _snap(s):
    nb = s.nblk
    return [s.be.get_mat(w, k) for w in (host.MAT_U, host.MAT_V) for k in range(nb)] + [s.be.get_vec(host.VEC_LAMBDA)]


@pytest.mark.parametrize("name", ["maxcut100", "blk4x60"])
def test_read_only_continuation(name):
    path = _path(name)
    runs = []
    for rnd in (True, False):
        s, rho, e0 = _phase2(path, steps=0)
        try:
            a = s.admm_steps(5, rho, e0)
            if rnd:
                s.round_pm1(trials=300, seed=3, local_search_rounds=100, tol=1e-8)
            b = s.admm_steps(5, rho, a[0])
            runs.append((a, b, _snap(s)))
        finally:
            s.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for x, y in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(x, y)


def test_sharded_refusal():
    s = common.hip_session(common.instance_path("blk4x60"), world=2, rank=0, separable=True)
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            s.round_pm1(trials=16)
    finally:
        s.close()


@pytest.mark.parametrize("name,why", [("theta30", "entries"), ("rand120", "entries"), ("sdplp40", "LP block"), ("mix4", "entries"),
                                      ("maxcut_uncovered60", "diagonal 60"), ("maxcut_negratio60", "b / a")])
def test_refusals(name, why):
    s = common.hip_session(_path(name))
    try:
        with pytest.raises(NotImplementedError, match=why):
            s.round_pm1(trials=0)
        with pytest.raises(NotImplementedError):
            s.round_pm1(trials=8)
    finally:
        s.close()


def test_cli(tmp_path):
    exe = os.path.join(host.LIB_DIR, "lorads")
    path = common.instance_path("maxcut800")
    out = tmp_path / "round.txt"
    p = subprocess.run([exe, path, "--roundTrials", "256", "--roundFile", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert "Hyperplane rounding (256 trials" in p.stdout and "dual bound d" in p.stdout and "gap" in p.stdout
    s = common.hip_session(path)
    try:
        s.solve()
        s.write_rounding(tmp_path / "py.txt", trials=256, seed=0, local_search_rounds=100, tol=1e-8)
        mine = s.round_pm1(trials=256, seed=0, local_search_rounds=100, tol=1e-8)
    finally:
        s.close()
    assert (tmp_path / "py.txt").read_bytes() == out.read_bytes()
    got = read_rounding(out)
    assert got.best == mine.best and got.f_best == mine.f_best and got.bound == mine.bound
    assert np.array_equal(got.sign, mine.sign)
    bad = subprocess.run([exe, common.instance_path("theta30"), "--roundTrials", "64"], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 2
    assert "End Program" not in bad.stdout and "+-1" in bad.stderr
