"""The trial chunks of the one-trial-per-workgroup roundings (stable sets, bisections).  A chunk holds 2^24 (trial, vertex) pairs, so
no call a test can afford walks more than one; LORADS_TRIAL_CHUNK, read when the context is created, caps the trials per chunk.  A
call of 40 trials in chunks of 16 -- three chunks, the last one short -- and a call of 16 trials in one full chunk must give, bit
for bit, what a fresh context without the cap gives on the same seeded factors: the other tests pin that path to the models.  The
long-row bisection cases (tests/bisect_cases.py) go in chunks of 2 of 5 trials."""
import numpy as np
import pytest

from lorads_amd import host
from tests import bisect_cases as bc
from tests import common
from tests.test_bisection import INST as BIS_INST
from tests.test_stable_set import _graph_problem, _named, _random_edges

pytestmark = pytest.mark.gpu

RR = host.PAIR_RR
L = 100
PICK = (3, 20, 39)   # one trial of each of the three chunks of 40 trials


def _stable_cones(name):
    if name == "two33_17":   # two cones of unequal n
        rng = np.random.default_rng(3317)
        return [(33, _random_edges(rng, 33, 50)), (17, _random_edges(rng, 17, 30))]
    return _named(name)


def _stable_path(name):
    tag = "chunks_stable_" + name
    return common.generated_instance(tag, lambda: _graph_problem(_stable_cones(name), len(tag)))


def _bisect_path(name, inst=BIS_INST):
    return common.generated_instance("chunks_bis_" + name, inst[name][0])


def _fresh(monkeypatch, path, chunk, env, rank=None):
    """a context of its own, created with LORADS_TRIAL_CHUNK = chunk (None: unset) and `env`, holding seeded factors R"""
    monkeypatch.delenv("LORADS_TRIAL_CHUNK", raising=False)
    if chunk is not None:
        monkeypatch.setenv("LORADS_TRIAL_CHUNK", str(chunk))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = common.hip_session(path, **({"timesLogRank": 1e-3} if rank else {}))
    if rank:
        s.be.resize_rank([rank] * s.nblk)
    rng = np.random.default_rng(77)
    for k in range(s.nblk):
        s.be.set_mat(host.MAT_R, k, rng.standard_normal(s.block_shape(k)))
    return s


def _same(a, b, keys, lists):
    for key in keys:
        assert np.array_equal(a[key], b[key]), key
    for key in lists:   # per cone
        assert len(a[key]) == len(b[key]) and all(np.array_equal(x, y) for x, y in zip(a[key], b[key])), key


def _stable(monkeypatch, name, chunk, K):
    s = _fresh(monkeypatch, _stable_path(name), chunk, {}, rank=3)
    try:
        rc, d = s.be.round_stable(RR, K, 11, L, want_scores=True)
        assert rc == 0
        return d, [s.be.stable_trial(t).copy() for t in PICK if t < K]
    finally:
        s.close()


@pytest.mark.parametrize("K", [40, 16])
@pytest.mark.parametrize("name", ["cliques35", "two33_17"])
def test_stable_sets_in_chunks(monkeypatch, name, K):
    want, wt = _stable(monkeypatch, name, None, K)
    got, gt = _stable(monkeypatch, name, 16, K)
    assert want["sizes"].shape[1] == K and len(want["obj"]) == K
    _same(got, want, ["obj", "obj0", "best", "best0", "sizes", "rounds", "member"], ["scores"])
    assert len(gt) == len(wt) and all(np.array_equal(x, y) for x, y in zip(gt, wt))


def _bisect(monkeypatch, name, chunk, K, env, inst=BIS_INST, pick=PICK):
    s = _fresh(monkeypatch, _bisect_path(name, inst), chunk, dict(inst[name][1], **env))
    try:
        rc, d = s.be.round_bisect(RR, K, 13, 1000, want_hyperplanes=True)
        assert rc == 0
        return d, [s.be.bisect_trial(t).copy() for t in pick if t < K]
    finally:
        s.close()


@pytest.mark.parametrize("env", [{}, {"LORADS_BISECT_LDS": "0"}], ids=["lds", "slab"])
@pytest.mark.parametrize("name,K", [("d40", 40), ("two", 40), ("two", 16)])
def test_bisections_in_chunks(monkeypatch, name, K, env):
    """`two`: cones of 24 and 40 rows.  The slab path indexes a trial's fields by its place in the chunk."""
    want, wt = _bisect(monkeypatch, name, None, K, env)
    got, gt = _bisect(monkeypatch, name, 16, K, env)
    assert want["imbalance"].shape[1] == K and len(want["obj"]) == K
    _same(got, want, ["obj", "obj0", "best", "best0", "sign", "imbalance", "rounds"], ["hyperplanes"])
    assert len(gt) == len(wt) and all(np.array_equal(x, y) for x, y in zip(gt, wt))


@pytest.mark.parametrize("env", [{}, {"LORADS_BISECT_LDS": "0"}], ids=["lds", "slab"])
@pytest.mark.parametrize("name", ["mixed", "densec300"])
def test_long_row_bisections_in_short_chunks(monkeypatch, name, env):
    """5 trials in chunks of 2 -- three chunks, the last one short -- on cones of 300 rows whose row lists outgrow the workgroup
    (mixed: beside a cone of 24 rows with another t and d; densec300: rows of Cfull): a slab row starts at (place in the chunk) * n
    with n = 300, and every trial is read back"""
    K, every = 5, tuple(range(5))
    want, wt = _bisect(monkeypatch, name, None, K, env, bc.LONG, every)
    got, gt = _bisect(monkeypatch, name, 2, K, env, bc.LONG, every)
    assert want["imbalance"].shape[1] == K and len(want["obj"]) == K and len(wt) == K
    assert want["rounds"] > 20 and np.all(want["obj"] < want["obj0"])
    _same(got, want, ["obj", "obj0", "best", "best0", "sign", "imbalance", "rounds", "t", "diff"], ["hyperplanes"])
    assert len(gt) == len(wt) and all(np.array_equal(x, y) for x, y in zip(gt, wt))
