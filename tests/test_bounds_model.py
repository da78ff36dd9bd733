"""The numpy model of the separation of entry bounds (tests/bounds_model.py) against first principles, the writer of the bounded
problem (lrd_session_write_bounded) against the model's writer, the Hamming-graph theta problem end to end through the CPU oracle
(theta = 16/3 becomes theta' = 4, twice), and the refusals that need no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.bounds import Bounds, BoundsStruct, read_bounded
from lorads_amd.cuts import read_sdpa
from tests import bounds_model as bm
from tests import common


@pytest.mark.parametrize("r", [1, 5, 6])
@pytest.mark.parametrize("n", [1, 2, 3, 33, 70])
def test_model_against_double_loop(n, r):
    rng = np.random.default_rng(100 * n + r)
    F = rng.standard_normal((n, r)) / np.sqrt(r)
    lower, upper = -0.1, 0.25
    want = {}
    for p in range(n):
        for q in range(p + 1, n):
            x = 0.0
            for k in range(r):
                x += F[p, k] * F[q, k]
            want[(p, q, 0)] = lower - x
            want[(p, q, 1)] = x - upper
    P, Q, Cl, V = bm.enumerate_all(F, lower, upper)
    assert len(V) == n * (n - 1) == len(want)
    eps = bm.eps_of(F, P, Q, Cl, lower, upper)
    keys = list(zip(P.tolist(), Q.tolist(), Cl.tolist()))
    assert set(keys) == set(want)
    assert all(abs(float(v) - want[k]) <= e for k, v, e in zip(keys, V, eps))
    # the total order: v descending, then p, q, c ascending
    o = bm.order(V, P, Q, Cl)
    srt = [(-V[i], int(P[i]), int(Q[i]), int(Cl[i])) for i in o]
    assert srt == sorted(srt)
    # a class that is off violates nothing
    _, _, Cl1, V1 = bm.enumerate_all(F, -np.inf, upper)
    assert np.all(V1[Cl1 == 0] == -np.inf) and np.array_equal(V1[Cl1 == 1], V[Cl == 1])
    sc = bm.Scan(F, lower, upper, 1e-3)
    assert sc.count_hi <= sum(1 for v in want.values() if v > 1e-3) <= sc.count_lo
    assert len(sc.v) >= sc.count_hi and np.all(np.diff(sc.v.astype(np.float64)) <= 0)


def _bounds(cuts, nblk=1):
    a = np.array([c[:4] for c in cuts], dtype=np.int64).reshape(-1, 4)
    return Bounds(np.zeros(nblk, dtype=np.int64), a[:, 0], a[:, 1], a[:, 2], a[:, 3], np.zeros(len(a)),
                  np.array([c[4] for c in cuts], dtype=np.float64))


def _random_cuts(rng, prob, count, rounds):
    """`count` cuts per round on the SDP cones of a generator dict, each round with its own pair of bounds"""
    sdp = [k for k, d in enumerate(prob["blocks"]) if d > 0]
    out = []
    for lower, upper in rounds:
        for _ in range(count):
            k = int(rng.choice(sdp))
            p, q = sorted(rng.choice(prob["blocks"][k], 2, replace=False).tolist())
            cl = int(rng.integers(0, 2))
            out.append((k, p, q, cl, upper if cl else lower))
    return out


def _same_problem(got_path, want_path):
    gm, gblocks, gb, gent = read_sdpa(got_path)
    wm, wblocks, wb, went = read_sdpa(want_path)
    assert (gm, gblocks) == (wm, wblocks)
    assert np.array_equal(gb, wb)
    assert sorted(gent) == sorted(went)


@pytest.mark.parametrize("name,rounds", [("theta30", [(0.0, 0.5)]), ("sdplp40", [(0.0, 0.5)]),
                                         ("theta30", [(0.0, 0.5), (-0.125, 0.3)]), ("sdplp40", [(0.0, 0.5), (-0.125, 0.3)])])
def test_c_writer_against_model_writer(tmp_path, name, rounds):
    """no LP block: a new last one; one LP block: it grows and the old columns keep their indices; two rounds: both classes, two
    different bound values, each cut with its own"""
    prob = instances.NAMED[name]()
    path = common.instance_path(name)
    cuts = _random_cuts(np.random.default_rng(len(name) + len(rounds)), prob, 25, rounds)
    assert {c[3] for c in cuts} == {0, 1} and len({c[4] for c in cuts}) == 2 * len(rounds)
    s = host.Session.open(path, lib=common.load_oracle())
    try:
        for tag, lst in (("cuts", cuts), ("none", [])):
            got_path, want_path = str(tmp_path / (tag + "_c.dat-s")), str(tmp_path / (tag + "_model.dat-s"))
            s.write_bounded(got_path, _bounds(lst, len(prob["blocks"])) if lst else None)
            instances.write_sdpa(bm.bounded(prob, lst), want_path)
            _same_problem(got_path, want_path)
            assert read_bounded(got_path, prob["m"]) == lst
            m, blocks, b, ent = read_sdpa(got_path)
            om, oblocks, ob, oent = read_sdpa(path)
            if not lst:   # zero cuts: the original problem
                assert (m, blocks) == (om, oblocks) and np.array_equal(b, ob) and sorted(ent) == sorted(oent)
            elif any(d < 0 for d in oblocks):   # the LP block grew where it stands; what was there is there still
                lp = [k for k, d in enumerate(oblocks) if d < 0][0]
                assert blocks == [d - len(lst) if k == lp else d for k, d in enumerate(oblocks)]
                assert sorted(e for e in ent if e[0] <= om) == sorted(oent)
            else:
                assert blocks == oblocks + [-len(lst)]
    finally:
        s.close()


def test_read_bounded_round_trip(tmp_path):
    """write, read, write what was read: the same bytes"""
    prob = instances.NAMED["sdplp40"]()
    cuts = _random_cuts(np.random.default_rng(4), prob, 30, [(0.0, 0.75), (-1e-3, 1.0 / 3.0)])
    s = host.Session.open(common.instance_path("sdplp40"), lib=common.load_oracle())
    try:
        a, b = str(tmp_path / "a.dat-s"), str(tmp_path / "b.dat-s")
        s.write_bounded(a, _bounds(cuts, 2))
        back = read_bounded(a, prob["m"])
        assert back == cuts
        s.write_bounded(b, _bounds(back, 2))
        assert open(a, "rb").read() == open(b, "rb").read()
    finally:
        s.close()
    with pytest.raises(ValueError):
        read_bounded(common.instance_path("sdplp40"), prob["m"] - 1)   # (a constraint of the problem is no bound cut)


@pytest.mark.parametrize("cut", [(0, 5, 5, 0, 0.0), (0, 7, 3, 0, 0.0), (0, -1, 3, 0, 0.0), (0, 3, 40, 0, 0.0), (2, 1, 2, 0, 0.0),
                                 (-1, 1, 2, 0, 0.0), (1, 1, 2, 0, 0.0), (0, 1, 2, 2, 0.0), (0, 1, 2, -1, 0.0), (0, 1, 2, 0, np.inf),
                                 (0, 1, 2, 1, -np.inf), (0, 1, 2, 1, np.nan)])
def test_writer_refuses(tmp_path, cut):
    """p >= q or outside the cone, a cone out of range, the LP cone (block 1 of sdplp40), a class outside {0, 1}, a bound that is not
    finite: nothing is written"""
    s = host.Session.open(common.instance_path("sdplp40"), lib=common.load_oracle())
    try:
        out = tmp_path / "bad.dat-s"
        with pytest.raises(ValueError):
            s.write_bounded(str(out), _bounds([(0, 1, 2, 0, 0.0), cut], 2))
        assert not out.exists()
    finally:
        s.close()


def test_oracle_backend_refuses_and_table_mirror():
    s = common.oracle_session(common.instance_path("theta30"))
    try:
        assert not s.be.has_entry_bounds()
        with pytest.raises(NotImplementedError):
            s.entry_bounds(max_cuts=10)
    finally:
        s.close()
    names = [f[0] for f in host.BackendStruct._fields_]
    assert names.index("triangle_cuts") + 1 == names.index("entry_bounds") == len(names) - 3
    lib = host.host_lib()
    lib.lrd_backend_sizeof.restype = C.c_size_t
    assert lib.lrd_backend_sizeof() == C.sizeof(host.BackendStruct)
    assert C.sizeof(BoundsStruct) == 104
    hip = C.CDLL(os.path.join(host.LIB_DIR, "liblorads_hip.so"))
    assert hasattr(hip, "lorads_hip_entry_bounds")


@pytest.mark.parametrize("args", [["--boundsMax", "0"], ["--boundsMax", "-3"], ["--boundsMax", "1048577"], ["--boundsMax", "12x"],
                                  ["--boundsMax", "10", "--boundsMinViolation", "-1e-3"],
                                  ["--boundsMax", "10", "--boundsMinViolation", "nan"],
                                  ["--boundsMax", "10", "--boundsMinViolation", "inf"],
                                  ["--boundsMax", "10", "--boundsLower", "nan"], ["--boundsMax", "10", "--boundsLower", "inf"],
                                  ["--boundsMax", "10", "--boundsLower", "0.1z"], ["--boundsMax", "10", "--boundsUpper", "nan"],
                                  ["--boundsMax", "10", "--boundsUpper", "-inf"],
                                  ["--boundsMax", "10", "--boundsLower", "0.5", "--boundsUpper", "0.25"],
                                  ["--boundsMax", "10", "--boundsLower", "-inf"],
                                  ["--boundsFile", "out.dat-s"], ["--boundsMinViolation", "0.01"], ["--boundsLower", "0"],
                                  ["--boundsUpper", "1"]])
def test_cli_refuses_bad_values_before_the_backend(tmp_path, args):
    host.host_lib()
    exe = os.path.join(host.LIB_DIR, "lorads")
    # (no GPU and no HIP library in reach: whatever passes the options would fail with another code and message)
    r = subprocess.run([exe, common.instance_path("theta30")] + args, cwd=tmp_path, capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "bad value" in r.stderr or "needs --boundsMax" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.dat-s")


def _factor(s):
    """the factor the separation takes: (U + V) / 2 once phase 2 has run, the phase-1 R otherwise"""
    if s.results()["admm_iter"] > 0:
        return (s.be.get_mat(host.MAT_U, 0) + s.be.get_mat(host.MAT_V, 0)) / 2
    return s.be.get_mat(host.MAT_R, 0)


def test_hamming_theta_through_the_oracle(tmp_path):
    """The graph on {0,1}^5 with an edge at Hamming distance 1 or 2: theta = 16/3; exactly the 16 antipodal entries of the solution
    are negative, and with X_pq >= 0 on them the value is theta' = 4, the size of the largest code of distance 3.  Then a second
    round on the tightened solve's factor: the LP block grows, and the value cannot improve."""
    prob = instances.hamming_theta(5, 2)
    assert prob["blocks"] == [32] and prob["m"] == 241
    path, tight, tight2 = (str(tmp_path / f) for f in ("ham5.dat-s", "ham5_b.dat-s", "ham5_b2.dat-s"))
    instances.write_sdpa(prob, path)
    s = common.oracle_session(path)
    try:
        r = s.solve()
        print("hamming theta: pObj %.9f dObj %.9f" % (r["pObj"], r["dObj"]))
        assert abs(r["pObj"] + 16.0 / 3.0) <= 2e-4
        P, Q, Cl, V = bm.enumerate_all(_factor(s), 0.0, np.inf)
        viol = V > 1e-4
        print("hamming theta: %d entries below -1e-4, the most negative %.6f" % (int(viol.sum()), -float(V.max())))
        assert int(viol.sum()) == 16
        assert sorted(zip(P[viol].tolist(), Q[viol].tolist())) == bm.antipodal_pairs(5)
        o = bm.order(V[viol], P[viol], Q[viol], Cl[viol])
        cuts = [(0, int(P[viol][i]), int(Q[viol][i]), 0, 0.0) for i in o]
        s.write_bounded(tight, _bounds(cuts))
    finally:
        s.close()
    assert read_bounded(tight, prob["m"]) == cuts
    assert read_sdpa(tight)[1] == [32, -16]
    s2 = common.oracle_session(tight, phase2Tol=1e-4)
    try:
        r2 = s2.solve()
        print("hamming theta: bounded pObj %.9f dObj %.9f" % (r2["pObj"], r2["dObj"]))
        assert abs(r2["pObj"] + 4.0) <= 5e-4
        # round two: separate on the tightened solve's factor at V = 1e-3, write onto the tightened session
        sc = bm.Scan(_factor(s2), 0.0, np.inf, 1e-3)
        cuts2 = [(0, int(p), int(q), 0, 0.0) for p, q in zip(sc.p, sc.q)]
        print("hamming theta: round two finds %d entries below -1e-3" % len(cuts2))
        s2.write_bounded(tight2, _bounds(cuts2) if cuts2 else None)
    finally:
        s2.close()
    m2, blocks2, _, _ = read_sdpa(tight2)
    assert blocks2 == [32, -(16 + len(cuts2))] and m2 == prob["m"] + 16 + len(cuts2)
    assert read_bounded(tight2, prob["m"]) == cuts + cuts2
    s3 = common.oracle_session(tight2, phase2Tol=1e-4)
    try:
        r3 = s3.solve()
    finally:
        s3.close()
    print("hamming theta: round two pObj %.9f" % r3["pObj"])
    # a minimisation over a smaller set cannot improve: not below round one's by more than the solve tolerance (phase2Tol 1e-4,
    # relative to 1 + |pObj| + |dObj|)
    assert r3["pObj"] >= r2["pObj"] - 1e-4 * (1 + abs(r2["pObj"]) + abs(r2["dObj"]))
