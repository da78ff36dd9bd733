"""Separation of entry bounds on the GPU (lorads_hip_entry_bounds, Session.entry_bounds, Session.write_bounded, --boundsMax) against
the numpy model (tests/bounds_model.py): exact counts, the selection in its total order with any number of ties, determinism,
read-only continuation, refusals, and the bounded Hamming-graph theta problem solved on the device."""
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.bounds import read_bounded
from tests import bounds_model as bm
from tests import common
from tests.test_rounding import _phase2
from tests.test_triangle_cuts import _last_error, _load, _maxcut_session, _mem, _path, _state

pytestmark = pytest.mark.gpu

TILE = 32        # BND_T of csrc/hip/bounds.inc
RR, UV = host.PAIR_RR, host.PAIR_UV
INF = float("inf")
CASES = [(0.0, INF), (-INF, 0.3), (-0.2, 0.3)]   # lower only, upper only, both


def _call(s, lower, upper, minv, K, src=RR, blk=0):
    rc, cnt, p, q, cl, v, passes = s.be.entry_bounds(src, blk, lower, upper, minv, K)
    assert rc == 0, _last_error(s)
    return cnt, p, q, cl, v, passes


SIZES = [1, 2, 3, TILE - 1, TILE, TILE + 1, 63, 64, 65, 129, 200]


@pytest.mark.parametrize("r", [6, 5, 1])
@pytest.mark.parametrize("n", SIZES)
def test_synthetic_factors_against_model(n, r):
    """random rows through set_mat, src = RR: an even rank, an odd rank (the device pads a column), r = 1; lower only, upper only,
    both; max_cuts 0, 1, 100 and more than the count"""
    rng = np.random.default_rng(1000 * n + r)
    F = rng.standard_normal((n, r)) / np.sqrt(r)
    minv = 1e-3
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        for lower, upper in CASES:
            cnt0, *_rest, passes0 = _call(s, lower, upper, minv, 0)
            assert all(len(x) == 0 for x in _rest)
            assert passes0 == (1 if n >= 2 else 0)
            if n >= TILE - 1:
                assert cnt0 > 0
            scans = [bm.Scan(F, lower, upper, minv)]
            for K in (1, 100, cnt0 + 7):
                cnt, p, q, cl, v, passes = _call(s, lower, upper, minv, K)
                assert cnt == cnt0
                assert passes >= (2 if cnt else passes0)
                bm.check_against_model([F], lower, upper, minv, K, [cnt], np.zeros(len(p)), p, q, cl, v, scans=scans)
                if upper == INF:
                    assert (cl == 0).all()
                if lower == -INF:
                    assert (cl == 1).all()
                again = _call(s, lower, upper, minv, K)
                assert again[0] == cnt and again[5] == passes
                for a, b in zip(again[1:5], (p, q, cl, v)):
                    assert a.tobytes() == b.tobytes()
            if n < 2:
                assert cnt0 == 0
    finally:
        s.close()


def test_wide_factor_reads_the_strip_from_memory():
    """a rank above the columns the row strip keeps in LDS (BND_LDS_COLS = 128): the other operand path, two row tiles and a ragged one"""
    n, r = 70, 131
    rng = np.random.default_rng(7)
    F = rng.standard_normal((n, r)) / np.sqrt(r)
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        for K in (0, 100):
            cnt, p, q, cl, v, _ = _call(s, -0.05, 0.1, 1e-3, K)
            bm.check_against_model([F], -0.05, 0.1, 1e-3, K, [cnt], np.zeros(len(p)), p, q, cl, v)
        assert cnt > 100
    finally:
        s.close()


@pytest.mark.parametrize("signed", [False, True])
def test_massive_ties(signed):
    """all rows equal, upper = 0.5: X_pq = 1 for every one of the 19900 pairs at n = 200, v = 0.5 in class 1, the same bits.  Rows
    +-f with lower = -0.5 as well: every pair ties, in class 0 where the signs differ and class 1 where they agree.  The cut-off
    group is larger than the buffer (16384 + 100 keys): the selection has to tell the pairs apart by the digits of their indices."""
    n = 200
    sign = np.where(np.arange(n) % 3 == 1, -1.0, 1.0) if signed else np.ones(n)
    F = sign[:, None] * np.array([[0.6, 0.8]])
    lower = -0.5 if signed else -INF
    s = _maxcut_session(n, 2)
    try:
        _load(s, F)
        cnt, p, q, cl, v, passes = _call(s, lower, 0.5, 0.25, 100)
        print("massive ties: count %d, kept %d, passes %d, v in [%.17g, %.17g]" % (cnt, len(p), passes, v.min(), v.max()))
        assert cnt == n * (n - 1) // 2 == 19900
        assert len(p) == 100 and passes > 3
        eps = bm.eps_of(F, p, q, cl, lower, 0.5)
        assert np.all(np.abs(v - 0.5) <= eps)
        assert len(set(v.tolist())) == 1    # (the same two rows up to sign: the same bits)
        want = [(a, b) for a in range(n) for b in range(a + 1, n)][:100]
        assert list(zip(p.tolist(), q.tolist())) == want
        assert cl.tolist() == [int(sign[a] == sign[b]) for a, b in want]
        again = _call(s, lower, 0.5, 0.25, 100)
        assert again[0] == cnt and again[5] == passes
        for a, b in zip(again[1:5], (p, q, cl, v)):
            assert a.tobytes() == b.tobytes()
    finally:
        s.close()


def _quantile_bounds(F):
    """bounds that leave a good share of the entries of X = F F^T outside: the 30 % and 80 % quantiles of its off-diagonal entries
    (from the factors, in numpy), and a threshold a thousandth of their distance"""
    x = np.concatenate([(f @ f.T)[np.triu_indices(f.shape[0], 1)] for f in F])
    lo, up = np.quantile(x, [0.3, 0.8])
    return float(lo), float(up), float(1e-3 * (up - lo))


@pytest.mark.parametrize("name", ["blkmix5", "blk4x60", "theta30", "densea40", "sdplp40"])
def test_solved_states_against_model(name):
    """Session.entry_bounds after phase 1 and three ADMM steps (src = UV: F = (U + V) / 2 formed on the device) against the model on
    the exported factors: cones of a common rank (blkmix5: the pad columns are not read), the merged list over cones (blk4x60), a
    dense-C cone (theta30), dense constraints (densea40), an SDP cone beside the LP block (sdplp40: the LP block is passed over by the
    session and refused by the slot)"""
    s, _, _ = _phase2(_path(name))
    try:
        cones = s.solution(tol=0).cones
        sdp = [k for k, c in enumerate(cones) if not c.is_lp]
        F = [cones[k].R for k in sdp]
        if name == "blkmix5":
            assert len({f.shape[1] for f in F}) > 1   # (own ranks differ; the device stores them at a common one)
        lower, upper, minv = _quantile_bounds(F)
        K = 100
        b = s.entry_bounds(max_cuts=K, lower=lower, upper=upper, min_violation=minv)
        assert b.src == UV and len(b.count) == s.nblk and b.passes >= len(sdp)
        assert (b.lower, b.upper, b.min_violation, b.max_cuts) == (lower, upper, minv, K)
        assert np.array_equal(b.bound, np.where(b.cls == 0, lower, upper))
        assert all(b.count[k] == 0 for k in range(s.nblk) if k not in sdp)
        assert set(b.cone.tolist()) <= set(sdp)
        if name == "blk4x60":
            assert len(set(b.cone.tolist())) > 1
        bm.check_against_model(F, lower, upper, minv, K, [int(b.count[k]) for k in sdp], np.searchsorted(sdp, b.cone), b.p, b.q, b.cls,
                               b.violation)
        assert int(b.count.sum()) > K == len(b)
        again = s.entry_bounds(max_cuts=K, lower=lower, upper=upper, min_violation=minv)
        for a in ("count", "cone", "p", "q", "cls", "violation", "bound"):
            assert getattr(again, a).tobytes() == getattr(b, a).tobytes(), a
        assert again.passes == b.passes
        if name == "sdplp40":
            lp = [k for k in range(s.nblk) if k not in sdp]
            assert len(lp) == 1
            assert s.be.entry_bounds(UV, lp[0], lower, upper, minv, 10)[0] == 1
            assert "LP block" in _last_error(s)
    finally:
        s.close()


def test_read_only_and_memory():
    """ADMM steps after a call give the bits they give without it, with a dual update pending at the call; U, V and lambda too; the
    scratch is the context's and goes with it"""
    before = _mem()
    runs = []
    for look in (True, False):
        s, rho, e0 = _phase2(_path("blk4x60"), steps=0)
        try:
            a = s.admm_steps(3, rho, e0)   # (its last dual update still waits for a carrier)
            if look:
                held = _mem()
                c = s.entry_bounds(max_cuts=50, lower=0.0, upper=0.5)
                assert len(c) == 50
                assert _mem()[1] > held[1]   # (the feature's own scratch)
            b = s.admm_steps(3, rho, a[0])
            runs.append((a, b, _state(s)))
        finally:
            s.close()
    (a1, b1, st1), (a2, b2, st2) = runs
    assert a1 == a2 and b1 == b2
    for x, y in zip(st1, st2):
        assert np.array_equal(x, y)
    assert _mem() == before, (before, _mem())


def test_bad_arguments_are_refused():
    """every refusal of the slot but the cone dimension above 2^24 (test_cone_dimension_above_the_limit_is_refused): code 1 and the
    message, before any device work -- no launch, no scratch, the state untouched"""
    s = common.hip_session(_path("theta30"))
    try:
        n, r = s.block_shape(0)
        _load(s, np.random.default_rng(0).standard_normal((n, r)) / np.sqrt(n))
        assert _call(s, 0.0, INF, 1e-3, 0)[0] >= 0   # (the scratch is made)
        st0, held, launches = _state(s), _mem(), s.hip_launch_count()
        be = s.be
        nan = float("nan")
        calls = [
            ("src", lambda: be.entry_bounds(7, 0, 0.0, INF, 1e-3, 10)[0]),
            ("block", lambda: be.entry_bounds(RR, 1, 0.0, INF, 1e-3, 10)[0]),
            ("block", lambda: be.entry_bounds(RR, -1, 0.0, INF, 1e-3, 10)[0]),
            ("max_cuts", lambda: be.entry_bounds(RR, 0, 0.0, INF, 1e-3, -1)[0]),
            ("max_cuts", lambda: be.entry_bounds(RR, 0, 0.0, INF, 1e-3, (1 << 20) + 1)[0]),
            ("min_violation", lambda: be.entry_bounds(RR, 0, 0.0, INF, -1e-3, 10)[0]),
            ("min_violation", lambda: be.entry_bounds(RR, 0, 0.0, INF, nan, 10)[0]),
            ("min_violation", lambda: be.entry_bounds(RR, 0, 0.0, INF, INF, 10)[0]),
            ("NaN", lambda: be.entry_bounds(RR, 0, nan, INF, 1e-3, 10)[0]),
            ("NaN", lambda: be.entry_bounds(RR, 0, 0.0, nan, 1e-3, 10)[0]),
            ("lower is above upper", lambda: be.entry_bounds(RR, 0, 0.5, 0.25, 1e-3, 10)[0]),
            ("both classes are off", lambda: be.entry_bounds(RR, 0, -INF, INF, 1e-3, 10)[0]),
            ("wrong side", lambda: be.entry_bounds(RR, 0, INF, INF, 1e-3, 10)[0]),
            ("wrong side", lambda: be.entry_bounds(RR, 0, -INF, -INF, 1e-3, 10)[0]),
            ("NULL", lambda: be.entry_bounds(RR, 0, 0.0, INF, 1e-3, 10, want_arrays=False)[0]),
        ]
        for what, call in calls:
            assert call() == 1, what
            assert what in _last_error(s), (what, _last_error(s))
            assert _mem() == held, what
            assert s.hip_launch_count() == launches, what
        for x, y in zip(st0, _state(s)):
            assert np.array_equal(x, y)
        assert be.entry_bounds(RR, 0, 0.0, INF, 1e-3, 0, want_arrays=False)[0] == 0   # (counting needs no arrays)
    finally:
        s.close()


def test_cone_dimension_above_the_limit_is_refused(tmp_path):
    """one cone of 2^24 + 1 rows at rank 1 (one entry in C, one constraint X_11 = 1: the file is six lines and the context a few
    vectors of that length): refused before any device work"""
    n = (1 << 24) + 1
    path = str(tmp_path / "big.dat-s")
    with open(path, "w") as f:
        f.write("1\n1\n%d\n1.0\n0 1 1 1 -1.0\n1 1 1 1 1.0\n" % n)
    s = common.hip_session(path, timesLogRank=1e-3)
    try:
        assert s.block_shape(0) == (n, 1)
        held, launches = _mem(), s.hip_launch_count()
        assert s.be.entry_bounds(RR, 0, 0.0, INF, 1e-3, 10)[0] == 1
        assert "cone dimension above 2^24" in _last_error(s)
        assert _mem() == held and s.hip_launch_count() == launches
    finally:
        s.close()


def test_lp_block_and_sharded_refusals():
    s = common.hip_session(_path("sdplp40"))
    try:
        held, launches = _mem(), s.hip_launch_count()
        assert s.be.entry_bounds(RR, 1, 0.0, INF, 1e-3, 10)[0] == 1
        assert "LP block" in _last_error(s)
        assert _mem() == held and s.hip_launch_count() == launches
    finally:
        s.close()
    s = common.hip_session(_path("blk4x60"), world=2, rank=0, separable=True)
    try:
        held, launches = _mem(), s.hip_launch_count()
        assert s.be.entry_bounds(RR, 0, 0.0, INF, 1e-3, 10)[0] == 3
        assert "sharded" in _last_error(s)
        with pytest.raises(NotImplementedError, match="sharded"):
            s.entry_bounds(max_cuts=10)
        assert _mem() == held and s.hip_launch_count() == launches
    finally:
        s.close()


def test_hamming_theta_end_to_end_and_cli(tmp_path):
    """the graph on {0,1}^5 with an edge at Hamming distance 1 or 2, solved, separated with the defaults, written and solved again on
    the device: the list is the model's 16 antipodal pairs and theta = 16/3 becomes theta' = 4; the command line prints the line and
    writes the same file"""
    prob = instances.hamming_theta(5, 2)
    path, tight = str(tmp_path / "ham5.dat-s"), str(tmp_path / "ham5_b.dat-s")
    instances.write_sdpa(prob, path)
    s = common.hip_session(path)
    try:
        r = s.solve()
        b = s.entry_bounds()
        print("hamming theta: pObj %.9f, count %s, kept %d, largest violation %.6f, passes %d"
              % (r["pObj"], b.count, len(b), b.violation[0] if len(b) else 0.0, b.passes))
        assert abs(r["pObj"] + 16.0 / 3.0) <= 2e-4
        F = [c.R for c in s.solution(tol=0).cones]
        bm.check_against_model(F, 0.0, INF, 1e-3, 1000, b.count.tolist(), b.cone, b.p, b.q, b.cls, b.violation)
        assert b.count.tolist() == [16] and len(b) == 16 and (b.cls == 0).all() and (b.bound == 0.0).all()
        assert sorted(zip(b.p.tolist(), b.q.tolist())) == bm.antipodal_pairs(5)
        s.write_bounded(tight, b)
    finally:
        s.close()
    assert read_bounded(tight, prob["m"]) == [(0, int(p), int(q), 0, 0.0) for p, q in zip(b.p, b.q)]
    s2 = common.hip_session(tight, phase2Tol=1e-4)
    try:
        r2 = s2.solve()
    finally:
        s2.close()
    print("hamming theta: bounded pObj %.9f" % r2["pObj"])
    assert abs(r2["pObj"] + 4.0) <= 5e-4, r2["pObj"]
    exe = os.path.join(host.LIB_DIR, "lorads")
    out = tmp_path / "cli.dat-s"
    pr = subprocess.run([exe, path, "--boundsMax", "100", "--boundsFile", str(out)], capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr
    assert "Entry bounds [0, inf] violated by more than 0.001: 16, kept 16, largest violation" in pr.stdout, pr.stdout
    assert "%d passes -> %s" % (b.passes, out) in pr.stdout, pr.stdout
    assert out.read_bytes() == open(tight, "rb").read()
