"""Separation of the triangle inequalities on the GPU (lorads_hip_triangle_cuts, Session.triangle_cuts, Session.write_tightened,
--cutsMax) against the numpy model (tests/triangle_model.py): exact counts, the selection in its total order with any number of
ties, packed indices past 32 bits and a wide rank on planted factors, determinism, read-only continuation, refusals, and the
tightened problem solved on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.cuts import read_tightened
from tests import common
from tests import triangle_model as tm
from tests.test_rounding import _odd_rank_params, _phase2

pytestmark = pytest.mark.gpu

TILE = 32        # CUT_T of csrc/hip/cuts.inc
RR = host.PAIR_RR
GOLDEN = {"maxcut100", "maxcut800", "blk4x60", "theta30", "sdplp40"}


def _path(name):
    if name == "maxcut100odd":
        name = "maxcut100"
    return common.instance_path(name) if name in GOLDEN else common.generated_instance(name)


def _mem():
    d = host.Session.hip_memory_stats()
    return (d["device_allocations"], d["device_bytes"], d["pinned_allocations"], d["pinned_bytes"])


def _last_error(s):
    lib, _ = s._hip()
    lib.lorads_hip_last_error.restype = C.c_char_p
    return lib.lorads_hip_last_error().decode()


def _maxcut_problem(n):
    if n == 1:   # (no edge to draw: the one vertex alone)
        return dict(m=1, blocks=[1], b=np.ones(1), entries=[(0, 1, 1, 1, 0.25), (1, 1, 1, 1, 1.0)])
    return instances.maxcut(n, min(2 * n, n * (n - 1) // 2), 900 + n)


def _maxcut_session(n, r):
    """a Max-Cut context of n vertices (t = 1) at rank r"""
    path = common.generated_instance("cuts_maxcut%d" % n, lambda: _maxcut_problem(n))
    s = common.hip_session(path, timesLogRank=1e-3)   # (the rank rule gives 1; resize_rank grows it to what the case asks for)
    assert s.block_shape(0) == (n, 1)
    if r != 1:
        s.be.resize_rank([r])
    assert s.block_shape(0) == (n, r)
    return s


def _load(s, F):
    common.load_r_state(s.be, [F], np.zeros(s.m))


def _sphere_rows(rng, n, r, t):
    F = rng.standard_normal((n, r))
    return F / np.linalg.norm(F, axis=1)[:, None] * np.asarray(t)[:, None]


def _call(s, minv, K, src=RR, blk=0):
    rc, cnt, p, q, s_, cl, v, passes = s.be.triangle_cuts(src, blk, minv, K)
    assert rc == 0, _last_error(s)
    return cnt, p, q, s_, cl, v, passes


SIZES = [1, 2, 3, 5, TILE - 1, TILE, 63, 64, 2 * TILE + 1, 129, 200]


@pytest.mark.parametrize("r", [6, 5, 1])
@pytest.mark.parametrize("n", SIZES)
def test_synthetic_factors_against_model(n, r):
    """random rows on the sphere of radius t through set_mat, src = RR: an even rank, an odd rank (the device pads a column), r = 1
    (a +-1 point: nothing is violated); max_cuts 0, 1, 100 and more than the count; at two thresholds where the cone is small enough
    for the lower one's count"""
    rng = np.random.default_rng(1000 * n + r)
    t = np.ones(n)
    F = _sphere_rows(rng, n, r, t)
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        for minv in ([1e-3, 0.4] if n <= 2 * TILE + 1 else [0.4]):
            cnt0, *_rest, passes0 = _call(s, minv, 0)
            assert all(len(x) == 0 for x in _rest)
            assert passes0 == (1 if n >= 3 else 0)
            assert cnt0 + 7 <= 1 << 20
            scans = None
            for K in (1, 100, cnt0 + 7):
                cnt, p, q, s_, cl, v, passes = _call(s, minv, K)
                assert cnt == cnt0
                assert passes >= (2 if cnt else passes0)
                scans = tm.check_against_model([(F, t)], minv, K, [cnt], np.zeros(len(p)), p, q, s_, cl, v,
                                               scans=scans or [tm.Scan(F, t, minv, cnt0 + 8)])
                again = _call(s, minv, K)
                assert again[0] == cnt and again[6] == passes
                for a, b in zip(again[1:6], (p, q, s_, cl, v)):
                    assert a.tobytes() == b.tobytes()
            if n < 3 or r == 1:
                assert cnt0 == 0
    finally:
        s.close()


def test_scaled_rows_and_uv_source():
    """t away from 1 (scaledpm1: a_i X_pp = b_i of mixed signs) and src = UV: F = (U + V) / 2 formed on the device"""
    name = "scaledpm1_120"
    prob = instances.NAMED[name]()
    t = tm.t_of(prob)[0]
    s = common.hip_session(_path(name))
    try:
        n, r = s.block_shape(0)
        rng = np.random.default_rng(3)
        F = _sphere_rows(rng, n, r, t)
        D = rng.standard_normal((n, r)) * 0.05
        U, V = F + D, F - D
        common.load_uv_state(s.be, [U], [V], np.zeros(s.m))
        Fd = (s.be.get_mat(host.MAT_U, 0) + s.be.get_mat(host.MAT_V, 0)) / 2
        cnt, p, q, s_, cl, v, _ = _call(s, 0.2, 200, src=host.PAIR_UV)
        assert cnt > 200
        tm.check_against_model([(Fd, t)], 0.2, 200, [cnt], np.zeros(len(p)), p, q, s_, cl, v)
    finally:
        s.close()


def test_massive_ties():
    """three unit vectors at 120 degrees, 32 copies of each: the 32^3 triples with one row of each direction have rho = -1/2 three
    times, v = 1/2 in class 0, the same bits; every other pair has v <= 0.  The cut-off group (32768 equal values, 100 wanted) is
    larger than the buffer: the selection has to tell them apart by their indices."""
    n = 96
    dirs = np.array([[1.0, 0.0], [-0.5, np.sqrt(0.75)], [-0.5, -np.sqrt(0.75)]])
    F = dirs[np.arange(n) % 3]
    t = np.ones(n)
    s = _maxcut_session(n, 2)
    try:
        _load(s, F)
        cnt, p, q, s_, cl, v, passes = _call(s, 0.25, 100)
        print("massive ties: count %d, kept %d, passes %d, v in [%.17g, %.17g]" % (cnt, len(p), passes, v.min(), v.max()))
        assert cnt == 32 ** 3
        assert len(p) == 100 and (cl == 0).all()
        eps = tm.eps_of(F, t, p, q, s_)
        assert np.all(np.abs(v - 0.5) <= eps)
        assert ((p < q) & (q < s_) & (s_ < n)).all()
        assert sorted({int(x) % 3 for x in (p[0], q[0], s_[0])}) == [0, 1, 2]
        assert (tm.order(v, p, q, s_, cl) == np.arange(100)).all()
        if len(set(v.tolist())) == 1:   # equal bits: the first 100 triples of distinct directions in (p, q, s) order
            want = [(a, b, c) for a in range(n) for b in range(a + 1, min(n, a + 8)) for c in range(b + 1, n)
                    if len({a % 3, b % 3, c % 3}) == 3][:100]
            assert list(zip(p.tolist(), q.tolist(), s_.tolist())) == want
        again = _call(s, 0.25, 100)
        assert again[0] == cnt
        for a, b in zip(again[1:6], (p, q, s_, cl, v)):
            assert a.tobytes() == b.tobytes()
    finally:
        s.close()


# ---- past 1024 rows: packed indices ((p n + q) n + s) 4 + class above 2^32, tiles I dealt by the cap of CUT_ITERS = 16 per workgroup, and
# a rank as wide as maxcut20000's.  Planted integer factors (tests/triangle_model.py: plant_rows) make every v exact and give the
# counts in closed form (checked against the full enumeration in test_triangle_model.py), so nothing is enumerated on the host.

BIG_N = 1430


def _deal(n):
    """cut_launch's deal of the tiles I over blockIdx.y restated: (row tiles nt, the cap's term ceil(nt / 16), the small-cone term
    min(nt, ceil(2048 / pairs)), tiles I the longest workgroup walks)"""
    nt = -(-n // TILE)
    npairs = nt * (nt + 1) // 2
    cap, fill = -(-nt // 16), min(nt, -(-2048 // npairs))
    return nt, cap, fill, -(-nt // max(cap, fill))


def _assert_big_deal(n):
    nt, cap, fill, walk = _deal(n)
    assert (nt, n - (nt - 1) * TILE) == (45, 22)     # a ragged last tile of 22 rows
    assert (cap, fill) == (3, 2) and cap > fill      # the cap's term decides the deal, as from n = 1409 on ...
    assert walk == 15                                # ... and a workgroup walks up to 15 tiles I
    assert 4 * n ** 3 > 1 << 32
    assert all(_deal(m)[1] <= _deal(m)[2] for m in SIZES + [800])   # (in every other case the small-cone term decides)


def _packed(n, p, q, s, cl):
    return ((p.astype(np.int64) * n + q) * n + s) * 4 + cl


def _same_bytes(a, b):
    assert a[0] == b[0] and a[6] == b[6]
    for x, y in zip(a[1:6], b[1:6]):
        assert x.tobytes() == y.tobytes()


def test_planted_directions_past_1024_rows():
    """plant A: row p = D[p % 3].  477 477 476 pairs share v = 2, the same bits, and their indices run to 34 bits: the selection closes
    on the index digits of the low word alone"""
    n = BIG_N
    _assert_big_deal(n)
    hi, lo = tm.plant_counts(n)
    assert np.bincount(np.arange(n) % 3).tolist() == [477, 477, 476] and hi == 477 * 477 * 476
    s = _maxcut_session(n, 3)
    try:
        _load(s, tm.plant_rows(n))
        assert _call(s, 1.5, 0)[0] == hi
        assert _call(s, 0.5, 0)[0] == lo
        got = _call(s, 1.5, 100)
        cnt, p, q, s_, cl, v, passes = got
        print("plant A: n %d, count %d above 1.5, %d above 0.5, kept %d, passes %d" % (n, cnt, lo, len(p), passes))
        assert cnt == hi and len(p) == 100
        assert (v == 2.0).all() and (cl == 0).all()
        assert list(zip(p.tolist(), q.tolist(), s_.tolist())) == tm.first_distinct_triples(list(range(n)), 100)
        # no digit above bit 34 tells two keys apart (v's 64 bits and the complement's leading ones): the first pass, seven that
        # cannot narrow (shifts 104 .. 32 of 12 bits each; the last one sees bits 32 and 33), at least the emit
        assert passes >= 9
        _same_bytes(_call(s, 1.5, 100), got)
    finally:
        s.close()


def test_planted_tail_has_every_index_above_2_32():
    """plant B: zero rows but the last 96.  Every kept triple starts at p >= n - 96: its packed index does not fit 32 bits"""
    n, live = BIG_N, 96
    _assert_big_deal(n)
    hi, lo = tm.plant_counts(n, live)
    assert hi == 32 ** 3
    s = _maxcut_session(n, 3)
    try:
        _load(s, tm.plant_rows(n, live))
        assert _call(s, 0.5, 0)[0] == lo
        got = _call(s, 1.5, 100)
        cnt, p, q, s_, cl, v, passes = got
        print("plant B: n %d, count %d, kept %d, passes %d, smallest packed index 2^%.2f" % (n, cnt, len(p), passes,
                                                                                           np.log2(float(_packed(n, p, q, s_, cl).min()))))
        assert cnt == hi and len(p) == 100
        assert (v == 2.0).all() and (cl == 0).all()
        assert (p >= n - live).all() and (_packed(n, p, q, s_, cl) > 1 << 32).all()
        assert list(zip(p.tolist(), q.tolist(), s_.tolist())) == tm.first_distinct_triples(list(range(n - live, n)), 100)
        _same_bytes(_call(s, 1.5, 100), got)
    finally:
        s.close()


def test_scattered_support_past_1024_rows():
    """200 unit rows of rank 6 at scattered positions of 1430, zero rows between them.  A triple with a zero row has two rho = 0 and
    |third| <= 1: v <= 0.  So the list is the 200-row problem's with its rows renumbered -- the positions ascend, so the total order
    carries over -- and its v are the bits the 200-row context gives (a rho depends on its two rows alone)"""
    n, m, r, minv = BIG_N, 200, 6, 0.4
    _assert_big_deal(n)
    rng = np.random.default_rng(1430200)
    fixed = np.array([0, 1023, 1024, 1408, 1429])
    pos = np.sort(np.concatenate([fixed, rng.choice(np.setdiff1d(np.arange(n), fixed), m - len(fixed), replace=False)]))
    assert len(np.unique(pos)) == m and set(fixed.tolist()) <= set(pos.tolist())
    t = np.ones(m)
    Fs = _sphere_rows(rng, m, r, t)
    F = np.zeros((n, r))
    F[pos] = Fs
    back = np.full(n, -1)
    back[pos] = np.arange(m)
    big, small = _maxcut_session(n, r), _maxcut_session(m, r)
    try:
        _load(big, F)
        _load(small, Fs)
        cnt0 = _call(big, minv, 0)[0]
        assert 100 < cnt0 and cnt0 + 7 <= 1 << 20
        scans = None
        for K in (1, 100, cnt0 + 7):
            cnt, p, q, s_, cl, v, passes = _call(big, minv, K)
            assert cnt == cnt0
            mp, mq, ms = back[p], back[q], back[s_]
            assert (mp >= 0).all() and (mq >= 0).all() and (ms >= 0).all()   # no triple with a zero row
            scans = tm.check_against_model([(Fs, t)], minv, K, [cnt], np.zeros(len(p)), mp, mq, ms, cl, v,
                                           scans=scans or [tm.Scan(Fs, t, minv, cnt0 + 8)])
            c2, p2, q2, s2, cl2, v2, _ = _call(small, minv, K)
            assert c2 == cnt and v2.tobytes() == v.tobytes() and cl2.tobytes() == cl.tobytes()
            assert np.array_equal(p2, mp) and np.array_equal(q2, mq) and np.array_equal(s2, ms)
        print("scattered support: count %d, %d of the kept triples reach past row 1024, largest packed index 2^%.2f"
              % (cnt0, int((s_ >= 1024).sum()), np.log2(float(_packed(n, p, q, s_, cl).max()))))
        assert (_packed(n, p, q, s_, cl) > 1 << 32).any() and (p == 0).any() and (s_ == n - 1).any()
    finally:
        big.close()
        small.close()


def test_wide_odd_rank_is_exact_on_integer_rows():
    """rank 41 (padded to 44: 11 steps of the matrix cores, as maxcut20000's rank 40) on rows of integers in [-2, 2]: every product and
    sum is exact, so the count and the kept values are the enumeration's with no tolerance, in the total order"""
    n, r, minv = 200, 41, 50.5   # (v is an integer: none sits on the threshold)
    F = np.random.default_rng(41200).integers(-2, 3, (n, r)).astype(np.float64)
    t = np.ones(n)
    P, Q, S, Cl, V = tm.enumerate_all(F, t)
    assert np.array_equal(V, np.round(V)) and np.abs(V).max() < 2.0 ** 20
    m = V > minv
    o = tm.order(V[m], P[m], Q[m], S[m], Cl[m])
    want = [x[m][o] for x in (P, Q, S, Cl, V)]
    s = _maxcut_session(n, r)
    try:
        assert (r + 3) // 4 == 11
        _load(s, F)
        assert _call(s, minv, 0)[0] == int(m.sum()) > 100
        for K in (100, int(m.sum()) + 7):
            cnt, p, q, s_, cl, v, passes = _call(s, minv, K)
            kept = min(K, int(m.sum()))
            print("wide rank: n %d, r %d, count %d, kept %d, passes %d, v in [%g, %g]" % (n, r, cnt, len(p), passes, v.min(), v.max()))
            assert cnt == int(m.sum()) and len(p) == kept
            assert np.array_equal(v, tm.exact_values(F, t, p, q, s_, cl).astype(np.float64))
            for got, w in zip((p, q, s_, cl, v), want):
                assert np.array_equal(got, w[:kept])
    finally:
        s.close()


def test_pm1_point_has_no_violation():
    n, r = 129, 4
    rng = np.random.default_rng(8)
    sigma = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    f = rng.standard_normal(r)
    f /= np.linalg.norm(f)
    s = _maxcut_session(n, r)
    try:
        _load(s, sigma[:, None] * f[None, :])
        cnt, p, *_ = _call(s, 1e-9, 100)
        assert cnt == 0 and len(p) == 0
    finally:
        s.close()


SOLVED = ["maxcut100", "blk4x60", "blkmix5", "scaledpm1_120", "wmaxcut150", "densemaxcut120", "maxcut100odd", "maxcut800"]


@pytest.mark.parametrize("name", SOLVED)
def test_solved_states_against_model(name):
    """Session.triangle_cuts after phase 1 and three ADMM steps, against the model on the exported factors: per-cone counts and the
    merged order across cones"""
    kw = _odd_rank_params() if name == "maxcut100odd" else {}
    s, _, _ = _phase2(_path(name), **kw)
    try:
        prob_t = tm.t_of(dict(zip(("m", "blocks", "b", "entries"), _read(_path(name)))))
        F = [c.R for c in s.solution(tol=0).cones]
        if name == "maxcut100odd":
            assert F[0].shape[1] % 2 == 1
        K, minv = 300, 1e-3
        cuts = s.triangle_cuts(max_cuts=K, min_violation=minv)
        assert cuts.src == host.PAIR_UV and len(cuts.count) == s.nblk and cuts.passes >= s.nblk
        tm.check_against_model(list(zip(F, prob_t)), minv, K, cuts.count.tolist(), cuts.cone, cuts.p, cuts.q, cuts.s, cuts.cls,
                               cuts.violation)
        again = s.triangle_cuts(max_cuts=K, min_violation=minv)
        for a in ("count", "cone", "p", "q", "s", "cls", "violation"):
            assert getattr(again, a).tobytes() == getattr(cuts, a).tobytes(), a
    finally:
        s.close()


def _read(path):
    from lorads_amd.cuts import read_sdpa
    return read_sdpa(path)


def _state(s):
    mats = [s.be.get_mat(w, k) for k in range(s.nblk) for w in (host.MAT_R, host.MAT_U, host.MAT_V)]
    return mats + [s.be.get_vec(host.VEC_LAMBDA)]


def test_read_only_and_memory():
    """ADMM steps after a call give the bits they give without it; the scratch is the context's and goes with it"""
    before = _mem()
    runs = []
    for look in (True, False):
        s, rho, e0 = _phase2(_path("blk4x60"), steps=0)
        try:
            a = s.admm_steps(3, rho, e0)   # (its last dual update still waits for a carrier)
            if look:
                held = _mem()
                c = s.triangle_cuts(max_cuts=50)
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


@pytest.mark.parametrize("name", ["theta30", "sdplp40"])
def test_not_pm1_structured_is_refused(name):
    s = common.hip_session(_path(name))
    try:
        held = _mem()
        rc = s.be.triangle_cuts(RR, 0, 1e-3, 10)[0]
        assert rc == 2
        assert "not +-1-structured" in _last_error(s)
        with pytest.raises(NotImplementedError, match="not \\+-1-structured"):
            s.triangle_cuts(max_cuts=10)
        assert _mem() == held   # (refused before any scratch was made)
    finally:
        s.close()


def test_bad_arguments_are_refused():
    s = common.hip_session(_path("maxcut100"))
    try:
        _load(s, _sphere_rows(np.random.default_rng(0), *s.block_shape(0), np.ones(100)))
        assert _call(s, 0.4, 0)[0] >= 0   # (the applicability check and the scratch are made)
        st0, held = _state(s), _mem()
        be = s.be
        calls = [
            ("src", lambda: be.triangle_cuts(7, 0, 1e-3, 10)[0]),
            ("block", lambda: be.triangle_cuts(RR, 1, 1e-3, 10)[0]),
            ("block", lambda: be.triangle_cuts(RR, -1, 1e-3, 10)[0]),
            ("max_cuts", lambda: be.triangle_cuts(RR, 0, 1e-3, -1)[0]),
            ("max_cuts", lambda: be.triangle_cuts(RR, 0, 1e-3, (1 << 20) + 1)[0]),
            ("min_violation", lambda: be.triangle_cuts(RR, 0, -1e-3, 10)[0]),
            ("min_violation", lambda: be.triangle_cuts(RR, 0, float("nan"), 10)[0]),
            ("min_violation", lambda: be.triangle_cuts(RR, 0, float("inf"), 10)[0]),
            ("NULL", lambda: be.triangle_cuts(RR, 0, 1e-3, 10, want_arrays=False)[0]),
        ]
        for what, call in calls:
            assert call() == 1, what
            assert what in _last_error(s), (what, _last_error(s))
            assert _mem() == held, what
        for x, y in zip(st0, _state(s)):
            assert np.array_equal(x, y)
        assert be.triangle_cuts(RR, 0, 0.4, 0, want_arrays=False)[0] == 0   # (counting needs no arrays)
    finally:
        s.close()


def test_lp_block_and_sharded_refusals():
    s = common.hip_session(_path("sdplp40"))
    try:
        assert s.be.triangle_cuts(RR, 1, 1e-3, 10)[0] == 1
        assert "LP block" in _last_error(s)
    finally:
        s.close()
    s = common.hip_session(_path("blk4x60"), world=2, rank=0, separable=True)
    try:
        held = _mem()
        assert s.be.triangle_cuts(RR, 0, 1e-3, 10)[0] == 3
        with pytest.raises(NotImplementedError, match="sharded"):
            s.triangle_cuts(max_cuts=10)
        assert _mem() == held
    finally:
        s.close()


def test_c5_end_to_end(tmp_path):
    """the 5-cycle: 10 violated inequalities; with them the relaxation's value is the maximum cut, 4 (untightened: 4.5225)"""
    prob = tm.c5_problem()
    path, tight = str(tmp_path / "c5.dat-s"), str(tmp_path / "c5_tight.dat-s")
    instances.write_sdpa(prob, path)
    s = common.hip_session(path)
    try:
        r = s.solve()
        cuts = s.triangle_cuts(max_cuts=300, min_violation=1e-3)
        print("C5: pObj %.9f, count %s, largest violation %.6f" % (r["pObj"], cuts.count, cuts.violation[0]))
        assert abs(r["pObj"] + 4.52254) <= 1e-4
        assert cuts.count.tolist() == [10] and len(cuts) == 10
        assert abs(cuts.violation[0] - 0.427) <= 2e-3
        s.write_tightened(tight, cuts)
    finally:
        s.close()
    assert read_tightened(tight, 5) == list(zip(cuts.cone.tolist(), cuts.p.tolist(), cuts.q.tolist(), cuts.s.tolist(), cuts.cls.tolist()))
    s2 = common.hip_session(tight)
    try:
        r2 = s2.solve()
    finally:
        s2.close()
    print("C5: tightened pObj %.9f" % r2["pObj"])
    assert abs(r2["pObj"] + 4.0) <= 5 * 1e-5 * 5, r2["pObj"]


def test_maxcut100_end_to_end_and_cli(tmp_path):
    """solve, separate (K = 300, V = 1e-3), write the tightened problem, solve it on the device and by the oracle; the command line
    writes the same file"""
    path, tight = _path("maxcut100"), str(tmp_path / "tight.dat-s")
    s = common.hip_session(path)
    try:
        r = s.solve()
        cuts = s.triangle_cuts(max_cuts=300, min_violation=1e-3)
        assert len(cuts) == 300 and cuts.count[0] > 300
        s.write_tightened(tight, cuts)
    finally:
        s.close()
    s2 = common.hip_session(tight)
    try:
        r2 = s2.solve()
    finally:
        s2.close()
    so = common.oracle_session(tight)
    try:
        ro = so.solve()
    finally:
        so.close()
    p2 = 1e-5
    gap_o = abs(ro["pObj"] - ro["dObj"]) / (1 + abs(ro["pObj"]) + abs(ro["dObj"]))
    tol = max(1e-6, 5 * gap_o)
    print("maxcut100: pObj %.9f, count %d, tightened pObj %.9f (oracle %.9f, gap %.3e), constrVio1 %.3e (oracle %.3e)"
          % (r["pObj"], cuts.count[0], r2["pObj"], ro["pObj"], gap_o, r2["constrVio1"], ro["constrVio1"]))
    assert r2["pObj"] >= r["pObj"] - tol * (1 + abs(r["pObj"]))   # (the feasible set shrank)
    assert abs(r2["pObj"] - ro["pObj"]) <= tol * (1 + abs(ro["pObj"]))
    assert r2["constrVio1"] <= max(2 * ro["constrVio1"], p2)
    # the command line: the same solve, the same separation, the same writer
    exe = os.path.join(host.LIB_DIR, "lorads")
    out = tmp_path / "cli.dat-s"
    pr = subprocess.run([exe, path, "--cutsMax", "300", "--cutsFile", str(out)], capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr
    assert "Triangle inequalities violated by more than 0.001: %d, kept 300" % cuts.count[0] in pr.stdout, pr.stdout
    assert out.read_bytes() == open(tight, "rb").read()
