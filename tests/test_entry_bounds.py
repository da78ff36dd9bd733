"""Separation of entry bounds on the GPU (lorads_hip_entry_bounds, Session.entry_bounds, Session.write_bounded, --boundsMax) against
the numpy model (tests/bounds_model.py): exact counts, the selection in its total order with any number of ties, determinism,
read-only continuation, refusals, the tile groups of the grid's second dimension (n > 512), and the bounded Hamming-graph theta
problem solved on the device."""
import os
import re
import subprocess
import time

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


# ------------------------------------------------------------------ past one tile group
# A workgroup of k_bnd_enum walks at most BND_ITERS tiles J from J0 = I + BND_ITERS blockIdx.y, so from 17 row tiles on (n > 512) the
# grid has a second dimension: J0 of a later group, the early return J0 >= nt and J1 clipped inside a later group.


def _bounds_inc(name):
    text = open(os.path.join(common.ROOT, "lorads_amd", "csrc", "hip", "bounds.inc")).read()
    return int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))


BND_T, BND_ITERS, BND_LDS_COLS = (_bounds_inc(k) for k in ("BND_T", "BND_ITERS", "BND_LDS_COLS"))


def tile_groups(n):
    """(row tiles, the second dimension of bnd_launch's grid), restated"""
    nt = -(-n // BND_T)
    return nt, -(-nt // BND_ITERS)


GROUPS = {512: (16, 1), 513: (17, 2), 545: (18, 2), 1025: (33, 3)}   # 545 and 1025: a ragged last tile of one row


def test_the_restated_groups():
    assert (BND_T, BND_ITERS, BND_LDS_COLS) == (TILE, 16, 128)
    for n, want in GROUPS.items():
        assert tile_groups(n) == want, n


def _far(p, q):
    """the pairs a later group than the first enumerates"""
    return np.asarray(q) // BND_T - np.asarray(p) // BND_T >= BND_ITERS


def _tail_bounds(F, lo=0.01, up=0.995):
    """bounds at the 1 % and 99.5 % quantiles of the off-diagonal entries of X (numpy, from the factor): the count stays in the
    thousands -- about 1.5 % of n (n - 1) / 2 -- and the model's loops stay short.  Where a later group has so few entries that
    none of them may lie that far out (n = 513: the 32 of tile pair (0, 16)), the bound moves in to 0.01 inside the most extreme
    of them (ten times the threshold), so that each class has a violation there (at n = 513 and rank 5 that is a third of the
    pairs, 45186 items with both bounds on: the case still takes 0.2 s)."""
    p, q = np.triu_indices(F.shape[0], 1)
    x = (F @ F.T)[p, q]
    lower, upper = np.quantile(x, [lo, up])
    far = x[_far(p, q)]
    if len(far):
        lower, upper = max(lower, far.min() + 0.01), min(upper, far.max() - 0.01)
    return float(lower), float(upper)


@pytest.mark.parametrize("r", [6, 5])
@pytest.mark.parametrize("n", sorted(GROUPS))
def test_synthetic_factors_against_model_past_one_group(n, r):
    """test_synthetic_factors_against_model's inputs and checks at 16 tiles (still one group), 17, 18 with a ragged last tile and 33
    (three groups, the last of one tile).  Cheap: one context of n <= 1025 rows, one Scan of the model per case (0.14 s at 1025)."""
    t0 = time.perf_counter()
    nt, groups = tile_groups(n)
    assert (nt, groups) == GROUPS[n] and (groups > 1) == (n > 512)
    rng = np.random.default_rng(1000 * n + r)
    F = rng.standard_normal((n, r)) / np.sqrt(r)
    lo, up = _tail_bounds(F)
    minv = 1e-3
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        for lower, upper in [(lo, INF), (-INF, up), (lo, up)]:   # lower only, upper only, both: CASES at these bounds
            cnt0, *_rest, passes0 = _call(s, lower, upper, minv, 0)
            assert all(len(x) == 0 for x in _rest) and passes0 == 1 and cnt0 > 0
            sc = bm.Scan(F, lower, upper, minv)
            far = int(np.count_nonzero(_far(sc.p, sc.q)))
            print("n %d r %d [%g, %g]: count %d, the model has %d, %d of them in later groups" % (n, r, lower, upper, cnt0, len(sc.v), far))
            assert (far > 0) == (groups > 1)   # (without one the case says nothing about the groups)
            for K in (1, 100, cnt0 + 7):
                cnt, p, q, cl, v, passes = _call(s, lower, upper, minv, K)
                assert cnt == cnt0 and passes >= 2
                bm.check_against_model([F], lower, upper, minv, K, [cnt], np.zeros(len(p)), p, q, cl, v, scans=[sc])
                if K > cnt0 and sc.count_hi == sc.count_lo:   # (no item at the threshold: the whole list is the model's,
                    assert int(np.count_nonzero(_far(p, q))) == far   #  every later group's pairs in it)
                if upper == INF:
                    assert (cl == 0).all()
                if lower == -INF:
                    assert (cl == 1).all()
                again = _call(s, lower, upper, minv, K)
                assert again[0] == cnt and again[5] == passes
                for a, b in zip(again[1:5], (p, q, cl, v)):
                    assert a.tobytes() == b.tobytes()
    finally:
        s.close()
    print("n %d r %d: %.2f s" % (n, r, time.perf_counter() - t0))


# rows that share a column of the planted factor, per n; every row of a set carries +-1 in the set's column (the sign is the row's
# parity) and zeros elsewhere, so X_pq = +-1 inside a set and 0 everywhere else, exactly.  Tile distances J - I inside the sets: 15
# (the last tile group 0 walks), 16 (the first of group 1), 31 (the last of group 1 at I = 0) and 32 (group 2, clipped to one tile);
# row n - 1 is alone in the ragged last tile.
PLANTED = {
    1025: [[2, 16 * 32 + 9, 1024],            # tiles 0, 16, 32: distances 16, 32 (group 2, J1 clipped, the ragged tile), 16
           [31, 15 * 32, 30 * 32 + 31],       # tiles 0, 15, 30: 15, 30, 15 at the tiles' first and last rows
           [0, 16 * 32],                      # 16, first rows
           [63, 16 * 32 + 31],                # tiles 1, 16: 15, last rows
           [10, 31 * 32 + 31],                # 31: the last J of group 1
           [37, 17 * 32 + 3],                 # tiles 1, 17: 16
           [100, 20 * 32 + 1]],               # tiles 3, 20: 17
    545: [[3, 544],                           # tiles 0, 17: 17, group 1 clipped to two tiles, the ragged one its last
          [33, 16 * 32 + 31],                 # tiles 1, 16: 15
          [0, 16 * 32],                       # 16
          [31, 15 * 32],                      # 15
          [35, 16 * 32 + 1]],                 # tiles 1, 16: 15
}


def _planted_factor(n, r):
    """(F, the planted pairs).  Columns past the sets' hold one row each (decoys next to the planted rows: X = 0 with everything)."""
    sets = PLANTED[n]
    F = np.zeros((n, r))
    pairs = []
    for c, rows in enumerate(sets):
        for i in rows:
            F[i, c] = -1.0 if i % 2 else 1.0
        pairs += [(a, b) for x, a in enumerate(rows) for b in rows[x + 1:]]
    used = {i for rows in sets for i in rows}
    assert len(used) == sum(len(rows) for rows in sets)
    decoys = [i + d for rows in sets for i in rows for d in (1, -1) if 0 <= i + d < n and i + d not in used]
    for c, i in zip(range(len(sets), r), dict.fromkeys(decoys)):
        F[i, c] = -1.0 if i % 2 else 1.0
    return F, sorted(pairs)


@pytest.mark.parametrize("n", sorted(PLANTED))
def test_planted_violations_in_later_groups_are_exact(n):
    """entries of X that are exactly 0 or +-1 against the bounds [-0.5, 0.5]: the violations are the planted pairs alone, all at
    v = 0.5 exactly, and every one lies in a tile pair with J - I >= 15 -- the count is the planted number and the list the model's
    bit for bit.  Cheap: n <= 1025, a handful of pairs."""
    t0 = time.perf_counter()
    r = 32
    F, pairs = _planted_factor(n, r)
    X = F @ F.T
    assert set(np.unique(X).tolist()) <= {-1.0, 0.0, 1.0}
    assert sorted(zip(*np.nonzero(np.triu(X, 1)))) == pairs   # (the planted pairs and no other)
    dist = sorted({q // BND_T - p // BND_T for p, q in pairs})
    nt, groups = tile_groups(n)
    assert dist[0] == BND_ITERS - 1 and BND_ITERS in dist and any(q == n - 1 for _, q in pairs) and n - 1 == (nt - 1) * BND_T
    assert dist[-1] == nt - 1   # (the last, clipped group)
    planted = {1025: 11, 545: 5}[n]
    assert len(pairs) == planted
    lower, upper, minv = -0.5, 0.5, 0.25
    sc = bm.Scan(F, lower, upper, minv)
    assert len(sc.v) == planted and (sc.v == 0.5).all() and {0, 1} == set(sc.c.tolist())
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        for K in (0, 1, planted + 7):
            cnt, p, q, cl, v, passes = _call(s, lower, upper, minv, K)
            print("planted, n %d, max_cuts %d: count %d, kept %d, passes %d" % (n, K, cnt, len(p), passes))
            assert cnt == planted
            kept = min(K, planted)
            assert np.array_equal(p, sc.p[:kept]) and np.array_equal(q, sc.q[:kept]) and np.array_equal(cl, sc.c[:kept])
            assert v.tobytes() == sc.v[:kept].astype(np.float64).tobytes()
            again = _call(s, lower, upper, minv, K)
            assert again[0] == cnt and again[5] == passes
            for a, b in zip(again[1:5], (p, q, cl, v)):
                assert a.tobytes() == b.tobytes()
    finally:
        s.close()
    print("planted, n %d: %.2f s" % (n, time.perf_counter() - t0))


def test_wide_factor_past_one_group():
    """rl4 = 132 > BND_LDS_COLS at 18 row tiles: the strip-from-memory operands in a second, clipped group and on the ragged tile"""
    t0 = time.perf_counter()
    n, r = 545, 131
    assert tile_groups(n) == (18, 2) and ((r + 3) & ~3) > BND_LDS_COLS
    rng = np.random.default_rng(11)
    F = rng.standard_normal((n, r)) / np.sqrt(r)
    lower, upper = _tail_bounds(F)
    sc = bm.Scan(F, lower, upper, 1e-3)
    far = int(np.count_nonzero(_far(sc.p, sc.q)))
    assert far > 0
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        for K in (0, 100, len(sc.v) + 7):
            cnt, p, q, cl, v, _ = _call(s, lower, upper, 1e-3, K)
            bm.check_against_model([F], lower, upper, 1e-3, K, [cnt], np.zeros(len(p)), p, q, cl, v, scans=[sc])
        assert cnt > 100 and (sc.count_hi != sc.count_lo or int(np.count_nonzero(_far(p, q))) == far)
    finally:
        s.close()
    print("wide factor, n %d r %d: count %d, %d in the later group; %.2f s" % (n, r, cnt, far, time.perf_counter() - t0))


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
