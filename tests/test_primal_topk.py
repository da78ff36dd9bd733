"""The k best entries per row of the primal on the GPU (lorads_hip_primal_topk, Session.primal_topk, --topkFile) against the numpy
model (tests/topk_model.py): the total order with ties and zeros of either sign, NaN rows, windows that cut tiles, the prune of a full
row buffer, the merge of a split window, batches, determinism, read-only continuation, refusals and the command line."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, topk
from tests import common
from tests import topk_model as tm
from tests.admm_model import read_sdpa
from tests.test_primal import _path
from tests.test_rounding import _phase2
from tests.test_triangle_cuts import _last_error, _load, _maxcut_session, _mem, _state

pytestmark = pytest.mark.gpu

# the constants of csrc/hip/topk.inc
T = 16            # TOPK_T: query rows of a tile
STEP = 64         # TOPK_STEP: columns of a step
W = 128           # TOPK_MINSTEPS * TOPK_STEP: the columns a run has at least; a window is split only into runs that long
LDS_COLS = 112    # TOPK_LDS_COLS: the query strip sits in LDS up to this many padded columns
MAXRUNS = 32      # TOPK_MAXRUNS: the runs of a window at most
BATCH = 16384     # TOPK_BATCH: queries of a batch; at this many nothing is split on a card of up to 512 CUs
KMAX = 128


def cap(k):
    """topk_cap: the row buffer's capacity B"""
    return 128 if k <= 32 else 256


RR, UV = host.PAIR_RR, host.PAIR_UV


def _csr(skip):
    if skip is None:
        return None, None
    ptr = np.zeros(len(skip) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in skip])
    col = np.concatenate([np.asarray(x, dtype=np.int32) for x in skip]) if len(skip) else np.zeros(0, dtype=np.int32)
    return ptr, col.astype(np.int32)


def _call(s, rows, lo, hi, k, smallest=False, diag=False, skip=None, src=RR, blk=0):
    ptr, col = _csr(skip)
    rc, idx, val, found = s.be.primal_topk(src, blk, rows, lo, hi, k, int(smallest), int(diag), ptr, col)
    assert rc == 0, _last_error(s)
    return idx, val, found


def _twice(s, *a, **kw):
    """a call, run twice: the same bytes"""
    one, two = _call(s, *a, **kw), _call(s, *a, **kw)
    for x, y in zip(one, two):
        assert x.tobytes() == y.tobytes()
    return one


def _skip_lists(rng, rows, n):
    """per query: duplicates, the row itself, columns outside any proper window (0 and n - 1), and every third query nothing"""
    out = []
    for i, p in enumerate(rows):
        if i % 3 == 2:
            out.append([])
            continue
        c = rng.integers(0, n, size=min(n, 5)).tolist()
        out.append(c + c[:2] + [int(p), 0, n - 1])
    return out


SIZES = [1, 2, 3, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 129, 200]


@pytest.mark.parametrize("r", [6, 5, 1])
@pytest.mark.parametrize("n", SIZES)
def test_synthetic_factors_against_model(n, r):
    """random rows through set_mat, src = RR: an even rank, an odd rank (the device pads), r = 1; k 1, 5, 32, 128 (above n too); the
    full window, one that cuts tiles at both ends, one column, none; one query, T + 1, all rows in reverse with three duplicates;
    both orders, with and without the diagonal, with and without skip lists (the eight combinations go round over the 48 cases)"""
    rng = np.random.default_rng(1000 * n + r)
    F = rng.standard_normal((n, r)) / np.sqrt(r)
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        windows = [(0, n), (n // 3, max(n - 1, n // 3)), (n // 2, n // 2 + 1), (n // 2, n // 2)]
        queries = [[n // 2], rng.integers(0, n, size=T + 1).tolist(), list(range(n))[::-1] + [0, n // 2, n - 1]]
        for c, (k, (lo, hi), rows) in enumerate(itertools.product([1, 5, 32, 128], windows, queries)):
            smallest, diag, skip = bool(c & 1), bool(c & 2), (_skip_lists(rng, rows, n) if c & 4 else None)
            idx, val, found = _twice(s, rows, lo, hi, k, smallest, diag, skip)
            tm.check_against_model(F, rows, lo, hi, k, smallest, diag, skip, idx, val, found, "n %d r %d case %d" % (n, r, c))
            if lo == hi:
                assert (found == 0).all()
            if rows is queries[2] and skip is None:   # (the three duplicates at the end: rows 0, n // 2, n - 1)
                for j, p in enumerate([0, n // 2, n - 1]):
                    i = n - 1 - p
                    assert idx[i].tobytes() == idx[n + j].tobytes() and val[i].tobytes() == val[n + j].tobytes()
        if n == 1:
            assert _call(s, [0], 0, 1, 5)[2].tolist() == [0] and _call(s, [0], 0, 1, 5, diag=True)[2].tolist() == [1]
    finally:
        s.close()


def _exact(s, F, rows, lo, hi, k, smallest=False, diag=False, skip=None):
    idx, val, found = _twice(s, rows, lo, hi, k, smallest, diag, skip)
    midx, mval, mfound = tm.model_topk(F, rows, lo, hi, k, smallest, diag, skip)
    assert np.array_equal(found, mfound)
    assert np.array_equal(idx, midx), (idx[:2], midx[:2])
    assert np.array_equal(val, mval)
    assert not np.signbit(val).any() or (val[np.signbit(val)] != 0).all()
    return idx, val, found


@pytest.mark.parametrize("smallest", [False, True])
def test_exact_small_integers(smallest):
    """integers in [-3, 3]: every chain is exact in any order, many ties and many exact zeros: equal to the model"""
    n, r = 129, 5
    rng = np.random.default_rng(11)
    F = rng.integers(-3, 4, size=(n, r)).astype(np.float64)
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        rows = list(range(n)) + [5, 5]
        for k in (1, 5, 32, 128):
            for lo, hi in ((0, n), (n // 3, n - 1)):
                _exact(s, F, rows, lo, hi, k, smallest, diag=(k == 5), skip=_skip_lists(rng, rows, n) if k == 32 else None)
    finally:
        s.close()


def test_exact_all_rows_equal():
    """all rows equal: every candidate ties, idx is the first k admissible columns"""
    n, r = 200, 2
    F = np.tile(np.array([[3.0, 4.0]]), (n, 1))
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        rows = [0, 7, 199, 64]
        skip = [[1, 2], [], [0, 0, 198], [63, 65, 66]]
        for smallest in (False, True):
            for k in (5, 128):
                idx, val, found = _exact(s, F, rows, 3, n, k, smallest, False, skip)
                for i, p in enumerate(rows):
                    want = [q for q in range(3, n) if q != p and q not in skip[i]][:k]
                    assert idx[i, :found[i]].tolist() == want
                assert (val[:, 0] == 25.0).all()
    finally:
        s.close()


def test_exact_orthogonal_signed_unit_rows():
    """F = diag(+-1) with zeros of either sign off the diagonal: X_pq = 0 (p != q) however the signs fall, so both orders list the
    columns ascending; with the diagonal X_pp = 1 comes first, or last"""
    n = 12
    sign = np.where(np.arange(n) % 3 == 1, -1.0, 1.0)
    F = np.diag(sign)
    F[F == 0] = np.where(np.add.outer(np.arange(n), np.arange(n)) % 2 == 0, 0.0, -0.0)[F == 0]
    assert np.signbit(F).sum() > n
    s = _maxcut_session(n, n)
    try:
        _load(s, F)
        rows = list(range(n))
        for smallest in (False, True):
            idx, val, found = _exact(s, F, rows, 0, n, n, smallest)
            for p in rows:
                assert idx[p].tolist() == [q for q in range(n) if q != p] + [-1]
            assert (val == 0).all() and not np.signbit(val).any()
            idx, val, found = _exact(s, F, rows, 0, n, n, smallest, diag=True)
            for p in rows:
                others = [q for q in range(n) if q != p]
                assert idx[p].tolist() == (others + [p] if smallest else [p] + others)
    finally:
        s.close()


@pytest.mark.parametrize("k", [5, 128])
def test_exact_monotone_rows_prune_repeatedly(k):
    """F_q = q e_1, the query row e_1: X increases along the columns over more than 3 B candidates, so every candidate beats the
    threshold, enters the buffer, and the prune runs again and again; decreasing (the other order on the same factor), nothing
    enters after the first k.  Exact in any order."""
    n = 3 * cap(k) + 2 * STEP + 7
    assert n - 1 > 3 * cap(k)
    F = np.arange(n, dtype=np.float64)[:, None]
    s = _maxcut_session(n, 1)
    try:
        _load(s, F)
        idx, val, found = _exact(s, F, [1, 1, 2], 0, n, k)                     # increasing: the best are the last columns
        assert idx[0].tolist() == list(range(n - 1, n - 1 - k, -1))
        assert val[2].tolist() == [2.0 * q for q in range(n - 1, n - 1 - k, -1)]
        idx, val, found = _exact(s, F, [1, 1, 2], 0, n, k, smallest=True)      # decreasing: the best are the first columns
        assert idx[0].tolist() == [q for q in range(k + 1) if q != 1]
        _exact(s, F, [1], 5, n - 3, k, skip=[list(range(n - 40, n, 2))])
    finally:
        s.close()


def test_split_and_merge_equal_one_workgroup():
    """three queries over 3 W + 5 columns: the window is split into runs and merged.  The best candidates are planted in different
    runs and on their edges.  The same rows among 16384 queries -- where one workgroup walks the whole window -- give the same bytes."""
    n, r, k = 3 * W + 5, 4, 8
    rng = np.random.default_rng(5)
    F = rng.standard_normal((n, r)) / 8
    rows = [10, 200, 388]
    planted = [0, STEP - 1, STEP, W - 1, W, 2 * W - 1, 2 * W, 3 * W - 1, 3 * W, n - 1, 191, 192, 383, 384]
    for j, q in enumerate(planted):
        F[q] = (3 + j / 16) * F[rows[j % 3]]
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        for smallest, diag in ((False, False), (True, True)):
            skip = [[planted[0]], [], [planted[3], 5]]
            idx, val, found = _twice(s, rows, 0, n, k, smallest, diag, skip)
            tm.check_against_model(F, rows, 0, n, k, smallest, diag, skip, idx, val, found, "split")
            many = rows + rng.integers(0, n, size=BATCH - 3).tolist()
            big = _call(s, many, 0, n, k, smallest, diag, skip + [[]] * (BATCH - 3))
            for a, b in zip((idx, val, found), big):
                assert a.tobytes() == b[:3].tobytes()
            pick = list(range(3, BATCH, 1021))
            tm.check_against_model(F, [many[i] for i in pick], 0, n, k, smallest, diag, None, big[0][pick], big[1][pick], big[2][pick],
                                   "one workgroup per tile")
    finally:
        s.close()


@pytest.mark.parametrize("k", [8, 100])
def test_many_runs_merge_in_several_passes(k):
    """three queries over 70 steps: the most runs a window is cut into (24 here, of 3 steps; MAXRUNS caps them), more than the merge
    takes in one pass -- (B - k) / k = 15 at k = 8, one at k = 100 -- with the best candidates spread over the runs, short lists in
    the runs a skip list empties, both orders"""
    n, r = 70 * STEP + 5, 4
    assert min(2 * 256, (n + STEP - 1) // STEP // 2, MAXRUNS) == MAXRUNS and cap(k) - k < 24 * k
    rng = np.random.default_rng(21 + k)
    F = rng.standard_normal((n, r)) / 8
    rows = [3, 2000, n - 1]
    for j, q in enumerate(range(7, n, 151)):
        F[q] = (3 + j / 64) * F[rows[j % 3]]
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        skip = [list(range(3 * STEP, 9 * STEP)), [], list(range(n - 2 * STEP, n))]   # (whole runs without a candidate)
        for smallest in (False, True):
            idx, val, found = _twice(s, rows, 0, n, k, smallest, False, skip)
            tm.check_against_model(F, rows, 0, n, k, smallest, False, skip, idx, val, found, "many runs, k %d" % k)
    finally:
        s.close()


def test_more_queries_than_a_batch():
    """BATCH + 5 queries with skip lists: the second batch reads its own part of the lists"""
    n, r, k = 40, 3, 3
    rng = np.random.default_rng(8)
    F = rng.standard_normal((n, r))
    rows = (list(range(n)) * (BATCH // n + 1))[:BATCH + 5]
    skip = [[(p + 1 + i // n) % n] for i, p in enumerate(rows)]
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        idx, val, found = _call(s, rows, 0, n, k, skip=skip)
        pick = list(range(0, BATCH, 997)) + list(range(BATCH - 2, BATCH + 5))
        tm.check_against_model(F, [rows[i] for i in pick], 0, n, k, False, False, [skip[i] for i in pick], idx[pick], val[pick], found[pick],
                               "batches")
        assert (found == k).all()
    finally:
        s.close()


@pytest.mark.parametrize("r", [LDS_COLS, LDS_COLS + 1, 131])
def test_wide_factor(r):
    """the widest factor whose query strip sits in LDS, and ranks above it: the strip is read through the caches"""
    n = 70
    rng = np.random.default_rng(r)
    F = rng.standard_normal((n, r)) / np.sqrt(r)
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        rows = list(range(n))[::-1]
        for k, smallest in ((5, False), (128, True)):
            idx, val, found = _twice(s, rows, 2, n - 1, k, smallest)
            tm.check_against_model(F, rows, 2, n - 1, k, smallest, False, None, idx, val, found, "r %d" % r)
    finally:
        s.close()


def test_nan_row_is_passed_over():
    n, r, bad = 40, 6, 7
    rng = np.random.default_rng(2)
    F = rng.standard_normal((n, r))
    F[bad, 2] = np.nan
    s = _maxcut_session(n, r)
    try:
        _load(s, F)
        rows = list(range(n))
        for smallest, diag in ((False, False), (True, True)):
            idx, val, found = _twice(s, rows, 0, n, 128, smallest, diag)
            assert found[bad] == 0 and (idx[bad] == -1).all() and (val[bad] == 0).all()
            assert bad not in idx
            assert all(found[p] == n - 1 - (0 if diag else 1) for p in rows if p != bad)
            tm.check_against_model(F, rows, 0, n, 128, smallest, diag, None, idx, val, found, "nan")
    finally:
        s.close()


def _observed(path, n):
    """per row of cone 0 the columns at which some constraint matrix stores an entry (either triangle)"""
    _, _, _, ent = read_sdpa(path)
    obs = [set() for _ in range(n)]
    for mat, blk, i, j, _ in ent:
        if mat > 0 and blk == 1:
            obs[i - 1].add(j - 1)
            obs[j - 1].add(i - 1)
    return obs


@pytest.mark.parametrize("name", ["matcomp60", "blkmix5", "densea40", "theta30", "sdplp40"])
def test_solved_states_against_model(name):
    """after phase 1 and three ADMM steps: Session.primal_topk (src = UV: F = (U + V) / 2 formed on the device) and the slot at
    src = RR against the model on the factors read back with get_mat"""
    path = _path(name)
    s, _, _ = _phase2(path)
    try:
        lp = s._lp_blocks()
        sdp = [k for k in range(s.nblk) if not lp[k]]
        if name == "blkmix5":
            assert len({s.block_shape(k)[1] for k in sdp}) > 1   # (own ranks differ; the device stores them at a common one)
        if name == "sdplp40":
            assert sdp == [0] and len(lp) == 2
        for blk in sdp:
            n = s.block_shape(blk)[0]
            Fuv = (s.be.get_mat(host.MAT_U, blk) + s.be.get_mat(host.MAT_V, blk)) / 2
            Frr = s.be.get_mat(host.MAT_R, blk)
            rows = list(range(n))[::-1]
            for k, smallest in ((5, False), (n, True)):
                k = min(k, KMAX)
                idx, val, found = s.primal_topk(blk, rows, k, smallest=smallest)
                tm.check_against_model(Fuv, rows, 0, n, k, smallest, False, None, idx, val, found, "%s cone %d uv" % (name, blk))
                again = s.primal_topk(blk, rows, k, smallest=smallest)
                for a, b in zip(again, (idx, val, found)):
                    assert a.tobytes() == b.tobytes()
                idx, val, found = _call(s, rows, n // 4, n, k, smallest, True, src=RR, blk=blk)
                tm.check_against_model(Frr, rows, n // 4, n, k, smallest, True, None, idx, val, found, "%s cone %d rr" % (name, blk))
        if name == "matcomp60":
            n = s.block_shape(0)[0]
            obs = _observed(path, n)
            assert sum(len(o) for o in obs) == 400
            rows = list(range(30))
            own = [[p + 30, 59] for p in rows]
            F = (s.be.get_mat(host.MAT_U, 0) + s.be.get_mat(host.MAT_V, 0)) / 2
            idx, val, found = s.primal_topk(0, rows, 10, cols=(30, 60), skip=own, skip_constrained=True)
            both = [sorted(obs[p] | set(own[i])) for i, p in enumerate(rows)]
            tm.check_against_model(F, rows, 30, 60, 10, False, False, both, idx, val, found, "matcomp60, the free item columns")
            pair = s.primal_topk(0, rows, 10, cols=(30, 60), skip=_csr(own), skip_constrained=True)
            for a, b in zip(pair, (idx, val, found)):
                assert a.tobytes() == b.tobytes()
            same = 0
            for i, p in enumerate(rows):
                f = found[i]
                assert f == min(10, 30 - len([q for q in both[i] if q >= 30]))
                assert not (set(idx[i, :f].tolist()) & obs[p])
                ent = s.primal_entries(0, np.full(f, p), idx[i, :f])[0]
                assert (np.abs(ent - val[i, :f]) <= tm.eps_of(F, p, idx[i, :f].astype(np.int64))).all()
                same += int(np.count_nonzero(ent.view(np.int64) == val[i, :f].view(np.int64)))
            print("matcomp60: %d of %d listed values have the bits primal_entries gives" % (same, int(found.sum())))
    finally:
        s.close()


def test_read_only_and_memory():
    """ADMM steps after a call give the bits they give without it, with a dual update pending at the call; U, V and lambda too; the
    scratch is the context's and goes with it; a second call at the same sizes allocates nothing"""
    before = _mem()
    runs = []
    for look in (True, False):
        s, rho, e0 = _phase2(_path("blk4x60"), steps=0)
        try:
            a = s.admm_steps(3, rho, e0)   # (its last dual update still waits for a carrier)
            if look:
                held = _mem()
                one = s.primal_topk(1, [3, 5, 59], 7, skip=[[1], [], [2, 2]])
                assert (one[2] == 7).all()
                mine = _mem()
                assert mine[1] > held[1]   # (the feature's own scratch)
                two = s.primal_topk(1, [5, 3, 0], 7, skip=[[], [9], [4, 4]])
                assert _mem() == mine
                assert one[0][0].tobytes() != two[0][0].tobytes()
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
    """every refusal of the slot with code 1 and its own message, before any device work -- no launch, no scratch, the state
    untouched -- and Session.primal_topk's ValueError in the same words"""
    s = common.hip_session(_path("theta30"))
    try:
        n, r = s.block_shape(0)
        _load(s, np.random.default_rng(0).standard_normal((n, r)) / np.sqrt(n))
        assert (_call(s, [0, 1], 0, n, 3, skip=[[1], []])[2] == 3).all()   # (the scratch is made)
        st0, held, launches = _state(s), _mem(), s.hip_launch_count()
        be = s.be
        one = np.array([0, 1], dtype=np.int64)
        calls = [
            ("src 7 is neither", lambda: be.primal_topk(7, 0, [0], 0, n, 3)),
            ("block 1 is outside", lambda: be.primal_topk(RR, 1, [0], 0, n, 3)),
            ("block -1 is outside", lambda: be.primal_topk(RR, -1, [0], 0, n, 3)),
            ("nq -1 is negative", lambda: be.primal_topk(RR, 0, [0], 0, n, 3, nq=-1)),
            ("row must not be NULL", lambda: be.primal_topk(RR, 0, None, 0, n, 3, nq=1)),
            ("row %d is outside" % n, lambda: be.primal_topk(RR, 0, [0, n], 0, n, 3)),
            ("row -1 is outside", lambda: be.primal_topk(RR, 0, [-1], 0, n, 3)),
            ("window [-1, ", lambda: be.primal_topk(RR, 0, [0], -1, n, 3)),
            ("window [0, %d)" % (n + 1), lambda: be.primal_topk(RR, 0, [0], 0, n + 1, 3)),
            ("window [5, 4)", lambda: be.primal_topk(RR, 0, [0], 5, 4, 3)),
            ("k 0 is outside [1, 128]", lambda: be.primal_topk(RR, 0, [0], 0, n, 0)),
            ("k 129 is outside [1, 128]", lambda: be.primal_topk(RR, 0, [0], 0, n, 129)),
            ("smallest 2 is neither", lambda: be.primal_topk(RR, 0, [0], 0, n, 3, smallest=2)),
            ("include_diag -1 is neither", lambda: be.primal_topk(RR, 0, [0], 0, n, 3, include_diag=-1)),
            ("both or neither", lambda: be.primal_topk(RR, 0, [0], 0, n, 3, skip_ptr=one)),
            ("both or neither", lambda: be.primal_topk(RR, 0, [0], 0, n, 3, skip_col=[1])),
            ("does not start at 0", lambda: be.primal_topk(RR, 0, [0], 0, n, 3, skip_ptr=[1, 1], skip_col=[1])),
            ("decreases at query 1", lambda: be.primal_topk(RR, 0, [0, 1], 0, n, 3, skip_ptr=[0, 1, 0], skip_col=[1])),
            ("skip column %d" % n, lambda: be.primal_topk(RR, 0, [0], 0, n, 3, skip_ptr=[0, 2], skip_col=[1, n])),
            ("skip column -1", lambda: be.primal_topk(RR, 0, [0], 0, n, 3, skip_ptr=[0, 1], skip_col=[-1])),
            ("idx, val and found must not be NULL", lambda: be.primal_topk(RR, 0, [0], 0, n, 3, want_arrays=False)),
        ]
        for what, call in calls:
            assert call()[0] == 1, what
            assert _last_error(s).startswith("primal_topk: ") and what in _last_error(s), (what, _last_error(s))
            assert _mem() == held, what
            assert s.hip_launch_count() == launches, what
        lib, _ = s._hip()
        assert lib.lorads_hip_primal_topk(None, RR, 0, 0, None, 0, 0, 1, 0, 0, None, None, None, None, None) == 1
        assert "no context" in _last_error(s)
        for kw, what in ((dict(k=0), "k 0 is outside"), (dict(k=3, cols=(4, 2)), "window"), (dict(k=3, skip=[[n]]), "skip column")):
            with pytest.raises(ValueError, match="primal_topk: .*" + what):
                s.primal_topk(0, [0], **kw)
        with pytest.raises(ValueError, match="one list per query"):
            s.primal_topk(0, [0, 1], 3, skip=[[1]])
        assert _mem() == held and s.hip_launch_count() == launches
        for x, y in zip(st0, _state(s)):
            assert np.array_equal(x, y)
        # calls that do no device work: no query, an empty window
        rc, idx, val, found = be.primal_topk(RR, 0, None, 0, n, 3, nq=0, want_arrays=False)
        assert rc == 0 and len(found) == 0
        idx, val, found = _call(s, [0, 1], 4, 4, 3)
        assert (found == 0).all() and (idx == -1).all() and (val == 0).all()
        assert _mem() == held and s.hip_launch_count() == launches
    finally:
        s.close()


def test_lp_block_and_sharded_refusals():
    s = common.hip_session(_path("sdplp40"))
    try:
        held, launches = _mem(), s.hip_launch_count()
        assert s.be.primal_topk(RR, 1, [0], 0, 1, 3)[0] == 2
        assert "LP block" in _last_error(s)
        assert _mem() == held and s.hip_launch_count() == launches
    finally:
        s.close()
    s = common.hip_session(_path("blk4x60"), world=2, rank=0, separable=True)
    try:
        held, launches = _mem(), s.hip_launch_count()
        assert s.be.primal_topk(RR, 0, [0], 0, 60, 3)[0] == 3
        assert "sharded" in _last_error(s)
        assert _mem() == held and s.hip_launch_count() == launches
    finally:
        s.close()


def test_cli_end_to_end(tmp_path):
    """matcomp60 solved by the command line and by a session: the output file holds Session.primal_topk's bits"""
    path = _path("matcomp60")
    exe = os.path.join(host.LIB_DIR, "lorads")
    qf, of = tmp_path / "q.txt", tmp_path / "o.txt"
    rows = [5, 1, 30, 1, 12]
    lo, hi = [31, 31, 1, 31, 1], [60, 60, 60, 60, 30]          # (1-based, inclusive)
    skip = [[], [31, 45], [], [31, 45], [2]]
    topk.write_queries(qf, [1] * 5, rows, lo, hi, skip)
    k = 6
    pr = subprocess.run([exe, path, "--topkFile", str(qf), "--topkCount", str(k), "--topkOut", str(of), "--topkSkipConstrained", "--topkSmallest"],
                        capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr
    assert "Top-k entries per row of the primal X (%s): 5 queries, k %d, " % (qf, k) in pr.stdout and "-> %s" % of in pr.stdout, pr.stdout
    got = topk.read_topk(of)
    assert (got.count, got.k, got.src, got.order) == (5, k, "uv", "smallest")
    assert got.row.tolist() == rows and got.blk.tolist() == [1] * 5
    s = common.hip_session(path)
    try:
        s.solve()
        for e in range(5):
            idx, val, found = s.primal_topk(0, [rows[e] - 1], k, cols=(lo[e] - 1, hi[e]), smallest=True, skip=[[c - 1 for c in skip[e]]],
                                            skip_constrained=True)
            assert got.found[e] == found[0] > 0
            assert (got.idx[e] - 1).tolist() == idx[0].tolist()
            assert got.val[e].tobytes() == val[0].tobytes()
        assert got.idx[1].tolist() == got.idx[3].tolist()
    finally:
        s.close()
    # the default output name; refusals before the solve
    pr = subprocess.run([exe, path, "--topkFile", str(qf), "--topkCount", "2"], capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0 and os.path.exists(str(qf) + ".out"), pr.stderr
    assert topk.read_topk(str(qf) + ".out").order == "largest"
    for args, say in ((["--topkCount", "3"], "needs --topkFile"), (["--topkFile", str(qf), "--topkCount", "0"], "bad value 0")):
        pr = subprocess.run([exe, path] + args, capture_output=True, text=True, timeout=120)
        assert pr.returncode == 2 and say in pr.stderr and "End Program" not in pr.stdout
