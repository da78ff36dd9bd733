"""Entries of the primal X = F F^T and its products with a block of vectors on the GPU (DESIGN.md section 13;
lorads_amd/csrc/hip/primal.inc) against numpy in np.longdouble on the read-back factors.

u = 2^-53.  F is numpy's (U + V) / 2 or R of the read-back factors (the average is the same bits on both sides).
  entries     |val - F_i . F_j| <= 2 rl u sum_c |F_ic F_jc|                      (the dot-product bound gamma_rl, any order, FMA included)
  apply       |T - F^T B| <= 2 n u (|F^T| |B|),  |Y - F (F^T B)| <= 2 (n + rl) u (|F| |F^T| |B|), elementwise
  statistics  stats[2] bit-equal to max |val - ref|; stats[0], [1], [3] within 2 (count + 4) u of their own value
The longdouble references carry 2^-64: below 2^-10 of the bounds.  Every test prints the worst achieved ratio to its bound.
The size splits of primal_apply (row strips past 256 rows, row panels past 65536) have cases of their own at the end of the file, on
integer data and exact."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

from lorads_amd import host, instances, primal
from lorads_amd.solution import read_solution
from tests import common
from tests.admm_model import read_sdpa
from tests.test_triangle_cuts import _maxcut_session

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
GOLDEN = {os.path.basename(f)[:-6] for f in os.listdir(common.GOLD) if f.endswith(".dat-s")}


def _consts():
    text = open(os.path.join(common.ROOT, "include", "lorads_hip.h")).read()
    return tuple(int(re.search(r"#define\s+%s\s+(\d+)" % k, text).group(1)) for k in ("LORADS_HIP_PRIMAL_CHUNK", "LORADS_HIP_PRIMAL_EPW"))


CHUNK, EPW = _consts()


def _path(name):
    return common.instance_path(name) if name in GOLDEN else common.generated_instance(name)


def _factor(s, k, src):
    if src == host.PAIR_UV:
        return (s.be.get_mat(host.MAT_U, k) + s.be.get_mat(host.MAT_V, k)) / 2
    return s.be.get_mat(host.MAT_R, k)


def _mem():
    d = host.Session.hip_memory_stats()
    return (d["device_allocations"], d["device_bytes"], d["pinned_allocations"], d["pinned_bytes"])


def _state(s):
    mats = [s.be.get_mat(w, k) for w in (host.MAT_R, host.MAT_U, host.MAT_V) for k in range(s.nblk)]
    return mats + [s.be.get_vec(host.VEC_LAMBDA)]


def _last_error(s):
    lib, _ = s._hip()
    lib.lorads_hip_last_error.restype = C.c_char_p
    return lib.lorads_hip_last_error().decode()


def entry_reference(F, rows, cols, is_lp):
    """(want, bound) of the positions in longdouble"""
    Fl = F.astype(LD)
    rl = F.shape[1]
    if is_lp:
        d = (Fl[rows, 0] * Fl[cols, 0]) * (rows == cols)
        return d, 2 * U * np.abs(d)
    prod = Fl[rows] * Fl[cols]
    return prod.sum(axis=1), 2 * rl * U * np.abs(prod).sum(axis=1)


def check_entries(val, F, rows, cols, is_lp, tag):
    want, bound = entry_reference(F, rows, cols, is_lp)
    err = np.abs(val.astype(LD) - want)
    tiny = float(np.finfo(float).tiny)
    ratio = float(np.max(err / np.maximum(bound, tiny))) if len(val) else 0.0
    print("%s: %d entries, rl %d, max |dval| %.2e, worst ratio to the bound %.3f" % (tag, len(val), F.shape[1], float(err.max()) if len(val) else 0.0, ratio))
    assert np.all(err <= bound), (tag, ratio)
    return ratio


def check_stats(st, val, ref, tag):
    d = val.astype(LD) - ref.astype(LD)
    want = [np.sum(d * d), np.sum(np.abs(d)), None, np.sum(ref.astype(LD) ** 2)]
    tol = 2 * (len(val) + 4) * U
    assert st[2] == (np.max(np.abs(val - ref)) if len(val) else 0.0), tag
    worst = 0.0
    for i in (0, 1, 3):
        e = abs(LD(st[i]) - want[i])
        b = tol * want[i]
        assert e <= b, (tag, i, float(e), float(b))
        worst = max(worst, float(e / b) if b > 0 else 0.0)
    print("%s: statistics of %d entries, worst ratio to the bound %.4f" % (tag, len(val), worst))
    return worst


def all_positions(s, src, tag, session_too=False):
    """test 1's body on the session's current state: every cone, all n^2 positions in shuffled order.  Returns X per block."""
    lp = s._lp_blocks()
    out = []
    for k in range(s.nblk):
        F = _factor(s, k, src)
        n = F.shape[0]
        rng = np.random.default_rng(1000 + k)
        pos = rng.permutation(n * n)
        rows, cols = (pos // n).astype(np.int32), (pos % n).astype(np.int32)
        rc, val, st = s.be.primal_entries(src, k, rows, cols)
        assert rc == 0 and st is None
        check_entries(val, F, rows, cols, lp[k], "%s block %d" % (tag, k))
        X = np.zeros((n, n))
        X[rows, cols] = val
        assert np.array_equal(X, X.T), (tag, k)       # val(i, j) and val(j, i): the same bits
        assert np.all(np.diag(X) >= 0)
        if lp[k]:
            assert np.array_equal(X, np.diag(np.diag(X)))   # r_i^2 on the diagonal (checked to its bound above), 0 off it
        if session_too:
            v2, st2 = s.primal_entries(k, rows, cols)
            assert st2 is None and np.array_equal(v2, val)
            assert np.array_equal(s.primal_diag(k), np.diag(X))
        out.append(X)
    return out


SOLVED = ["maxcut100", "theta30", "rand120", "matcomp60", "blk4x60", "mix4", "sdplp40", "densec40"]


@pytest.mark.parametrize("name", SOLVED)
def test_solved_points(built, name):
    s = common.hip_session(_path(name))
    try:
        s.solve()
        all_positions(s, host.PAIR_UV, name, session_too=True)
    finally:
        s.close()


def _random_state(s, seed, host_too=False):
    """a seeded ADMM state in the table; host_too: the host's record says phase 2 as well, so the Session calls take (U + V) / 2"""
    if host_too:
        s.alm_to_admm()
    Us, Vs, lam = common.random_uv_state(s, seed)
    common.load_uv_state(s.be, Us, Vs, lam)


@pytest.mark.parametrize("name", ["maxcut100", "rand120", "blk4x60", "sdplp40", "densec40"])
def test_random_full_rank_states(built, name):
    s = common.hip_session(_path(name))
    try:
        _random_state(s, 17)
        all_positions(s, host.PAIR_UV, name + " random UV")
        all_positions(s, host.PAIR_RR, name + " random R")
    finally:
        s.close()


def _rank_params(path, r):
    """timesLogRank that aims at rank r from below (the rank rule gives ceil(t ln n), capped)"""
    probe = host.Session.open(path)
    try:
        probe.set_params(verbose=0)
        probe.prepare()
        n0 = probe.block_shape(0)[0]
    finally:
        probe.close()
    return dict(timesLogRank=float((r - 0.5) / np.log(n0)))


def _open_at_rank(name, r):
    path = _path(name)
    s = common.hip_session(path, **_rank_params(path, r))
    cur = s.block_shape(0)[1]
    assert cur <= r
    if cur != r:
        s.be.resize_rank([r])
    assert s.block_shape(0)[1] == r
    return s


def _apply_check(s, src, k, B, tag, X=None):
    """Y and T of one call against their bounds; returns (Y, T)"""
    F = _factor(s, k, src)
    n, rl = F.shape
    lp = s._lp_blocks()[k]
    rc, Y, T = s.be.primal_apply(src, k, B, want_t=not lp)
    assert rc == 0
    Fl, Bl = F.astype(LD), B.astype(LD).reshape(n, -1)
    aF, aB = np.abs(Fl), np.abs(Bl)
    tiny = float(np.finfo(float).tiny)
    if lp:
        want = (Fl[:, :1] * Fl[:, :1]) * Bl
        by = 2 * (n + 1) * U * np.abs(want)
        rt = 0.0
    else:
        Tw = Fl.T @ Bl
        bt = 2 * n * U * (aF.T @ aB)
        et = np.abs(T.astype(LD) - Tw)
        assert T.shape == (rl, Bl.shape[1])
        assert np.all(et <= bt), (tag, "T")
        rt = float(np.max(et / np.maximum(bt, tiny)))
        want = Fl @ Tw
        by = 2 * (n + rl) * U * (aF @ (aF.T @ aB))
    ey = np.abs(Y.astype(LD) - want)
    assert np.all(ey <= by), (tag, "Y")
    ry = float(np.max(ey / np.maximum(by, tiny)))
    rx = 0.0
    if X is not None:   # X assembled from the entry queries: X @ B within the sum of both bounds
        bx = (2 * max(rl, 1) * U * (aF @ (aF.T @ aB)) if not lp else 2 * U * np.abs(want)) + by
        ex = np.abs(X.astype(LD) @ Bl - Y.astype(LD))
        assert np.all(ex <= bx), (tag, "X @ B")
        rx = float(np.max(ex / np.maximum(bx, tiny)))
    print("%s block %d (n %d, rl %d, %d columns): worst ratios T %.3g, Y %.3g, X @ B %.3g" % (tag, k, n, rl, Bl.shape[1], rt, ry, rx))
    return Y, T


@pytest.mark.parametrize("r", [1, 2, 9, 17, 40, 64, 65])
def test_rank_shapes(built, r):
    s = _open_at_rank("rand120", r)
    try:
        _random_state(s, 100 + r)
        X = all_positions(s, host.PAIR_UV, "rand120 r=%d" % r)
        B = np.random.default_rng(r).standard_normal((120, 17))
        _apply_check(s, host.PAIR_UV, 0, B, "rand120 r=%d" % r, X[0])
    finally:
        s.close()


def test_rank_258_through_resize(built):
    s = _open_at_rank("densec40", 258)
    try:
        _random_state(s, 258)
        X = all_positions(s, host.PAIR_UV, "densec40 r=258")
        _apply_check(s, host.PAIR_UV, 0, np.random.default_rng(9).standard_normal((40, 3)), "densec40 r=258", X[0])
    finally:
        s.close()


def test_unequal_cones_on_a_common_device_rank(built):
    s = common.hip_session(_path("blkmix5"))
    try:
        assert len({s.block_shape(k)[1] for k in range(s.nblk)}) > 1
        _random_state(s, 5)
        X = all_positions(s, host.PAIR_UV, "blkmix5")
        for k in range(s.nblk):
            n = s.block_shape(k)[0]
            _apply_check(s, host.PAIR_UV, k, np.random.default_rng(k).standard_normal((n, 5)), "blkmix5", X[k])
    finally:
        s.close()


def test_count_edges(built):
    s = common.hip_session(_path("rand120"))
    try:
        _random_state(s, 31)
        F = _factor(s, 0, host.PAIR_UV)
        n = F.shape[0]
        rng = np.random.default_rng(4)
        for count in (0, 1, 7, 8, 9, EPW - 1, EPW, EPW + 1):
            rows, cols = rng.integers(0, n, count).astype(np.int32), rng.integers(0, n, count).astype(np.int32)
            for e, (i, j) in enumerate([(0, 0), (n - 1, n - 1), (0, n - 1)][:count]):
                rows[e], cols[e] = i, j
            ref = rng.standard_normal(count)
            rc, val, st = s.be.primal_entries(host.PAIR_UV, 0, rows, cols)
            assert rc == 0 and st is None and val.shape == (count,)
            check_entries(val, F, rows, cols, False, "rand120 count %d" % count)
            rc, val2, st = s.be.primal_entries(host.PAIR_UV, 0, rows, cols, ref=ref)
            assert rc == 0 and np.array_equal(val, val2)
            if count == 0:
                assert np.array_equal(st, np.zeros(4))
            else:
                check_stats(st, val, ref, "rand120 count %d" % count)
            rc, none, st2 = s.be.primal_entries(host.PAIR_UV, 0, rows, cols, ref=ref, want_val=False)   # (a score without val)
            assert rc == 0 and none is None and np.array_equal(st, st2)
        # one entry more than a chunk, positions repeating
        count = CHUNK + 1
        rows, cols = rng.integers(0, n, count).astype(np.int32), rng.integers(0, n, count).astype(np.int32)
        edge = [0, CHUNK - 1, CHUNK]
        for e, (i, j) in zip(edge, [(0, 0), (n - 1, n - 1), (0, n - 1)]):
            rows[e], cols[e] = i, j
        want, bound = entry_reference(F, rows, cols, False)
        ref = np.asarray(want, dtype=np.float64) + 1e-3 * rng.standard_normal(count)
        rc, val, st = s.be.primal_entries(host.PAIR_UV, 0, rows, cols)
        assert rc == 0 and st is None
        check_entries(val, F, rows, cols, False, "rand120 chunk + 1")
        for e in edge:   # the first and last entry of every chunk, one by one
            rc, one, _ = s.be.primal_entries(host.PAIR_UV, 0, rows[e:e + 1], cols[e:e + 1])
            assert rc == 0 and one[0] == val[e] and abs(LD(val[e]) - want[e]) <= bound[e], e
        rc, val2, st = s.be.primal_entries(host.PAIR_UV, 0, rows, cols, ref=ref)
        assert rc == 0 and np.array_equal(val, val2)
        check_stats(st, val, ref, "rand120 chunk + 1")
    finally:
        s.close()


def test_a_grid_larger_than_the_device(built):
    s = common.hip_session(_path("matcomp4000"))
    try:
        _random_state(s, 8, host_too=True)
        F = _factor(s, 0, host.PAIR_UV)
        rng = np.random.default_rng(12)
        count = 200000
        rows, cols = rng.integers(0, 2000, count).astype(np.int32), (2000 + rng.integers(0, 2000, count)).astype(np.int32)
        want, _ = entry_reference(F, rows, cols, False)
        ref = np.asarray(want, dtype=np.float64) + 1e-2 * rng.standard_normal(count)
        val, st = s.primal_entries(0, rows, cols, ref=ref)
        check_entries(val, F, rows, cols, False, "matcomp4000")
        check_stats(st, val, ref, "matcomp4000")
    finally:
        s.close()


APPLY = ["maxcut100", "theta30", "rand120", "mix4", "sdplp40", "densec40"]


@pytest.mark.parametrize("name", APPLY)
def test_apply(built, name):
    s = common.hip_session(_path(name))
    try:
        _random_state(s, 23, host_too=True)
        X = all_positions(s, host.PAIR_UV, name)
        lp = s._lp_blocks()
        for k in range(s.nblk):
            n = s.block_shape(k)[0]
            rng = np.random.default_rng(50 + k)
            Y65 = None
            for nc in (1, 15, 16, 17, 64, 65):
                B = rng.standard_normal((n, nc))
                Y, T = _apply_check(s, host.PAIR_UV, k, B, name, X[k])
                if nc == 65:
                    B65, Y65, T65 = B, Y, T
            for c in (0, 15, 16, 40, 64):   # a column does not depend on which other columns share the call
                rc, y1, t1 = s.be.primal_apply(host.PAIR_UV, k, B65[:, c], want_t=not lp[k])
                assert rc == 0 and np.array_equal(y1[:, 0], Y65[:, c]), (name, k, c)
                if not lp[k]:
                    assert np.array_equal(t1[:, 0], T65[:, c])
            # the session's call: the same bits, the vector form
            Ys, Ts = s.primal_apply(k, B65, return_t=True) if not lp[k] else (s.primal_apply(k, B65), None)
            assert np.array_equal(Ys, Y65) and (lp[k] or np.array_equal(Ts, T65))
            assert np.array_equal(s.primal_apply(k, B65[:, 3]), Y65[:, 3])
            _apply_check(s, host.PAIR_RR, k, B65[:, :5], name + " R", None)
    finally:
        s.close()


@pytest.mark.parametrize("name", ["matcomp60", "maxcut100"])
def test_cross_check_with_the_certificate(built, name):
    """at the constraints' positions val - b_i / a_i is the certificate's residual_i / a_i (a_i: the weight of X_pq in <A_i, X>):
    within the entry bound plus the same bound again, for the certificate's own dot"""
    path = _path(name)
    m, b, dims, ent = read_sdpa(path)
    cons = {}
    for mat, blk, i, j, v in ent:
        if mat > 0:
            assert mat not in cons and blk == 1
            cons[mat] = (i - 1, j - 1, v * (1.0 if i == j else 2.0))
    s = common.hip_session(path)
    try:
        s.solve()
        lib, ctx = s._hip()
        out, res = (C.c_double * 10)(), np.zeros(m)
        lib.lorads_hip_certificate.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p,
                                               C.POINTER(C.c_double), C.c_void_p]
        assert lib.lorads_hip_certificate(ctx, host.PAIR_UV, 0.0, 40, 600, out, None, res.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
        rows = np.array([cons[i + 1][0] for i in range(m)], dtype=np.int32)
        cols = np.array([cons[i + 1][1] for i in range(m)], dtype=np.int32)
        a = np.array([cons[i + 1][2] for i in range(m)])
        val, _ = s.primal_entries(0, rows, cols)
        F = _factor(s, 0, host.PAIR_UV)
        _, bound = entry_reference(F, rows, cols, False)
        tol = 2 * bound   # the entry bound plus the same bound again, for the certificate's own dot
        err = np.abs((val.astype(LD) - np.asarray(b, dtype=LD) / a) - res.astype(LD) / a)
        print("%s: %d constraint positions, worst ratio to the bound %.3f" % (name, m, float(np.max(err / tol))))
        assert np.all(err <= tol)
    finally:
        s.close()


def _phase2(path, **kw):
    s = common.hip_session(path, **kw)
    s.alm()
    s.alm_to_admm()
    s.be.init_constr(host.PAIR_UV)
    s.be.cal_obj(host.PAIR_UV)
    e0 = s.be.update_dimacs(host.PAIR_UV)
    res = s.results()
    rho = min(res["admm_rho"] if res["admm_rho"] > 0 else res["alm_rho"], 5000.0)
    return s, rho, e0


@pytest.mark.parametrize("name", ["maxcut100", "rand120", "sdplp40"])
def test_read_only_deterministic_and_owned(built, name):
    path = _path(name)
    before = _mem()
    K = 5
    runs = []
    for look in (True, False):
        s, rho, e0 = _phase2(path)
        try:
            a = s.admm_steps(K, rho, e0)   # (its last dual update still waits for a carrier)
            if look:
                held = _mem()
                for k in range(s.nblk):
                    n = s.block_shape(k)[0]
                    rng = np.random.default_rng(k)
                    rows, cols = rng.integers(0, n, 1000).astype(np.int32), rng.integers(0, n, 1000).astype(np.int32)
                    ref = rng.standard_normal(1000)
                    v1, s1 = s.primal_entries(k, rows, cols, ref=ref)
                    v2, s2 = s.primal_entries(k, rows, cols, ref=ref)
                    assert np.array_equal(v1, v2) and np.array_equal(s1, s2)
                    B = rng.standard_normal((n, 20))
                    assert np.array_equal(s.primal_apply(k, B), s.primal_apply(k, B))
                assert _mem()[1] > held[1]   # (the feature's own scratch)
            b = s.admm_steps(K, rho, a[0])
            runs.append((a, b, _state(s)))
        finally:
            s.close()
    (a1, b1, st1), (a2, b2, st2) = runs
    assert a1 == a2 and b1 == b2
    for x, y in zip(st1, st2):
        assert np.array_equal(x, y)
    assert _mem() == before, (before, _mem())


@pytest.mark.parametrize("name", ["rand120", "sdplp40"])
def test_refusals(built, name):
    s, rho, e0 = _phase2(_path(name))
    try:
        s.admm_steps(3, rho, e0)
        st0, held = _state(s), _mem()
        lp = s._lp_blocks()
        n = s.block_shape(0)[0]
        be, UV = s.be, host.PAIR_UV
        ok = np.zeros(8, dtype=np.int32)

        def with_at(v, at):
            a = ok.copy()
            a[at] = v
            return a

        calls = [
            ("block", lambda: be.primal_entries(UV, s.nblk, ok, ok)[0]),
            ("block", lambda: be.primal_entries(UV, -1, ok, ok)[0]),
            ("src", lambda: be.primal_entries(7, 0, ok, ok)[0]),
            ("row[5] = %d" % n, lambda: be.primal_entries(UV, 0, with_at(n, 5), ok)[0]),
            ("col[6] = -1", lambda: be.primal_entries(UV, 0, ok, with_at(-1, 6))[0]),
            ("col[1] = -1", lambda: be.primal_entries(UV, 0, with_at(n, 2), with_at(-1, 1))[0]),   # (the first offending position)
            ("negative", lambda: be.primal_entries(UV, 0, ok, ok, count=-1)[0]),
            ("NULL", lambda: be.primal_entries(UV, 0, None, ok, count=8)[0]),
            ("NULL", lambda: be.primal_entries(UV, 0, ok, None, count=8)[0]),
            ("NULL", lambda: be.primal_entries(UV, 0, ok, ok, want_val=False)[0]),          # neither val nor ref
            ("ncols 0", lambda: be.primal_apply(UV, 0, np.zeros((n, 1)), ncols=0)[0]),
            ("ncols 1025", lambda: be.primal_apply(UV, 0, np.zeros((n, 1025)))[0]),
            ("NULL", lambda: be.primal_apply(UV, 0, None, ncols=1)[0]),
            ("block", lambda: be.primal_apply(UV, s.nblk, np.zeros((n, 1)))[0]),
        ]
        if any(lp):
            k = lp.index(True)
            calls.append(("LP block", lambda: be.primal_apply(UV, k, np.zeros((s.block_shape(k)[0], 2)), want_t=True)[0]))
        for what, call in calls:
            rc = call()
            assert rc not in (0, 3), what
            assert what in _last_error(s), (what, _last_error(s))
            assert _mem() == held, what   # (refused on the host: not even the scratch was made)
        for x, y in zip(st0, _state(s)):
            assert np.array_equal(x, y)
        with pytest.raises(RuntimeError):
            s.primal_entries(0, [n], [0])
        with pytest.raises(ValueError):
            s.primal_entries(0, [0, 1], [0])
        # the state is still whole
        all_positions(s, UV, name + " after the refusals")
    finally:
        s.close()


def test_sharded_refusal(built):
    s = common.hip_session(_path("blk4x60"), world=2, rank=0, separable=True)
    try:
        held = _mem()
        with pytest.raises(NotImplementedError, match="sharded"):
            s.primal_entries(0, [0], [0])
        with pytest.raises(NotImplementedError, match="sharded"):
            s.primal_apply(0, np.ones(60))
        z = np.zeros(1, dtype=np.int32)
        assert s.be.primal_entries(host.PAIR_UV, 0, z, z)[0] == 3
        assert s.be.primal_apply(host.PAIR_UV, 0, np.ones(60))[0] == 3
        assert _mem() == held
    finally:
        s.close()


def test_cli(built, tmp_path):
    exe = os.path.join(host.LIB_DIR, "lorads")
    path = _path("matcomp60")
    m, b, dims, ent = read_sdpa(path)
    obs = [(i, j, v) for mat, blk, i, j, v in ent if mat > 0]
    assert len(obs) == 200 and all(v == 0.5 for _, _, v in obs)
    seen = {(i, j) for i, j, _ in obs}
    rng = np.random.default_rng(6)
    free = []
    while len(free) < 100:
        i, j = int(rng.integers(1, 31)), int(rng.integers(31, 61))
        if (i, j) not in seen:
            free.append((i, j))
    runs = [([1] * 200, [i for i, _, _ in obs], [j for _, j, _ in obs], np.array(b)), ([1] * 100, [i for i, _ in free], [j for _, j in free], None)]
    for blk, row, col, ref in runs:
        qf, of, sf = tmp_path / "q.txt", tmp_path / "o.txt", tmp_path / "sol.txt"
        primal.write_queries(qf, blk, row, col, ref)
        p = subprocess.run([exe, path, "--solutionFile", str(sf), "--entriesFile", str(qf), "--entriesOut", str(of)], capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        assert "Entries of the primal X" in p.stdout and "%d positions" % len(blk) in p.stdout
        got = primal.read_entries(of)
        assert got.count == len(blk) and got.src == "uv" and got.refs == (ref is not None)
        assert list(got.blk) == blk and list(got.row) == row and list(got.col) == col   # order and 1-based indices
        F = read_solution(sf).cones[0].R
        check_entries(got.val, F, np.array(row) - 1, np.array(col) - 1, False, "cli, %d queries" % len(blk))
        if ref is None:
            assert "RMSE" not in p.stdout and got.stats is None
            continue
        assert np.array_equal(got.ref, ref)
        t = re.search(r"RMSE (\S+), MAE (\S+), max (\S+)", p.stdout)
        rmse, mae, mx = (float(x.rstrip(",")) for x in t.groups())
        assert (rmse, mae, mx) == (got.stats["rmse"], got.stats["mae"], got.stats["maxabs"])
        d = got.val.astype(LD) - ref.astype(LD)
        n = len(blk)
        tol = 2 * (n + 4) * U
        assert mx == np.max(np.abs(got.val - ref))
        # (rmse = sqrt(sum / n), mae = sum / n, refnorm = sqrt(sum): the division and the root add one rounding each)
        assert abs(LD(rmse) - np.sqrt(np.sum(d * d) / n)) <= (tol / 2 + 2 * U) * float(np.sqrt(np.sum(d * d) / n))
        assert abs(LD(mae) - np.sum(np.abs(d)) / n) <= (tol + U) * float(np.sum(np.abs(d)) / n)
        assert abs(LD(got.stats["refnorm"]) - np.sqrt(np.sum(ref.astype(LD) ** 2))) <= (tol / 2 + U) * float(np.linalg.norm(ref))
    bad = tmp_path / "bad.txt"
    bad.write_text("1 1 31\n1 2\n")
    p = subprocess.run([exe, path, "--entriesFile", str(bad)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "line 2" in p.stderr and "End Program" not in p.stdout


# ------------------------------------------------------------------ the size splits of lorads_hip_primal_apply
# Past 256 rows a row panel has more than one strip (k_primal_ftb's blockIdx.x, the partial's address, k_primal_ftb_sum's loop);
# past PRIMAL_ROWS there is a second row panel (first = 0 in the sum, the r0 offsets of the factor, of B and of Y, k_primal_lp
# again).  The cases below are exact: factors in [-3, 3] and B in [-4, 4] are integers, U = F + D and V = F - D with an integer D give
# (U + V) / 2 = F exactly, every product and partial sum is an integer below 2^53, so T = F^T B and Y = F T have ONE correct bit
# pattern whatever the order of the sums -- numpy's float64 product is the reference and nothing is tolerated.  They are cheap: a few
# launches and at most 66000 x 20 numbers each way; the contexts above 65535 rows are opened once for the module.


def _inc_int(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*;" % name, text)
    return int(m.group(1)) << int(m.group(2) or 0)


def _primal_inc_consts():
    text = open(os.path.join(common.ROOT, "lorads_amd", "csrc", "hip", "primal.inc")).read()
    return tuple(_inc_int(text, k) for k in ("PRIMAL_ROWS", "PRIMAL_MAX_STRIPS", "PRIMAL_PW"))


PRIMAL_ROWS, PRIMAL_MAX_STRIPS, PRIMAL_PW = _primal_inc_consts()


def row_strips(rows, smax):
    """(strips, rows_per_strip) of postsolve.inc's row_strips, restated"""
    s = max(1, min(smax, -(-rows // 256)))
    rps = max(64, (-(-rows // s) + 63) & ~63)
    return max(1, -(-rows // rps)), rps


def apply_plan(n):
    """[(first row, rows, strips, rows_per_strip)] of the row panels lorads_hip_primal_apply walks, restated"""
    return [(r0, min(PRIMAL_ROWS, n - r0)) + row_strips(min(PRIMAL_ROWS, n - r0), PRIMAL_MAX_STRIPS) for r0 in range(0, n, PRIMAL_ROWS)]


# n -> the panels (strips, rows_per_strip) the case is there for
PLAN = {256: [(1, 256)], 257: [(2, 192)], 1000: [(4, 256)], 4097: [(17, 256)], 65536: [(256, 256)], 65537: [(256, 256), (1, 64)],
        66000: [(256, 256), (2, 256)]}


def test_the_restated_plan():
    assert (PRIMAL_ROWS, PRIMAL_MAX_STRIPS, PRIMAL_PW) == (65536, 256, 16)
    for n, want in PLAN.items():
        assert [p[2:] for p in apply_plan(n)] == want, n
    assert [p[:2] for p in apply_plan(66000)] == [(0, 65536), (65536, 464)]


_BIG = {}


def _big(n, r):
    """a context of one SDP cone of n rows at rank r, kept for the module (n = 66000: the SDP + LP instance, an LP block of 66000
    columns beside the cone); the rank only grows, so a case that asks for a lower one than the kept context has opens it anew"""
    s = _BIG.get(n)
    if s is not None and s.block_shape(0)[1] > r:
        _BIG.pop(n).close()
        s = None
    if s is None:
        if n == 66000:
            s = common.hip_session(common.generated_instance("primal_sdplp66000", lambda: instances.sdp_lp(66000, 132000, 0, 66)), timesLogRank=1e-3)
            assert [s.block_shape(k) for k in range(s.nblk)] == [(66000, 1), (66000, 1)] and s._lp_blocks() == [False, True]
        else:
            s = _maxcut_session(n, 1)
        _BIG[n] = s
    if s.block_shape(0)[1] != r:
        s.be.resize_rank([r] + [1] * (s.nblk - 1))
    assert s.block_shape(0) == (n, r)
    return s


def teardown_module(module):
    for s in _BIG.values():
        s.close()
    _BIG.clear()


def _load_integers(s, k, seed):
    """integer factors into block k: R, and U = F + D, V = F - D around another F.  Returns {src: F}."""
    n, r = s.block_shape(k)
    rng = np.random.default_rng(seed)
    R, F, D = (rng.integers(-a, a + 1, (n, r)).astype(np.float64) for a in (3, 3, 5))
    s.be.set_mat(host.MAT_R, k, R)
    s.be.set_mat(host.MAT_U, k, F + D)
    s.be.set_mat(host.MAT_V, k, F - D)
    return {host.PAIR_RR: R, host.PAIR_UV: F}


def _indicator_rows(n):
    """the rows whose unit vectors ride in B: both ends of the cone, of the first strip, of the first row panel"""
    rps = apply_plan(n)[0][3]
    return sorted({i for i in (0, rps - 1, rps, PRIMAL_ROWS - 1, PRIMAL_ROWS, n - 1) if 0 <= i < n})


def _integer_b(rng, n, nc, rows):
    """B (n, nc) of integers in [-4, 4] whose last columns are the unit vectors of `rows` (column 0 stays random).  Returns
    (B, {column: row})."""
    B = rng.integers(-4, 5, (n, nc)).astype(np.float64)
    take = rows[len(rows) - min(len(rows), nc - 1):]
    at = {}
    for j, i in zip(range(nc - len(take), nc), take):
        B[:, j] = 0.0
        B[i, j] = 1.0
        at[j] = i
    return B, at


def _same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        print("%s: %d of %d values differ, first at %s (got %r, want %r), last at %s" % (tag, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])],
                                                                                         want[tuple(bad[0])], bad[-1].tolist()))
    assert len(bad) == 0, tag


def _exact_apply(s, src, k, F, nc, seed, tag, entries):
    """one call with integer data against numpy's exact product; with `entries`, column i of X is asked of primal_entries too"""
    n = F.shape[0]
    lp = s._lp_blocks()[k]
    B, at = _integer_b(np.random.default_rng(seed), n, nc, _indicator_rows(n))
    rc, Y, T = s.be.primal_apply(src, k, B, want_t=not lp)
    assert rc == 0, _last_error(s)
    if lp:
        _same(Y, (F[:, :1] * F[:, :1]) * B, tag + " Y")
    else:
        Tw = F.T @ B
        assert np.abs(F @ Tw).max() < 2.0 ** 53
        _same(T, Tw, tag + " T")
        _same(Y, F @ Tw, tag + " Y")
    for j, i in at.items():
        if lp:
            xi = np.zeros(n)
            xi[i] = F[i, 0] * F[i, 0]
        else:
            xi = F @ F[i]
            _same(T[:, j], F[i], "%s T of e_%d" % (tag, i))     # row i of F
        _same(Y[:, j], xi, "%s Y of e_%d" % (tag, i))           # column i of X
        if entries:
            rc, val, _ = s.be.primal_entries(src, k, np.arange(n, dtype=np.int32), np.full(n, i, dtype=np.int32))
            assert rc == 0, _last_error(s)
            _same(val, xi, "%s entries of column %d" % (tag, i))
    return len(at)


def _exact_block(s, k, seed, columns, tag):
    t0 = time.perf_counter()
    Fs = _load_integers(s, k, seed)
    seen = 0
    for src, what in ((host.PAIR_RR, "RR"), (host.PAIR_UV, "UV")):
        for nc in columns:
            seen += _exact_apply(s, src, k, Fs[src], nc, seed + nc, "%s %s, %d columns" % (tag, what, nc), entries=nc == max(columns))
    print("%s: bit-equal to numpy on both sources, columns %s, %d unit vectors; %.2f s" % (tag, list(columns), seen, time.perf_counter() - t0))


@pytest.mark.parametrize("r", [5, 20])
@pytest.mark.parametrize("n", [256, 257, 1000, 4097])
def test_apply_is_exact_on_integers_past_one_strip(built, n, r):
    """1, 2, 4 and 17 row strips (257: strips of 192 rows, a wavefront's quarter of 48), an odd padded rank and two rank tiles, one
    column, a full column panel and one column more"""
    (plan,) = apply_plan(n)
    assert plan[2:] == PLAN[n][0] and (plan[2] > 1) == (n > 256)
    s = _maxcut_session(n, r)
    try:
        _exact_block(s, 0, 7000 + n + r, (1, 16, 17), "n %d r %d (%d strips of %d rows)" % ((n, r) + plan[2:]))
    finally:
        s.close()


@pytest.mark.parametrize("n,r", [(65536, 5), (65536, 20), (65537, 5), (65537, 20), (66000, 5), (66000, 20)])
def test_apply_is_exact_on_integers_past_one_row_panel(built, n, r):
    """a full first row panel of 256 strips alone (65536), then a second panel of one row and of 464 rows in two strips: T is added
    to, not overwritten, and every array is read and written at r0 = 65536.  17 columns: two column panels, so T is opened anew for
    the second one after the first one's second row panel.  Unit vectors at rows 65535, 65536 and n - 1 cross the panel's edge; the
    entry kernel is asked for the same columns of X with row indices above 65535."""
    plan = apply_plan(n)
    assert [p[2:] for p in plan] == PLAN[n] and len(plan) == (2 if n > PRIMAL_ROWS else 1) and plan[0][2] == PRIMAL_MAX_STRIPS
    _exact_block(_big(n, r), 0, 9000 + n + r, (17,), "n %d r %d (%d row panels)" % (n, r, len(plan)))


def test_lp_block_is_exact_on_integers_past_one_row_panel(built):
    """Y = diag(f^2) B on an LP block of 66000 columns: k_primal_lp on a second panel; T is refused as on any LP block"""
    s = _big(66000, 5)
    assert len(apply_plan(s.block_shape(1)[0])) == 2
    _exact_block(s, 1, 9100, (1, 17), "LP block of 66000")
    rc = s.be.primal_apply(host.PAIR_UV, 1, np.zeros((66000, 2)), want_t=True)[0]
    assert rc not in (0, 3) and "LP block" in _last_error(s)


def test_apply_random_values_past_one_row_panel(built):
    """the longdouble route of _apply_check at two row panels.  Its bounds grow with n (2 n u |F^T| |B| for T): at n = 66000 they are
    wide, and the exact cases above carry the weight; this one shows that non-integer data takes the same path to the same bounds."""
    t0 = time.perf_counter()
    s = _big(66000, 20)
    assert len(apply_plan(66000)) == 2
    _random_state(s, 66)
    for k in range(s.nblk):
        n = s.block_shape(k)[0]
        _apply_check(s, host.PAIR_UV, k, np.random.default_rng(660 + k).standard_normal((n, 17)), "sdplp66000 random")
    print("sdplp66000 random: %.2f s" % (time.perf_counter() - t0))
