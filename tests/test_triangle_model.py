"""The separation's numpy model (tests/triangle_model.py) against first principles, the writer of the tightened problem
(lrd_session_write_tightened) against the model's writer, the 5-cycle end to end through the CPU oracle, and the refusals that need
no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.cuts import SIGNS, Cuts, CutsStruct, read_sdpa, read_tightened
from tests import common
from tests import triangle_model as tm


def _sphere_rows(rng, n, r, t):
    F = rng.standard_normal((n, r))
    return F / np.linalg.norm(F, axis=1)[:, None] * np.asarray(t)[:, None]


@pytest.mark.parametrize("n,r", [(3, 1), (4, 2), (7, 3), (12, 5)])
def test_model_against_triple_loop(n, r):
    rng = np.random.default_rng(n)
    t = rng.uniform(0.5, 2.0, n)
    F = _sphere_rows(rng, n, r, t)
    X = F @ F.T
    want = {}
    for p in range(n):
        for q in range(p + 1, n):
            for s in range(q + 1, n):
                a, b, c = X[p, q] / (t[p] * t[q]), X[p, s] / (t[p] * t[s]), X[q, s] / (t[q] * t[s])
                for cl in range(4):
                    want[(p, q, s, cl)] = -1.0 - (SIGNS[cl][0] * a + SIGNS[cl][1] * b + SIGNS[cl][2] * c)
    for dtype in (np.float64, np.longdouble):
        P, Q, S, Cl, V = tm.enumerate_all(F, t, dtype)
        assert len(V) == 4 * n * (n - 1) * (n - 2) // 6 == len(want)
        eps = tm.eps_of(F, t, P, Q, S)
        got = {k: v for k, v in zip(zip(P.tolist(), Q.tolist(), S.tolist(), Cl.tolist()), V)}
        assert set(got) == set(want)
        assert all(abs(float(got[k]) - want[k]) <= e for k, e in zip(zip(P.tolist(), Q.tolist(), S.tolist(), Cl.tolist()), eps))
        ex = tm.exact_values(F, t, P, Q, S, Cl)
        assert np.all(np.abs(V.astype(np.longdouble) - ex) <= eps)
    # the total order: v descending, then p, q, s, c ascending
    o = tm.order(V, P, Q, S, Cl)
    keys = [(-float(V[i]), int(P[i]), int(Q[i]), int(S[i]), int(Cl[i])) for i in o]
    assert keys == sorted(keys)


@pytest.mark.parametrize("n,live", [(7, None), (12, None), (20, None), (35, None), (40, None), (20, 6), (37, 12), (40, 11), (40, 40)])
def test_planted_counts_against_full_enumeration(n, live):
    """the closed forms the separation's cases past 1024 rows rest on (plant_counts: all rows planted, and zero rows above the last
    `live`), the values a planted triple takes and the kept list's first triples, against the stored enumeration"""
    F, t = tm.plant_rows(n, live), np.ones(n)
    assert np.array_equal(F[-1], tm.PLANT_D[(n - 1) % 3]) and (live is None or live == n or not F[0].any())
    P, Q, S, Cl, V = tm.enumerate_all(F, t)
    assert np.array_equal(V, tm.exact_values(F, t, P, Q, S, Cl).astype(np.float64))   # (small integers: exact in both)
    assert set(V.tolist()) <= {2.0, 1.0, 0.0, -1.0, -2.0, -3.0, -5.0, -7.0}
    hi, lo = tm.plant_counts(n, live)
    assert int(np.count_nonzero(V > 1.5)) == hi and int(np.count_nonzero(V > 0.5)) == lo
    top = V > 1.5
    assert (V[top] == 2.0).all() and (Cl[top] == 0).all()
    o = tm.order(V[top], P[top], Q[top], S[top], Cl[top])
    rows = list(range(0 if live is None else n - live, n))
    want = tm.first_distinct_triples(rows, 100)
    assert len(want) == min(100, hi)
    assert list(zip(P[top][o].tolist(), Q[top][o].tolist(), S[top][o].tolist()))[:100] == want


@pytest.mark.parametrize("n,r,minv,K", [(30, 4, 0.05, 50), (41, 7, 1e-3, 10 ** 6), (25, 1, 0.0, 7), (33, 6, 0.3, 1)])
def test_scan_against_full_enumeration(n, r, minv, K):
    """the streamed scan returns what the stored longdouble enumeration gives: counts at minv -+ eps and the top of the list"""
    rng = np.random.default_rng(n + r)
    t = rng.uniform(0.5, 2.0, n)
    F = _sphere_rows(rng, n, r, t)
    P, Q, S, Cl, V = tm.enumerate_all(F, t, np.longdouble)
    eps = tm.eps_of(F, t, P, Q, S)
    sc = tm.Scan(F, t, minv, K)
    assert sc.count_hi == int(np.count_nonzero(V > minv + eps))
    assert sc.count_lo == int(np.count_nonzero(V > minv - eps))
    m = V > minv
    o = tm.order(V[m], P[m], Q[m], S[m], Cl[m])[:K]
    k = len(o)
    assert len(sc.v) >= k
    for got, want in ((sc.p, P), (sc.q, Q), (sc.s, S), (sc.c, Cl)):
        assert np.array_equal(got[:k], want[m][o])
    # the same rows evaluated pair by pair and through the Gram matrix differ by rounding of the longdouble alone
    assert np.all(np.abs(sc.v[:k] - V[m][o]) <= eps[m][o] * 2.0 ** -8)


def test_pm1_point_violates_nothing():
    """X = x x^T with x = sigma o t is a cut matrix: it lies in the metric polytope, every v <= eps"""
    rng = np.random.default_rng(5)
    for n, r in ((9, 1), (20, 3)):
        t = rng.uniform(0.5, 2.0, n)
        sigma = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        f = rng.standard_normal(r)
        f /= np.linalg.norm(f)
        F = (sigma * t)[:, None] * f[None, :]
        P, Q, S, Cl, V = tm.enumerate_all(F, t)
        assert np.all(V <= tm.eps_of(F, t, P, Q, S))
        sc = tm.Scan(F, t, 1e-9, 100)
        assert sc.count_lo == 0 and len(sc.v) == 0


def _factor(s):
    """the factor the separation takes: (U + V) / 2 once phase 2 has run, the phase-1 R otherwise"""
    if s.results()["admm_iter"] > 0:
        return [(s.be.get_mat(host.MAT_U, k) + s.be.get_mat(host.MAT_V, k)) / 2 for k in range(s.nblk)]
    return [s.be.get_mat(host.MAT_R, k) for k in range(s.nblk)]


def _write_tightened(sess, path, cuts):
    """lrd_session_write_tightened with a cut list handed in: cuts = [(cone, p, q, s, cls)]"""
    a = np.array(cuts, dtype=np.int64).reshape(-1, 5)
    c = Cuts(np.zeros(int(a[:, 0].max()) + 1 if len(a) else 1, dtype=np.int64), a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], np.zeros(len(a)))
    sess.write_tightened(path, c)


def test_c5_through_the_oracle(tmp_path):
    """the 5-cycle: exactly 10 violated inequalities, and the tightened problem's optimum is the maximum cut, 4"""
    prob = tm.c5_problem()
    path = str(tmp_path / "c5.dat-s")
    instances.write_sdpa(prob, path)
    s = common.oracle_session(path)
    try:
        r = s.solve()
        assert abs(r["pObj"] + 4.52254) <= 1e-4
        F = _factor(s)[0]
        t = tm.t_of(prob)[0]
        P, Q, S, Cl, V = tm.enumerate_all(F, t, np.longdouble)
        viol = V > 1e-3
        assert int(viol.sum()) == 10, V[viol]
        assert abs(float(V.max()) - 0.427) <= 2e-3
        cuts = [(0, int(P[i]), int(Q[i]), int(S[i]), int(Cl[i])) for i in np.nonzero(viol)[0]]
        tight = str(tmp_path / "c5_tight.dat-s")
        _write_tightened(s, tight, cuts)
    finally:
        s.close()
    assert sorted(read_tightened(tight, 5)) == sorted(cuts)
    s2 = common.oracle_session(tight)
    try:
        r2 = s2.solve()
    finally:
        s2.close()
    p2tol = 1e-5
    print("C5: pObj %.9f -> tightened %.9f" % (r["pObj"], r2["pObj"]))
    assert abs(r2["pObj"] + 4.0) <= 5 * p2tol * (1 + 4), r2["pObj"]


def _multiset(ent):
    return sorted(ent)


@pytest.mark.parametrize("name", ["maxcut100", "blk4x60", "scaledpm1_120"])
def test_c_writer_against_model_writer(tmp_path, name):
    prob = instances.NAMED[name]()
    path = common.generated_instance(name)
    rng = np.random.default_rng(len(name))
    cuts = []
    for _ in range(40):
        k = int(rng.integers(0, len(prob["blocks"])))
        p, q, s_ = sorted(rng.choice(prob["blocks"][k], 3, replace=False).tolist())
        cuts.append((k, p, q, s_, int(rng.integers(0, 4))))
    s = host.Session.open(path, lib=common.load_oracle())
    try:
        for tag, lst in (("cuts", cuts), ("none", [])):
            got_path, want_path = str(tmp_path / (tag + "_c.dat-s")), str(tmp_path / (tag + "_model.dat-s"))
            if lst:
                _write_tightened(s, got_path, lst)
            else:
                s.write_tightened(got_path, None)
            instances.write_sdpa(tm.tightened(prob, lst), want_path)
            gm, gblocks, gb, gent = read_sdpa(got_path)
            wm, wblocks, wb, went = read_sdpa(want_path)
            assert (gm, gblocks) == (wm, wblocks)
            assert sorted(gb.tolist()) == sorted(wb.tolist()) and np.array_equal(gb, wb)
            assert _multiset(gent) == _multiset(went)
            if lst:
                assert read_tightened(got_path, prob["m"]) == lst
            else:   # zero cuts: the original problem, no LP block
                om, oblocks, ob, oent = read_sdpa(path)
                assert (gm, gblocks) == (om, oblocks) and np.array_equal(gb, ob) and _multiset(gent) == _multiset(oent)
        with pytest.raises(ValueError):
            _write_tightened(s, str(tmp_path / "bad.dat-s"), [(0, 3, 2, 5, 0)])
        with pytest.raises(ValueError):
            _write_tightened(s, str(tmp_path / "bad.dat-s"), [(0, 1, 2, prob["blocks"][0], 0)])
    finally:
        s.close()


def test_writer_refuses_a_problem_with_an_lp_block(tmp_path):
    s = host.Session.open(common.instance_path("sdplp40"), lib=common.load_oracle())
    try:
        with pytest.raises(ValueError):
            _write_tightened(s, str(tmp_path / "x.dat-s"), [(0, 1, 2, 3, 0)])
    finally:
        s.close()


def test_oracle_backend_refuses_and_table_mirror():
    s = common.oracle_session(common.instance_path("maxcut100"))
    try:
        assert not s.be.has_triangle_cuts()
        with pytest.raises(NotImplementedError):
            s.triangle_cuts(max_cuts=10)
    finally:
        s.close()
    names = [f[0] for f in host.BackendStruct._fields_]
    assert "triangle_cuts" in names
    lib = host.host_lib()
    lib.lrd_backend_sizeof.restype = C.c_size_t
    assert lib.lrd_backend_sizeof() == C.sizeof(host.BackendStruct)
    assert C.sizeof(CutsStruct) == 88
    hip = C.CDLL(os.path.join(host.LIB_DIR, "liblorads_hip.so"))
    assert hasattr(hip, "lorads_hip_triangle_cuts")


@pytest.mark.parametrize("args", [["--cutsMax", "0"], ["--cutsMax", "-3"], ["--cutsMax", "1048577"], ["--cutsMax", "12x"],
                                  ["--cutsMax", "10", "--cutsMinViolation", "-1e-3"], ["--cutsMax", "10", "--cutsMinViolation", "nan"],
                                  ["--cutsMax", "10", "--cutsMinViolation", "inf"], ["--cutsFile", "out.dat-s"],
                                  ["--cutsMinViolation", "0.01"]])
def test_cli_refuses_bad_values_before_the_backend(tmp_path, args):
    host.host_lib()
    exe = os.path.join(host.LIB_DIR, "lorads")
    # (no GPU and no HIP library in reach: whatever passes the options would fail with another code and message)
    r = subprocess.run([exe, common.instance_path("maxcut100")] + args, cwd=tmp_path, capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "bad value" in r.stderr or "needs --cutsMax" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.dat-s")


def test_sign_patterns():
    """the four classes in the issue's order; each triple's four left-hand sides sum to zero, so the violations sum to -4"""
    assert SIGNS.tolist() == [[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]
    a, b, c = 0.3, -0.7, 0.2
    v = tm.class_values(np.array([a]), np.array([b]), np.array([c]))[:, 0]
    assert abs(v.sum() + 4.0) <= 1e-15
    assert np.allclose(v, [-1 - (x * a + y * b + z * c) for x, y, z in SIGNS.tolist()], rtol=0, atol=1e-15)


def test_session_drivers_merge_the_cones_lists_through_a_stub_table():
    """lrd_session_triangle_cuts and lrd_session_entry_bounds over a table whose two slots return fixed, sorted lists for three
    cones: the merged list is (violation descending, cone, p, q[, s], class ascending) with violations that tie across cones
    and is cut off at max_cuts below the total; count stays per cone, passes add up.  No GPU: the merge is the host's."""
    path = common.generated_instance("blk3x8", make=lambda: instances.blockdiag_maxcut(3, 8, 10, 77))   # (three cones of 8)
    # per cone (p, q, s, class, violation), sorted as a backend returns them: 0.5 and 0.25 tie across the cones, 0.5 within cone 1
    cut_lists = [[(0, 1, 2, 3, 0.5), (0, 1, 3, 0, 0.25), (1, 2, 3, 1, 0.125)],
                 [(0, 1, 2, 1, 0.75), (0, 1, 2, 2, 0.5), (0, 2, 3, 0, 0.5), (2, 3, 4, 0, 0.25)],
                 [(0, 1, 2, 3, 0.5), (0, 1, 2, 0, 0.25), (4, 5, 6, 2, 0.0625)]]
    bnd_lists = [[(p, q, cl % 2, v) for p, q, _, cl, v in lst] for lst in cut_lists]  # (p, q, class, violation), sorted too
    counts, calls = [30, 41, 52], []

    def fill(rows, count, n_violated, cols, kept, passes, np_):
        count[0] = n_violated
        for e, row in enumerate(rows):
            for ptr, val in zip(cols, row):
                ptr[e] = val
        kept[0], passes[0] = len(rows), np_
        return 0

    def stub_cuts(ctx, src, blk, minv, max_cuts, count, p, q, s_, cls, viol, kept, passes):
        calls.append(("cuts", blk, minv, max_cuts))
        return fill(cut_lists[blk][:max_cuts], count, counts[blk], (p, q, s_, cls, viol), kept, passes, blk + 1)

    def stub_bounds(ctx, src, blk, lower, upper, minv, max_cuts, count, p, q, cls, viol, kept, passes):
        calls.append(("bounds", blk, lower, upper, minv, max_cuts))
        return fill(bnd_lists[blk][:max_cuts], count, counts[blk], (p, q, cls, viol), kept, passes, 1)

    s = host.Session.open(path)   # (the product's host library and a table of stubs alone: no oracle, no backend)
    s.set_params(verbose=0)
    s.prepare(1, 0)
    st = host.BackendStruct()
    types = dict(host.BackendStruct._fields_)
    keep = (types["set_mat"](lambda ctx, which, k, ptr: 0), types["triangle_cuts"](stub_cuts),
            types["entry_bounds"](stub_bounds))   # (alive as long as the table is)
    st.name = b"stub"
    st.set_mat, st.triangle_cuts, st.entry_bounds = keep
    s.attach(st)
    try:
        all_cuts = sorted([(k,) + r for k in range(3) for r in cut_lists[k]], key=lambda r: (-r[5],) + r[:5])
        all_bnds = sorted([(k,) + r for k in range(3) for r in bnd_lists[k]], key=lambda r: (-r[4],) + r[:4])
        assert [r[0] for r in all_cuts[:6]] == [1, 0, 1, 1, 2, 0] and [r[5] for r in all_cuts[:6]] == [0.75, 0.5, 0.5, 0.5, 0.5, 0.25]
        for max_cuts in (6, 4, 1, 100):
            c = s.triangle_cuts(max_cuts=max_cuts, min_violation=0.03125)
            got = list(zip(c.cone.tolist(), c.p.tolist(), c.q.tolist(), c.s.tolist(), c.cls.tolist(), c.violation.tolist()))
            assert got == all_cuts[:max_cuts], (max_cuts, got)
            assert c.count.tolist() == counts and len(c) == min(max_cuts, 10) and c.passes == 6 and c.max_cuts == max_cuts
            b = s.entry_bounds(max_cuts=max_cuts, lower=-0.5, upper=0.25, min_violation=0.03125)
            got = list(zip(b.cone.tolist(), b.p.tolist(), b.q.tolist(), b.cls.tolist(), b.violation.tolist()))
            assert got == all_bnds[:max_cuts], (max_cuts, got)
            assert b.count.tolist() == counts and len(b) == min(max_cuts, 10) and b.passes == 3 and b.max_cuts == max_cuts
            assert b.bound.tolist() == [0.25 if cl else -0.5 for cl in b.cls.tolist()]
        assert calls[:3] == [("cuts", k, 0.03125, 6) for k in range(3)]
        assert calls[3:6] == [("bounds", k, -0.5, 0.25, 0.03125, 6) for k in range(3)]
    finally:
        s.close()
    del keep
