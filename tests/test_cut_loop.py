"""Cut-tightened +-1 problems on the GPU: round_pm1 and triangle_cuts on a context whose LP block holds the
slacks of triangle cuts, against the untightened context's bits and the numpy models (tests/cutloop_model.py, rounding_model.py,
triangle_model.py); the device check's refusals in the host recogniser's words; read-only continuation; lorads_amd.cuts.cut_loop and
the command line on a tightened file."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.cuts import Cuts, cut_loop, read_sdpa
from tests import common
from tests import cutloop_model as cm
from tests import rounding_model as rm
from tests import triangle_model as tm
from tests.test_rounding import _phase2
from tests.test_triangle_cuts import BIG_N, _call, _last_error, _load, _maxcut_problem, _mem, _packed

pytestmark = pytest.mark.gpu

_DIR = None
_S = {}


def _dir():
    global _DIR
    if _DIR is None:
        _DIR = tempfile.mkdtemp(prefix="lorads_cutloop_")
        atexit.register(shutil.rmtree, _DIR, True)
    return _DIR


def teardown_module(module):
    for v in _S.values():
        v["s"].close()
    _S.clear()


def _cuts(lst):
    a = np.array(lst, dtype=np.int64).reshape(-1, 5)
    return Cuts(np.zeros(1, dtype=np.int64), a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], np.zeros(len(a)))


def _c5_cuts():
    """the 10 inequalities the 5-cycle's SDP optimum violates: its rows are unit vectors 4 pi / 5 apart"""
    ang = 4 * np.pi / 5 * np.arange(5)
    P, Q, S, Cl, V = tm.enumerate_all(np.stack([np.cos(ang), np.sin(ang)], 1), np.ones(5))
    m = V > 1e-3
    assert int(m.sum()) == 10
    return [(0, int(p), int(q), int(s), int(c)) for p, q, s, c in zip(P[m], Q[m], S[m], Cl[m])]


def _solved(name):
    """the module's solved tightened contexts: 'maxcut100' (the golden file, solved, its 300 most violated inequalities appended by
    Session.write_tightened, solved again) and 'c5' (the 5-cycle with the 10 inequalities its optimum violates).  s: the solved
    tightened context; plain / tight: the two files; r0 / r1: the two solves' results; present: the cuts of `tight`."""
    if name not in _S:
        tight = os.path.join(_dir(), name + "_round1.dat-s")
        if name == "c5":
            plain = common.generated_instance("cutloop_c5", tm.c5_problem)
            lst = _c5_cuts()
        else:
            plain = common.instance_path(name)
        s0 = common.hip_session(plain)
        try:
            r0 = s0.solve()
            if name != "c5":
                c = s0.triangle_cuts(max_cuts=300, min_violation=1e-3)
                assert len(c) == 300
                lst = list(zip(c.cone.tolist(), c.p.tolist(), c.q.tolist(), c.s.tolist(), c.cls.tolist()))
            s0.write_tightened(tight, _cuts(lst))
        finally:
            s0.close()
        s = common.hip_session(tight)
        r1 = s.solve()
        _S[name] = dict(s=s, plain=plain, tight=tight, r0=r0, r1=r1, cuts=lst, present=s.present_cuts())
        m0 = read_sdpa(plain)[0]
        assert _S[name]["present"] == [(k, p, q, s_, cl, m0 + e, e) for e, (k, p, q, s_, cl) in enumerate(lst)]
    return _S[name]


def _factor(s):
    if s.results()["admm_iter"] > 0:
        return (s.be.get_mat(host.MAT_U, 0) + s.be.get_mat(host.MAT_V, 0)) / 2
    return s.be.get_mat(host.MAT_R, 0)


# ---- 1. round_pm1: the bits of the untightened context, then the model's search on the union pattern

@pytest.mark.parametrize("name", ["maxcut100", "c5"])
def test_rounding_has_the_untightened_bits_and_the_union_colouring(name):
    """K = 65 trials (a second sign word with one trial) from one seeded factor in the phase-1 state of both contexts, the narrower
    rank padded with zero columns.  Before the search: f0 of every trial, the best trial and its signs, and the shared hyperplanes are
    the untightened context's bits (the sign words themselves are not exported per trial: every trial's f0 and the model's signs from
    the exported hyperplanes stand for them).  After it: f, the rounds and the best signs are the model's with the colouring of the
    union pattern.  NotImplementedError on a library that refuses the LP block."""
    S = _solved(name)
    K, seed = 65, 5
    sp, st = common.hip_session(S["plain"]), common.hip_session(S["tight"])
    try:
        (n, rp), (_, rt) = sp.block_shape(0), st.block_shape(0)
        R = np.zeros((n, max(rp, rt)))
        R[:, :min(rp, rt)] = np.random.default_rng(20261).standard_normal((n, min(rp, rt)))
        sp.be.set_mat(host.MAT_R, 0, np.ascontiguousarray(R[:, :rp]))
        st.be.set_mat(host.MAT_R, 0, np.ascontiguousarray(R[:, :rt]))
        a = sp.round_pm1(trials=K, seed=seed, local_search_rounds=0, tol=0, hyperplanes=True)
        b = st.round_pm1(trials=K, seed=seed, local_search_rounds=0, tol=0, hyperplanes=True)
        print("%s: ranks %d / %d, %d cuts, f0 of trial 0 %.17g / %.17g" % (name, rp, rt, len(S["present"]), a.obj0[0], b.obj0[0]))
        assert len(b.cones) == 2 and b.cones[1].n == 0 and len(b.lp_upper) == len(S["present"]) and (b.lp_upper == 4.0).all()
        assert a.obj0.tobytes() == b.obj0.tobytes() and a.obj.tobytes() == b.obj.tobytes()
        assert (a.best0, a.best, a.rounds) == (b.best0, b.best, b.rounds) == (a.best0, a.best0, 0)
        assert np.array_equal(a.cones[0].sigma, b.cones[0].sigma) and np.array_equal(a.sign, b.sign)
        r_ = min(rp, rt)
        assert a.cones[0].G[:r_].tobytes() == b.cones[0].G[:r_].tobytes()
        assert np.array_equal(b.cones[0].t, a.cones[0].t) and b.cones[0].T == a.cones[0].T
        # the search on the tightened context
        P = rm.Pm1Problem.read(S["plain"])
        c = st.round_pm1(trials=K, seed=seed, local_search_rounds=100, tol=0, hyperplanes=True)
        assert c.obj0.tobytes() == b.obj0.tobytes()
        Rd, G = st.be.get_mat(host.MAT_R, 0), c.cones[0].G
        sig0, proj = rm.signs(Rd, G)
        near = np.any(np.abs(proj) <= 1e-12 * np.linalg.norm(Rd, axis=1)[:, None] * np.linalg.norm(G, axis=0)[None, :], axis=0)
        keep = ~near
        adj = cm.union_adj(P.adj[0], S["present"], 0)
        assert sum(len(x) for x in adj) > sum(len(x) for x in P.adj[0])   # (the cuts add positions to the pattern)
        sig1, rounds = rm.local_search(P.C[0], P.t[0], adj, sig0, 100)
        want = rm.objective(P.C[0], P.t[0], sig1)
        scale = st.results()["scale_obj_his"]
        print("%s: scale %g, %d near-zero trials excluded, rounds %d (model %d), colours %d (C alone %d)"
              % (name, scale, int(near.sum()), c.rounds, rounds, rm.colouring(adj).max() + 1, rm.colouring(P.adj[0]).max() + 1))
        if scale == 1.0 and name == "maxcut100":   # unit weights: every sum is exact
            assert np.array_equal(c.obj[keep], want[keep])
        else:
            assert np.all(np.abs(c.obj[keep] - want[keep]) <= 1e-13 * np.maximum(1.0, np.abs(want[keep])))
        if keep.all():
            assert c.rounds == rounds
        if keep[c.best]:
            assert np.array_equal(c.cones[0].sigma, sig1[:, c.best])
        assert c.best == int(np.argmin(c.obj)) and c.f_best == c.obj[c.best]
    finally:
        sp.close()
        st.close()


# ---- 2. the dual bound with the LP term

@pytest.mark.parametrize("name", ["c5", "maxcut100"])
def test_dual_bound_with_the_slack_term(name):
    """d against the model's from the exported y, lambda_min and LP slacks with u_j = 4, to test_kcut.py's tolerance for the same
    comparison; d <= f_best; on the 5-cycle f_best = -4 and the gap is below a tenth of the untightened (4.5225 - 4) / 4.5225"""
    S = _solved(name)
    s = S["s"]
    r = s.round_pm1(trials=256, seed=1, local_search_rounds=100, tol=1e-8)
    sol = s.solution(tol=1e-8)
    row, col, val = sol.slack(0)
    n = sol.cones[0].n
    Sm = np.zeros((n, n))
    Sm[row, col] = val
    Sm[col, row] = val
    lam = float(np.linalg.eigvalsh(Sm)[0])
    row, _, val = sol.slack(1)
    slack = np.zeros(sol.cones[1].n)
    slack[row] = val
    b = read_sdpa(S["tight"])[2]
    d = cm.dual_bound(b, sol.y, [float(n)], [lam], [c.scale for c in S["present"]], slack)
    tol = 1e-8 * max(1.0, abs(d))
    print("%s: pObj %.9f -> %.9f, d %.12f (model %.12f), f_best %.12f, gap %.6e, lambda_min %.3e, %d of %d slacks negative, LP term %.3e"
          % (name, S["r0"]["pObj"], S["r1"]["pObj"], r.bound, d, r.f_best, r.gap, lam, r.lp_negative, len(slack),
             4.0 * np.minimum(0.0, slack).sum()))
    assert abs(r.bound - d) <= tol, (r.bound, d)
    assert abs(r.by - float(b @ sol.y)) <= 1e-12 * max(1.0, abs(r.by))
    assert r.bound <= r.f_best + tol
    assert r.gap == pytest.approx((r.f_best - r.bound) / max(1.0, abs(r.bound)), rel=1e-15)
    assert r.lp_negative == int(np.sum(slack < 0)) and np.array_equal(r.lp_upper, np.full(len(slack), 4.0))
    if name == "c5":
        assert r.f_best == -4.0
        untightened = (4.5225 - 4) / 4.5225
        assert abs(S["r0"]["pObj"] + 4.52254) <= 1e-3
        assert r.gap < untightened / 10, (r.gap, untightened)


# ---- 3. the exclusion, exact on planted integer rows

def _planted_context(n, present):
    """a Max-Cut context of n vertices whose file holds `present` as triangle rows, and its SDP cone's rank"""
    prob = _maxcut_problem(n)
    path = os.path.join(_dir(), "plant%d_%d.dat-s" % (n, len(present)))
    instances.write_sdpa(tm.tightened(prob, present), path)
    s = common.hip_session(path)
    assert s.block_shape(0)[0] == n and s.block_shape(0)[1] >= 3
    return s, s.block_shape(0)[1]


def _planted_case(n, live, violated, idle, K):
    rows = list(range(n)) if live is None else list(range(n - live, n))
    hi, _ = tm.plant_counts(n, live)
    present = [(0, p, q, s_, 0) for p, q, s_ in violated] + idle
    for p, q, s_ in violated:
        assert len({p % 3, q % 3, s_ % 3}) == 3 and p >= rows[0]
    s, r = _planted_context(n, present)
    try:
        F = np.zeros((n, r))
        F[:, :3] = tm.plant_rows(n, live)
        _load(s, F)
        assert _call(s, 1.5, 0)[0] == hi - len(violated)
        got = _call(s, 1.5, K)
        cnt, p, q, s_, cl, v, passes = got
        gone = set(violated)
        want = [x for x in tm.first_distinct_triples(rows, K + len(violated)) if x not in gone][:K]
        print("planted n %d: count %d (%d present and violated), kept %d, passes %d" % (n, cnt, len(violated), len(p), passes))
        assert cnt == hi - len(violated) and len(p) == min(K, cnt) == len(want)
        assert (v == 2.0).all() and (cl == 0).all()
        assert list(zip(p.tolist(), q.tolist(), s_.tolist())) == want
        again = _call(s, 1.5, K)
        assert again[0] == cnt and all(x.tobytes() == y.tobytes() for x, y in zip(again[1:6], got[1:6]))
        return p, q, s_, cl
    finally:
        s.close()


def _idle(rows, count):
    """`count` pairs that are not violated at the planted rows: classes 1 .. 3 of triples of three directions (v = -2)"""
    tri = tm.first_distinct_triples(rows, count)
    return [(0, p, q, s_, 1 + e % 3) for e, (p, q, s_) in enumerate(tri)]


def test_exclusion_on_planted_rows_inside_a_tie():
    """n = 200, all rows planted: 67 * 67 * 66 pairs share v = 2 -- a tie far larger than the key buffer, closed on index digits --
    and the 50 present ones among them sit in the first 150 of the order, 20 of them at its very head; 50 more present pairs are not
    violated.  The count is the closed form minus 50, the kept list the enumeration's without them: exactly max_cuts non-present pairs."""
    n = 200
    first = tm.first_distinct_triples(list(range(n)), 150)
    violated = first[:20] + first[60:150:3]
    assert len(violated) == 50 and tm.plant_counts(n)[0] == 67 * 67 * 66
    _planted_case(n, None, violated, _idle(list(range(n)), 50), 100)


def test_exclusion_searches_64_bit_keys():
    """n = 1430 with the last 96 rows planted: every violated pair, present or not, has a packed index above 2^32"""
    n, live = BIG_N, 96
    rows = list(range(n - live, n))
    first = tm.first_distinct_triples(rows, 150)
    violated = first[:10] + first[30:150:3]
    assert len(violated) == 50
    assert min(int(cm.packed(n, p, q, s_, 0)) for p, q, s_ in violated) > 1 << 32
    p, q, s_, cl = _planted_case(n, live, violated, _idle(rows, 50), 100)
    assert (_packed(n, p, q, s_, cl) > 1 << 32).all()


def test_exclusion_of_every_violated_pair():
    """the last 6 rows planted: 8 violated pairs, all present: count 0, kept 0"""
    n, live = 200, 6
    rows = list(range(n - live, n))
    violated = tm.first_distinct_triples(rows, 100)
    assert len(violated) == 8 == tm.plant_counts(n, live)[0]
    p, *_ = _planted_case(n, live, violated, _idle(rows, 8), 100)
    assert len(p) == 0


# ---- 4. the second round

def test_second_round_on_the_solved_tightened_problem():
    """count and list against the model on the read-back factor with the present pairs removed, under eps_of's bound"""
    S = _solved("maxcut100")
    s = S["s"]
    K, minv = 300, 1e-3
    c = s.triangle_cuts(max_cuts=K, min_violation=minv)
    F, t = _factor(s), np.ones(100)
    assert c.count.tolist()[1:] == [0]
    sc = tm.Scan(F, t, minv, K + len(S["present"]))
    pp, pq, ps, pc = (np.array([getattr(x, f) for x in S["present"]], dtype=np.int64) for f in ("p", "q", "s", "cls"))
    ve, ee = tm.exact_values(F, t, pp, pq, ps, pc), tm.eps_of(F, t, pp, pq, ps)
    sc.count_hi -= int(np.count_nonzero(ve > minv - ee))   # (a present pair that may be counted as violated is not counted at all)
    sc.count_lo -= int(np.count_nonzero(ve > minv + ee))
    have = set(cm.packed(100, pp, pq, ps, pc).tolist())
    m = np.array([k not in have for k in cm.packed(100, sc.p, sc.q, sc.s, sc.c).tolist()], dtype=bool)
    sc.p, sc.q, sc.s, sc.c, sc.v = sc.p[m], sc.q[m], sc.s[m], sc.c[m], sc.v[m]
    print("second round: %d present, %d of them still violated beyond %g, count %d" % (len(have), int((ve > minv).sum()), minv, c.count[0]))
    tm.check_against_model([(F, t)], minv, K, [int(c.count[0])], c.cone, c.p, c.q, c.s, c.cls, c.violation, scans=[sc])
    assert not have & set(cm.packed(100, c.p, c.q, c.s, c.cls).tolist())
    assert len(c) > 0


# ---- 5. refusals of the device check, in the host recogniser's words

@pytest.mark.parametrize("name", ["maxcut100", "blk4x60"])
def test_device_check_refuses_what_the_host_recogniser_refuses(name):
    prob = instances.NAMED[name]()
    rng = np.random.default_rng(11)
    cuts = []
    while len(cuts) < 6:
        k = int(rng.integers(0, len(prob["blocks"])))
        p, q, s_ = sorted(rng.choice(prob["blocks"][k], 3, replace=False).tolist())
        if (k, p, q, s_) not in {x[:4] for x in cuts}:
            cuts.append((k, p, q, s_, int(rng.integers(0, 4))))
    for case, (bad, needle) in cm.malformed(tm.tightened(prob, cuts), prob["m"]).items():
        path = os.path.join(_dir(), "%s_%s.dat-s" % (name, case))
        instances.write_sdpa(bad, path)
        s = common.hip_session(path)
        try:
            with pytest.raises(ValueError) as e:
                s.present_cuts()
            why = str(e.value)
            held = _mem()
            with pytest.raises(NotImplementedError) as e1:
                s.round_pm1(trials=0)
            assert "not +-1-structured: " + why in str(e1.value), (case, why, str(e1.value))
            with pytest.raises(NotImplementedError):
                s.round_pm1(trials=8)
            rc = s.be.triangle_cuts(host.PAIR_RR, 0, 1e-3, 10)[0]
            assert rc == 2 and _last_error(s) == "triangle_cuts: the context is not +-1-structured: " + why, (case, _last_error(s))
            assert needle in why + " "
            assert _mem() == held   # (refused before any scratch was made)
            print("%s / %s: %s" % (name, case, why))
        finally:
            s.close()


# ---- 6. read-only

def test_read_only_and_memory_on_a_tightened_context():
    S = _solved("maxcut100")
    before = _mem()
    runs = []
    for look in (True, False):
        s, rho, e0 = _phase2(S["tight"], steps=0)
        try:
            a = s.admm_steps(3, rho, e0)
            if look:
                held = _mem()
                r = s.round_pm1(trials=64, seed=3, local_search_rounds=10, tol=1e-8)
                c = s.triangle_cuts(max_cuts=50)
                assert len(r.sign) == 100 and len(c) <= 50
                assert _mem()[1] > held[1]
            b = s.admm_steps(3, rho, a[0])
            mats = [s.be.get_mat(w, 0) for w in (host.MAT_R, host.MAT_U, host.MAT_V)]   # (the slacks' state shows in lambda)
            runs.append((a, b, mats + [s.be.get_vec(host.VEC_LAMBDA)]))
        finally:
            s.close()
    (a1, b1, st1), (a2, b2, st2) = runs
    assert a1 == a2 and b1 == b2
    for x, y in zip(st1, st2):
        assert np.array_equal(x, y)
    assert _mem() == before, (before, _mem())


# ---- 7. the loop

def _two_c5():
    ent = []
    for o in (0, 5):
        ent += [(0, 1, o + i + 1, o + i + 1, 0.5) for i in range(5)]
        ent += [(0, 1, o + min(i, (i + 1) % 5) + 1, o + max(i, (i + 1) % 5) + 1, -0.25) for i in range(5)]
    ent += [(i + 1, 1, i + 1, i + 1, 1.0) for i in range(10)]
    return dict(m=10, blocks=[10], b=np.ones(10), entries=ent)


def test_cut_loop_on_two_five_cycles():
    """Two 5-cycles in one cone of 10 rows, at most 4 rounds of up to 300 cuts: f_best = -8 (two maximum cuts of 4), pObj does not
    decrease from round to round beyond max(1e-6, 5 x the oracle's own gap on the round's file), and the last gap is below a tenth of
    round 0's.  (On the CPU oracle: -9.04508 = 2 x 4.52254 untightened, -8.00000 from the first tightened round on; violated
    inequalities remain between the two cycles, whose entries the objective does not see, so all 4 rounds run.)"""
    path = common.generated_instance("cutloop_two_c5", _two_c5)
    work = os.path.join(_dir(), "loop")
    before = _mem()
    hist, f_best, sign = cut_loop(path, work, 4, max_cuts=300, trials=256, seed=2)
    assert _mem() == before
    for i, h in enumerate(hist):
        print("round %d: pObj %.9f, d %.9f, f_best %.9f, gap %.3e, present %d, added %d, dropped %d, count %d"
              % (i, h.pObj, h.d, h.f_best, h.gap, h.present, h.added, h.dropped, h.count))
    assert 2 <= len(hist) <= 4 and hist[0].present == 0 and abs(hist[0].pObj + 2 * 4.52254) <= 1e-3
    assert f_best == -8.0 and sign.shape == (10,) and set(np.abs(sign).tolist()) == {1}
    for i in range(1, len(hist)):
        assert hist[i].present == hist[i - 1].present + hist[i - 1].added - hist[i - 1].dropped and hist[i].path.endswith("round%d.dat-s" % i)
        so = common.oracle_session(hist[i].path)
        try:
            ro = so.solve()
        finally:
            so.close()
        tol = max(1e-6, 5 * abs(ro["pObj"] - ro["dObj"]) / (1 + abs(ro["pObj"]) + abs(ro["dObj"])))
        assert hist[i].pObj >= hist[i - 1].pObj - tol * (1 + abs(hist[i - 1].pObj)), (i, hist[i].pObj, hist[i - 1].pObj, tol)
    assert all(h.d <= f_best + 1e-8 * max(1.0, abs(h.d)) for h in hist)   # every round's bound holds for the best point of all
    assert hist[-1].gap < hist[0].gap / 10, (hist[-1].gap, hist[0].gap)


# ---- 8. the command line on a tightened file

def test_cli_on_a_tightened_file(tmp_path):
    S = _solved("maxcut100")
    s = S["s"]
    cuts = s.triangle_cuts(max_cuts=100, min_violation=1e-3)
    want = str(tmp_path / "py.dat-s")
    s.write_tightened(want, cuts)
    out = tmp_path / "round2.dat-s"
    exe = os.path.join(host.LIB_DIR, "lorads")
    pr = subprocess.run([exe, S["tight"], "--cutsMax", "100", "--cutsFile", str(out), "--roundTrials", "64"], capture_output=True,
                        text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr
    assert "Triangle inequalities violated by more than 0.001: %d, kept %d" % (int(cuts.count.sum()), len(cuts)) in pr.stdout, pr.stdout
    assert "Hyperplane rounding (64 trials" in pr.stdout and "triangle cuts in the problem     : 300" in pr.stdout
    assert out.read_bytes() == open(want, "rb").read()
    m, blocks, _, _ = read_sdpa(str(out))
    assert (m, blocks) == (100 + 300 + len(cuts), [100, -(300 + len(cuts))])
