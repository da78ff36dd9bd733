"""Spectrum and rank reduction of the solution factors on the GPU (lorads_amd/csrc/hip/spectral.inc) against
numpy on the read-back factors: eigenvalues and eigenvectors, every rank shape, the pure rotation, truncation and the ADMM steps
after it, phase 1, read-only / deterministic / owned, the one-launch paths after a reduction, the command line, and the two caps
of the Gram's row strips (n > 65536; a large rank).

u = 2^-53.  bound1 = 2 (n + 8 sweeps) rl u lambda_1: a dot of length n carries at most n u lambda_1, an eigenvalue moves by at most
rl max|dG|, numpy's own Gram carries the same, and the Jacobi part is 8 sweeps m u lambda_1 (tests/test_spectral_model.py)."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.rounding import read_rounding
from lorads_amd.solution import read_solution
from tests import common
from tests import rounding_model as rm
from tests.admm_model import read_sdpa
from tests.test_solution import _close, numpy_certificate

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GOLDEN = {os.path.basename(f)[:-6] for f in os.listdir(common.GOLD) if f.endswith(".dat-s")}


def _path(name):
    return common.instance_path(name) if name in GOLDEN else common.generated_instance(name)


def _factor(s, k, src):
    if src == host.PAIR_UV:
        return (s.be.get_mat(host.MAT_U, k) + s.be.get_mat(host.MAT_V, k)) / 2
    return s.be.get_mat(host.MAT_R, k)


def _lp(s):
    return s._lp_blocks()


def check_spectrum(s, src, tag):
    """check 1 of the issue on the session's current state; returns the worst achieved ratios (eigenvalues, orthogonality, residual)"""
    rc, lam, sweeps, Q = s.be.spectrum(src, vectors=True)
    assert rc == 0
    worst = [0.0, 0.0, 0.0]
    for k in range(s.nblk):
        if _lp(s)[k]:
            assert len(lam[k]) == 0 and sweeps[k] == 0
            continue
        F = _factor(s, k, src)
        n, rl = F.shape
        assert lam[k].shape == (rl,) and Q[k].shape == (rl, rl)
        G = F.T @ F
        want = np.linalg.eigvalsh(G)[::-1]
        l1 = max(want[0], np.finfo(float).tiny)
        m = rl + (rl & 1)
        assert 1 <= sweeps[k] <= 30, (tag, k, sweeps[k])
        b1 = 2 * (n + 8 * sweeps[k]) * rl * U * l1
        bq = 8 * sweeps[k] * m * U
        e = np.abs(lam[k] - want).max()
        o = np.abs(Q[k].T @ Q[k] - np.eye(rl)).max()
        r = np.abs(G @ Q[k] - Q[k] * lam[k]).max()
        print("%s cone %d (n %d, rl %d): %d sweeps, |dlam| %.2e (%.3f of bound), |QtQ - I| %.2e (%.3f), |GQ - QL| %.2e (%.3f)"
              % (tag, k, n, rl, sweeps[k], e, e / b1, o, o / bq, r, r / b1))
        assert np.all(np.diff(lam[k]) <= 0), (tag, k)
        assert e <= b1, (tag, k, e, b1)
        assert o <= bq, (tag, k, o, bq)
        assert r <= b1, (tag, k, r, b1)
        worst = [max(worst[0], e / b1), max(worst[1], o / bq), max(worst[2], r / b1)]
    return worst


SOLVED = ["maxcut100", "theta30", "theta50", "rand120", "blk4x60", "mix4", "sdplp40", "densea40", "densec40"]


@pytest.mark.parametrize("name", SOLVED)
def test_spectrum_after_solve_against_numpy(built, name):
    s = common.hip_session(_path(name))
    try:
        s.solve()
        check_spectrum(s, host.PAIR_UV, name)
        got = s.spectrum()
        _, lam, _, _ = s.be.spectrum(host.PAIR_UV)
        for a, b in zip(got, lam):
            assert np.array_equal(a, b)
    finally:
        s.close()


def _random_state(s, seed):
    Us, Vs, lam = common.random_uv_state(s, seed)
    common.load_uv_state(s.be, Us, Vs, lam)


@pytest.mark.parametrize("name", ["maxcut100", "rand120", "blk4x60", "sdplp40", "densec40"])
def test_spectrum_of_random_states_against_numpy(built, name):
    """full-rank spectra (a solved point's is usually deficient)"""
    s = common.hip_session(_path(name))
    try:
        _random_state(s, 17)
        check_spectrum(s, host.PAIR_UV, name + " random")
        # ... and of R alone
        check_spectrum(s, host.PAIR_RR, name + " random R")
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


@pytest.mark.parametrize("r", [1, 2, 9, 17, 40, 64, 65])
def test_rank_shapes(built, r):
    path = _path("rand120")
    s = common.hip_session(path, **_rank_params(path, r))
    try:
        cur = s.block_shape(0)[1]
        assert cur <= r
        if cur != r:
            s.be.resize_rank([r])
        assert s.block_shape(0)[1] == r
        _random_state(s, 100 + r)
        check_spectrum(s, host.PAIR_UV, "rand120 r=%d" % r)
    finally:
        s.close()


@pytest.mark.parametrize("name", ["densec300", "densea300", "denseac200", "mix4", "blkmix5", "blk16var"])
def test_dense_and_unequal_cones(built, name):
    """dense-storage cones at their own ranks; unequal cones that share a device rank (the spectrum is of the cone's OWN rank:
    blkmix5 stands at ranks 9 .. 12, blk16var -- 16 cones of n = 2000 .. 5750 -- at 16 .. 18; mix4's four cones share rank 9)"""
    s = common.hip_session(_path(name))
    try:
        _random_state(s, 5)
        check_spectrum(s, host.PAIR_UV, name)
    finally:
        s.close()


def test_rank_258_through_resize(built):
    path = _path("densec40")
    s = common.hip_session(path, **_rank_params(path, 258))
    try:
        if s.block_shape(0)[1] != 258:
            s.be.resize_rank([258])
        _random_state(s, 258)
        check_spectrum(s, host.PAIR_UV, "densec40 r=258")   # (n = 40 < rl: 218 eigenvalues at zero)
    finally:
        s.close()


def test_headline_size(built):
    prob = instances.randsparse(20000, 5000, 3)
    d = os.path.join(os.environ.get("TMPDIR", "/tmp"), "lorads_spec_rand20000_%d.dat-s" % os.getpid())
    instances.write_sdpa(prob, d)
    try:
        s = common.hip_session(d, timesLogRank=4.0)
        try:
            assert s.block_shape(0) == (20000, 40)
            s.alm_to_admm()
            s.be.init_constr(host.PAIR_UV)
            e0 = s.be.update_dimacs(host.PAIR_UV)
            s.admm_steps(3, 1.0, e0)
            check_spectrum(s, host.PAIR_UV, "rand20000 r=40")
        finally:
            s.close()
    finally:
        os.remove(d)


# ------------------------------------------------------------------ the two caps of the Gram's row strips
# Up to n = 65536 a strip has 256 rows.  Above it the cap of SPEC_MAX_STRIPS strips makes them 320, 384, ... rows: a wavefront's quarter
# of 80 and more no longer starts on a 64-row boundary.  At a large rank SPEC_PART_CAP (the doubles of Gram partials) allows fewer
# strips than that, and the strips grow at a far smaller n.


def _spec_inc(name):
    text = open(os.path.join(common.ROOT, "lorads_amd", "csrc", "hip", "spectral.inc")).read()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(?:\(size_t\))?\s*(\d+)(?:\s*<<\s*(\d+))?\s*;" % name, text)
    return int(m.group(1)) << int(m.group(2) or 0)


SPEC_MAX_STRIPS, SPEC_PART_CAP, SPEC_MAXR = (_spec_inc(k) for k in ("SPEC_MAX_STRIPS", "SPEC_PART_CAP", "SPEC_MAXR"))


def gram_strips(n, rl):
    """(strip cap by SPEC_PART_CAP, strips, rows_per_strip) of spec_run and postsolve.inc's row_strips, restated"""
    T = -(-rl // 16)
    npairs = T * (T + 1) // 2
    cap = SPEC_PART_CAP // (npairs * 256)
    s = max(1, min(SPEC_MAX_STRIPS, cap, -(-n // 256)))
    rps = max(64, (-(-n // s) + 63) & ~63)
    return cap, max(1, -(-n // rps)), rps


def test_the_restated_strips():
    assert (SPEC_MAX_STRIPS, SPEC_PART_CAP, SPEC_MAXR) == (256, 4 << 20, 512)
    assert gram_strips(20000, 40)[1:] == (79, 256) and gram_strips(65536, 20)[1:] == (256, 256)
    assert gram_strips(66000, 20) == (SPEC_PART_CAP // (3 * 256), 207, 320)
    assert gram_strips(40, 258)[0] == 107 and gram_strips(7937, 497) == (31, 25, 320)


_BIG = {}


def _sdplp66000(r):
    """the context of one SDP cone of 66000 rows at rank r (and an LP block of 66000 columns), kept for the module"""
    s = _BIG.get(r)
    if s is None:
        path = common.generated_instance("spec_sdplp66000", lambda: instances.sdp_lp(66000, 132000, 0, 66))
        s = _BIG[r] = common.hip_session(path, timesLogRank=1e-3)
        assert s.block_shape(0) == (66000, 1)
        s.be.resize_rank([r, 1])
    assert s.block_shape(0) == (66000, r) and _lp(s) == [False, True]
    return s


def teardown_module(module):
    for s in _BIG.values():
        s.close()
    _BIG.clear()


def test_strips_of_320_rows(built):
    """n = 66000: 207 strips of 320 rows.  A random state through check_spectrum as it stands, then a factor whose columns have
    disjoint supports and entries +-1: every partial Gram is a diagonal of integer counts, no rotation is due, and the eigenvalues
    must be the column counts exactly.  Cheap: two Grams of 66000 x 20 and an eigen-solve of order 20."""
    t0 = time.perf_counter()
    n, r = 66000, 20
    assert gram_strips(n, r)[1:] == (207, 320) and n > 256 * SPEC_MAX_STRIPS
    s = _sdplp66000(r)
    _random_state(s, 66)
    worst = check_spectrum(s, host.PAIR_UV, "sdplp66000 r=%d" % r)
    print("sdplp66000 r=%d: worst ratios %.3g, %.3g, %.3g" % ((r,) + tuple(worst)))
    rng = np.random.default_rng(67)
    col = rng.permutation(np.repeat(np.arange(r), np.arange(1, r + 1)))[np.arange(n) % (r * (r + 1) // 2)]   # column j: ~ (j + 1) / 210 of the rows
    F = np.zeros((n, r))
    F[np.arange(n), col] = rng.choice([-1.0, 1.0], n)
    D = rng.integers(-5, 6, (n, r)).astype(np.float64)
    s.be.set_mat(host.MAT_U, 0, F + D)
    s.be.set_mat(host.MAT_V, 0, F - D)
    counts = np.bincount(col, minlength=r).astype(np.float64)
    assert counts.sum() == n and len(set(counts.tolist())) == r
    rc, lam, sweeps, Q = s.be.spectrum(host.PAIR_UV, vectors=True)
    assert rc == 0
    print("sdplp66000 disjoint columns: %d sweeps, eigenvalues %s" % (sweeps[0], lam[0][:4]))
    assert sweeps[0] == 1   # (a diagonal Gram: the first sweep rotates nothing)
    assert np.array_equal(lam[0], np.sort(counts)[::-1])
    order = np.argsort(-counts, kind="stable")
    assert np.array_equal(Q[0], np.eye(r)[:, order])   # (and the vectors are the unit vectors of those columns)
    print("sdplp66000: %.2f s" % (time.perf_counter() - t0))


def _smallest_part_cap_case():
    """the smallest n, and the smallest rank at it, at which SPEC_PART_CAP and not SPEC_MAX_STRIPS sets the number of strips"""
    best = None
    for rl in range(1, SPEC_MAXR + 1):
        cap = gram_strips(1, rl)[0]
        if cap >= SPEC_MAX_STRIPS:
            continue
        n = 256 * cap + 1   # the smallest n with ceil(n / 256) > cap
        if best is None or n < best[0]:
            best = (n, rl)
    return best


def test_strips_capped_by_the_partials(built):
    """rank 497 (32 rank tiles, 528 tile pairs) leaves 31 strips; n = 7937 asks for 32.  Cheap for its size: a factor of 3.9 M
    numbers and one eigen-solve of order 498 in the scratch."""
    t0 = time.perf_counter()
    n, r = _smallest_part_cap_case()
    cap, strips, rps = gram_strips(n, r)
    print("SPEC_PART_CAP binds first at n %d, rank %d: at most %d strips, %d of %d rows" % (n, r, cap, strips, rps))
    assert (n, r) == (7937, 497)
    assert min(SPEC_MAX_STRIPS, cap) < -(-n // 256) and cap < SPEC_MAX_STRIPS and rps > 256
    path = common.generated_instance("spec_maxcut%d" % n, lambda: instances.maxcut(n, 2 * n, n))
    s = _open_at_ranks(path, [r])
    try:
        _random_state(s, r)
        worst = check_spectrum(s, host.PAIR_UV, "maxcut%d r=%d" % (n, r))
        print("maxcut%d r=%d: worst ratios %.3g, %.3g, %.3g; %.2f s" % ((n, r) + tuple(worst) + (time.perf_counter() - t0,)))
    finally:
        s.close()


def _rotation_bound(sweeps, rl):
    return 2 * 8 * sweeps * rl * U + 4 * rl * U


@pytest.mark.parametrize("name", ["maxcut100", "theta30", "rand120", "blk4x60", "sdplp40", "densec40", "densea40"])
def test_rotation_keeps_x(built, name):
    path = _path(name)
    s = common.hip_session(path)
    try:
        s.solve()
        nb, lp = s.nblk, _lp(s)
        F = [_factor(s, k, host.PAIR_UV) for k in range(nb)]
        ranks = [s.block_shape(k)[1] for k in range(nb)]
        rep = s.compress_rank(ranks=ranks)
        assert [c["rank_after"] for c in rep["cones"]] == ranks
        for k in range(nb):
            R, Um, Vm = (s.be.get_mat(w, k) for w in (host.MAT_R, host.MAT_U, host.MAT_V))
            if lp[k]:
                continue
            assert np.array_equal(R, Um) and np.array_equal(R, Vm)
            n, rl = F[k].shape
            assert R.shape == (n, rl)
            c = rep["cones"][k]
            lam, sw = c["eig"], c["sweeps"]
            l1 = max(np.linalg.eigvalsh(F[k].T @ F[k])[-1], np.finfo(float).tiny)
            b1 = 2 * (n + 8 * sw) * rl * U * l1
            G2 = R.T @ R
            off = np.abs(G2 - np.diag(np.diag(G2))).max(initial=0.0)
            dn = np.abs(np.diag(G2) - lam).max()
            X0, X1 = F[k] @ F[k].T, R @ R.T
            dx = np.linalg.norm(X1 - X0) / np.linalg.norm(X0)
            print("%s cone %d: off-diagonal %.2e, norms %.2e of bound %.2e; |X' - X|_F / |X|_F %.2e of %.2e"
                  % (name, k, off, dn, b1, dx, _rotation_bound(sw, rl)))
            assert off <= b1 and dn <= b1
            assert dx <= _rotation_bound(sw, rl)
        sol = s.solution()
        want = numpy_certificate(path, sol)
        cert = sol.certificate
        scale = max(1.0, abs(want["pobj"]), abs(want["dobj"]))
        for key in ("err1", "err1_inf", "err5", "err6"):
            assert _close(cert[key], want[key], 1e-10), (key, cert[key], want[key])
        for key in ("pobj", "dobj"):
            assert _close(cert[key], want[key], 1e-10, scale), (key, cert[key], want[key])
    finally:
        s.close()


def _c_norms(path):
    m, b, dims, ent = read_sdpa(path)
    out = [0.0] * len(dims)
    for mat, blk, i, j, v in ent:
        if mat == 0:
            out[blk - 1] += v * v * (1.0 if i == j else 2.0)
    return [np.sqrt(x) for x in out]


def _truncate_and_continue(name, tol, params, strict_k):
    """check 4 of the issue: returns (ranks before, ranks after, err1 before, err1 after the reduction, err1 after 10 steps)"""
    path = _path(name)
    s = common.hip_session(path, **params)
    try:
        res = s.solve()
        nb, lp = s.nblk, _lp(s)
        F = [_factor(s, k, host.PAIR_UV) for k in range(nb)]
        rep = s.compress_rank(tol=tol)
        cn = _c_norms(path)
        room = 0.0
        for k in range(nb):
            if lp[k]:
                continue
            n, rl = F[k].shape
            c = rep["cones"][k]
            kk = c["rank_after"]
            lam = np.linalg.eigvalsh(F[k].T @ F[k])[::-1]
            lo, hi = int(np.sum(lam > 4 * tol * lam[0])), int(np.sum(lam > tol * lam[0] / 4))
            pred = np.sqrt(np.sum(lam[kk:] ** 2) / np.sum(lam ** 2))
            print("%s cone %d: rank %d -> %d (numpy bracket %d..%d), sweeps %d, ||X - X_k|| / ||X|| %.3e (numpy %.3e), trace lost %.3e"
                  % (name, k, rl, kk, lo, hi, c["sweeps"], c["frob_lost"], pred, c["trace_lost"]))
            assert max(1, lo) <= kk <= max(1, hi), (name, k, lo, kk, hi)
            if strict_k:
                assert kk < rl, (name, k, kk, rl)
            assert abs(c["frob_lost"] - pred) <= max(1e-10 * pred, 4 * rl * U), (c["frob_lost"], pred)
            assert s.block_shape(k) == (n, kk)
            xn = np.sqrt(np.sum(lam ** 2))
            room += cn[k] * (pred * xn + _rotation_bound(c["sweeps"], rl) * xn)
        dp = abs(rep["pobj_after"] - rep["pobj_before"])
        print("%s: pobj %.12e -> %.12e (moved %.3e, room %.3e), err1 %.3e -> %.3e" % (name, rep["pobj_before"], rep["pobj_after"], dp, room,
                                                                                  rep["err1_before"], rep["err1_after"]))
        assert dp <= room, (dp, room)
        rho = min(res["admm_rho"], 5000.0)
        e1, cg, pobj, dobj = s.admm_steps(10, rho, rep["err1_after"])
        print("%s: err1 after 10 ADMM steps at rho %.4g: %.3e (%.3f x before the reduction), %d CG iterations"
              % (name, rho, e1, e1 / rep["err1_before"], cg))
        assert cg > 0
        assert np.isfinite(e1) and np.isfinite(pobj)
        before = [c["rank_before"] for c in rep["cones"]]
        after = [c["rank_after"] for c in rep["cones"]]
        return before, after, rep["err1_before"], rep["err1_after"], e1
    finally:
        s.close()


@pytest.mark.parametrize("name", ["theta30", "theta50", "rand120", "matcomp60"])
def test_truncation_at_1e_12(built, name):
    before, after, e_before, _, e10 = _truncate_and_continue(name, 1e-12, {}, strict_k=True)
    if name != "matcomp60":
        assert e10 <= 2 * e_before, (e10, e_before)


def test_truncation_maxcut800_at_1e_8(built):
    _truncate_and_continue("maxcut800", 1e-8, dict(timesLogRank=6.0), strict_k=True)


@pytest.mark.parametrize("name,params", [("maxcut100", dict(timesLogRank=4.0)), ("blk4x60", {})])
def test_truncation_at_1e_4(built, name, params):
    before, after, e_before, _, e10 = _truncate_and_continue(name, 1e-4, params, strict_k=False)
    assert sum(after) < sum(before), (before, after)
    assert e10 <= 2 * e_before, (e10, e_before)


@pytest.mark.parametrize("name", ["theta30", "rand120", "blk4x60"])
def test_phase_one_state(built, name):
    path = _path(name)
    with common.hip_session(path) as ref:
        want = ref.solve()
    s = common.hip_session(path)
    try:
        s.alm()
        R0 = [s.be.get_mat(host.MAT_R, k) for k in range(s.nblk)]
        rep = s.compress_rank()
        assert rep["src"] == host.PAIR_RR
        for k in range(s.nblk):
            lam = np.linalg.eigvalsh(R0[k].T @ R0[k])[::-1]
            kk = rep["cones"][k]["rank_after"]
            assert int(np.sum(lam > 4e-12 * lam[0])) <= kk <= int(np.sum(lam > 0.25e-12 * lam[0]))
        got = s.solve()
        print("%s: status %d / %d, pObj %.10e / %.10e" % (name, got["status"], want["status"], got["pObj"], want["pObj"]))
        assert got["status"] == want["status"]
        assert abs(got["pObj"] - want["pObj"]) <= 5e-4 * max(1.0, abs(want["pObj"]))
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


def _state(s):
    mats = [s.be.get_mat(w, k) for w in (host.MAT_R, host.MAT_U, host.MAT_V) for k in range(s.nblk)]
    return mats + [s.be.get_vec(host.VEC_LAMBDA)]


@pytest.mark.parametrize("name", ["maxcut100", "rand120", "blk4x60", "sdplp40"])
def test_read_only_and_deterministic(built, name):
    path = _path(name)
    K = 5
    runs = []
    for look in (True, False):
        s, rho, e0 = _phase2(path)
        try:
            a = s.admm_steps(K, rho, e0)   # (its last dual update still waits for a carrier)
            if look:
                x, y = s.spectrum(), s.spectrum()
                for p, q in zip(x, y):
                    assert np.array_equal(p, q)
                rc1, l1, sw1, q1 = s.be.spectrum(host.PAIR_UV, vectors=True)
                rc2, l2, sw2, q2 = s.be.spectrum(host.PAIR_UV, vectors=True)
                assert rc1 == 0 and rc2 == 0 and sw1 == sw2 and all(np.array_equal(p, q) for p, q in zip(l1 + q1, l2 + q2))
            b = s.admm_steps(K, rho, a[0])
            runs.append((a, b, _state(s)))
        finally:
            s.close()
    (a1, b1, st1), (a2, b2, st2) = runs
    assert a1 == a2 and b1 == b2
    for x, y in zip(st1, st2):
        assert np.array_equal(x, y)


def _mem():
    d = host.Session.hip_memory_stats()
    return (d["device_allocations"], d["device_bytes"], d["pinned_allocations"], d["pinned_bytes"])


@pytest.mark.parametrize("name", ["rand120", "sdplp40", "blk4x60"])
def test_refusals_and_ownership(built, name):
    before = _mem()
    s, rho, e0 = _phase2(_path(name))
    try:
        s.admm_steps(3, rho, e0)
        lp = _lp(s)
        ranks = [s.block_shape(k)[1] for k in range(s.nblk)]
        st0 = _state(s)
        held = _mem()
        bad = []
        for k in range(s.nblk):
            if lp[k]:
                bad.append([2 if j == k else r for j, r in enumerate(ranks)])   # LP block != 1
                bad.append([0 if j == k else r for j, r in enumerate(ranks)])
            else:
                bad.append([0 if j == k else r for j, r in enumerate(ranks)])   # rank 0
                bad.append([r + 1 if j == k else r for j, r in enumerate(ranks)])   # above the current rank
                bad.append([-3 if j == k else r for j, r in enumerate(ranks)])
        for nr in bad:
            rc, _ = s.be.compress_rank(host.PAIR_UV, nr)
            assert rc not in (0, 3), (nr, rc)
            assert [s.block_shape(k)[1] for k in range(s.nblk)] == ranks
            assert _mem() == held, nr
            with pytest.raises(RuntimeError):
                s.compress_rank(ranks=nr)
        for x, y in zip(st0, _state(s)):
            assert np.array_equal(x, y)
        assert _mem() == held
        # the state is still whole: a reduction goes through and the iteration runs on
        rep = s.compress_rank(tol=1e-6)
        assert _mem()[1] > before[1]
        e1, cg, _, _ = s.admm_steps(3, rho, rep["err1_after"])
        assert cg > 0 and np.isfinite(e1)
    finally:
        s.close()
    assert _mem() == before, (before, _mem())


def test_sharded_refusal(built):
    s = common.hip_session(_path("blk4x60"), world=2, rank=0, separable=True)
    try:
        held = _mem()
        with pytest.raises(NotImplementedError, match="sharded"):
            s.spectrum()
        with pytest.raises(NotImplementedError, match="sharded"):
            s.compress_rank()
        assert s.be.spectrum(host.PAIR_UV)[0] == 3
        ranks = [s.block_shape(k)[1] for k in range(s.nblk)]
        assert s.be.compress_rank(host.PAIR_UV, ranks)[0] == 3
        assert _mem() == held   # (refused before any device work: not even the scratch was made)
    finally:
        s.close()


@pytest.mark.parametrize("name,r", [("rand120", 9), ("densec40", 258)], ids=["lds", "scratch"])
def test_a_factor_that_is_not_finite_is_refused(built, name, r):
    """a NaN (a diverged solve) reaches ||G||_F: code 4 and a message, not a result and not an undefined sort"""
    path = _path(name)
    s = common.hip_session(path, **_rank_params(path, r))
    try:
        if s.block_shape(0)[1] != r:
            s.be.resize_rank([r])
        _random_state(s, 3)
        Um = s.be.get_mat(host.MAT_U, 0)
        Um[3, r // 2] = np.nan
        s.be.set_mat(host.MAT_U, 0, Um)
        assert s.be.spectrum(host.PAIR_UV)[0] == 4
        lib, _ = s._hip()
        lib.lorads_hip_last_error.restype = C.c_char_p
        assert b"not finite" in lib.lorads_hip_last_error()
        assert s.be.compress_rank(host.PAIR_UV, [r])[0] == 4
        assert s.block_shape(0)[1] == r
        Um[3, r // 2] = 0.25
        s.be.set_mat(host.MAT_U, 0, Um)
        check_spectrum(s, host.PAIR_UV, "%s r=%d after the NaN was removed" % (name, r))
    finally:
        s.close()


def test_two_contexts_with_different_lds_needs(built):
    """the dynamic-LDS allowance belongs to the kernel, not to a context: a small cone's call must not take it from a large one's"""
    path = _path("rand120")
    a = common.hip_session(path, **_rank_params(path, 65))
    b = common.hip_session(path)
    try:
        if a.block_shape(0)[1] != 65:
            a.be.resize_rank([65])
        _random_state(a, 1)
        _random_state(b, 2)
        for s, tag in ((a, "a"), (b, "b"), (a, "a again"), (b, "b again")):
            check_spectrum(s, host.PAIR_UV, "two contexts, " + tag)
    finally:
        a.close()
        b.close()


def test_session_reduction_refuses_a_stale_rank_record(built):
    """Backend.resize_rank goes past the host: Session.compress_rank, whose buffers the host's record sizes, refuses"""
    s = common.hip_session(_path("rand120"))
    try:
        r = s.block_shape(0)[1]
        s.be.resize_rank([r + 3])
        _random_state(s, 4)
        with pytest.raises(RuntimeError, match="stale"):
            s.compress_rank()
        lam = s.spectrum()   # (sized by the device's ranks)
        assert lam[0].shape == (r + 3,)
        rc, eig = s.be.compress_rank(host.PAIR_UV, [r])
        assert rc == 0 and eig[0].shape == (r + 3,) and s.block_shape(0)[1] == r
    finally:
        s.close()


def _open_at_ranks(path, ranks):
    """a fresh session whose cones stand at `ranks`: opened below them by the rank rule, grown by resize_rank"""
    s = common.hip_session(path, **_rank_params(path, min(ranks)))
    cur = [s.block_shape(k)[1] for k in range(s.nblk)]
    assert all(c <= r for c, r in zip(cur, ranks)), (cur, ranks)
    if cur != list(ranks):
        s.be.resize_rank(list(ranks))
    assert [s.block_shape(k)[1] for k in range(s.nblk)] == list(ranks)
    return s


@pytest.mark.parametrize("name,params,tol", [("maxcut800", {}, 1e-6), ("blk4x60", {}, 1e-4), ("rand120", {}, 1e-12), ("matcomp60", {}, 1e-12)])
def test_one_launch_paths_after_a_reduction(built, name, params, tol):
    """ten ADMM steps after a reduction against the same ten from the read-back state in a FRESH session opened at that rank: a stale
    plan, captured graph or recurrence over freed arrays would differ by orders, or fault.  The cap (two below the smallest rank) makes
    every cone's shape change whatever the spectrum of the unconverged point is."""
    path = _path(name)
    s, rho, e0 = _phase2(path, **params)
    try:
        s.admm_steps(12, rho, e0)
        rep = s.compress_rank(tol=tol, max_rank=min(s.block_shape(k)[1] for k in range(s.nblk)) - 2)
        ranks = [c["rank_after"] for c in rep["cones"]]
        assert all(c["rank_after"] < c["rank_before"] for c in rep["cones"])
        print("%s: ranks %s -> %s" % (name, [c["rank_before"] for c in rep["cones"]], ranks))
        Us = [s.be.get_mat(host.MAT_U, k) for k in range(s.nblk)]
        Vs = [s.be.get_mat(host.MAT_V, k) for k in range(s.nblk)]
        lam = s.be.get_vec(host.VEC_LAMBDA)
        a = s.admm_steps(10, rho, rep["err1_after"])
    finally:
        s.close()
    f = _open_at_ranks(path, ranks)
    try:
        common.load_uv_state(f.be, Us, Vs, lam)
        f.be.cal_obj(host.PAIR_UV)
        e = f.be.update_dimacs(host.PAIR_UV)
        print("%s: err1 of the loaded state %.17g, after the reduction %.17g" % (name, e, rep["err1_after"]))
        assert abs(e - rep["err1_after"]) <= 1e-9 * abs(rep["err1_after"])
        b = f.admm_steps(10, rho, e)
    finally:
        f.close()
    print("%s: after the reduction %r, fresh session %r" % (name, a, b))
    assert abs(a[1] - b[1]) <= 1, (a, b)
    for x, y in ((a[0], b[0]), (a[2], b[2]), (a[3], b[3])):   # err1, pobj, dobj to 1e-9 relative
        assert abs(x - y) <= 1e-9 * abs(y), (a, b)


def test_cli(built, tmp_path):
    exe = os.path.join(host.LIB_DIR, "lorads")
    path = _path("theta30")
    out = tmp_path / "sol.txt"
    p = subprocess.run([exe, path, "--compressTol", "1e-12", "--solutionFile", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert "Rank reduction of the solution:" in p.stdout and "block 1: sdp 30, rank" in p.stdout
    assert p.stdout.index("Rank reduction of the solution:") < p.stdout.index("Certificate of the exported solution")
    sol = read_solution(out)
    R = sol.cones[0].R
    line = [ln for ln in open(out).read().splitlines() if ln.startswith("sdp 1 30 ")][0]
    k = int(line.split()[3])
    plain = common.hip_session(path)
    try:
        rl = plain.block_shape(0)[1]
    finally:
        plain.close()
    assert R.shape == (30, k) and 1 <= k < rl, (k, rl)
    G = R.T @ R
    assert np.abs(G - np.diag(np.diag(G))).max() <= 2 * (30 + 8 * 30) * rl * U * np.diag(G).max()
    assert np.all(np.diff(np.diag(G)) <= 0)
    # the rounding after a reduction works on the reduced factor
    mc = _path("maxcut100")
    sf, rf = tmp_path / "mc_sol.txt", tmp_path / "mc_round.txt"
    p = subprocess.run([exe, mc, "--compressTol", "1e-4", "--solutionFile", str(sf), "--roundTrials", "64", "--roundLocalSearch", "0",
                        "--roundFile", str(rf)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert "Rank reduction of the solution:" in p.stdout and "Hyperplane rounding (64 trials" in p.stdout
    R = read_solution(sf).cones[0].R
    got = read_rounding(rf)
    P = rm.Pm1Problem.read(mc)
    sigma = got.cones[0].sigma
    assert sigma.shape == (100,) and set(np.unique(sigma)) <= {-1, 1}   # a valid +-1 point: x = sigma o t is feasible for every sigma
    Gh = rm.hyperplanes(0, 0, R.shape[1], 64)
    sig, proj = rm.signs(R, Gh)
    near = np.any(np.abs(proj) <= 1e-12 * np.linalg.norm(R, axis=1)[:, None] * np.linalg.norm(Gh, axis=0)[None, :], axis=0)
    f = rm.objective(P.C[0], P.t[0], sig)
    assert not near[got.best]
    assert np.array_equal(sig[:, got.best], sigma)
    assert abs(got.f_best - f[got.best]) <= 1e-13 * max(1.0, abs(f[got.best]))
    assert f[got.best] <= f[~near].min() + 1e-13 * max(1.0, abs(f[got.best]))
