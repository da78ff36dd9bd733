"""Solution export on the GPU: the certificate of the exported (X, y, S) against an independent numpy computation, agreement
with the solver's own report, read-only continuation, determinism, the command line's --solutionFile."""
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.solution import read_solution
from tests import common
from tests.admm_model import read_sdpa

pytestmark = pytest.mark.gpu


def _close(got, want, tol, scale=None):
    s = max(1.0, abs(want)) if scale is None else scale
    return abs(got - want) <= tol * s


def numpy_certificate(path, sol):
    m, b, dims, ent = read_sdpa(path)
    prob = {"blocks": dims, "entries": ent}
    b = np.asarray(b, dtype=np.float64)
    S = common.slack_matrices(prob, sol.y)
    X = []
    for k, n in enumerate(dims):
        c = sol.cones[k]
        X.append(np.diag(c.x) if n < 0 else c.R @ c.R.T)
    ax = np.zeros(m)
    p = 0.0
    for mat, blk, i, j, v in ent:
        w = v * X[blk - 1][i - 1, j - 1] * (1.0 if i == j else 2.0)
        if mat == 0:
            p -= w
        else:
            ax[mat - 1] += w
    d = float(b @ sol.y)
    xs = sum(float(np.sum(S[k].toarray() * X[k])) for k in range(len(dims)))
    lam = [float(np.linalg.eigvalsh(S[k].toarray())[0]) for k in range(len(dims))]
    r = ax - b
    den = 1 + abs(p) + abs(d)
    return dict(err1=np.linalg.norm(r) / (1 + np.abs(b).sum()), err1_inf=(np.abs(r).max() if m else 0.0) / (1 + (np.abs(b).max() if m else 0.0)),
                pobj=p, dobj=d, err5=(p - d) / den, err6=xs / den, err4=max(0.0, -min(lam)) / (1 + common.c_norm1(prob)),
                lam_min=lam, S=S)


CASES = [("maxcut100", {}), ("theta30", {}), ("rand120", {}), ("blk4x60", {}), ("sdplp40", {}), ("coupledlp", {}),
         ("sdpslack30", {}), ("densea40", {}), ("densec40", {}), ("matcomp60", {"reoptLevel": 2, "phase1Tol": 1e-2})]


@pytest.mark.parametrize("name,params", CASES, ids=[c[0] for c in CASES])
def test_certificate_matches_numpy(name, params):
    path = common.instance_path(name)
    s = common.hip_session(path, **params)
    try:
        res = s.solve()
        sol = s.solution()
        want = numpy_certificate(path, sol)
        cert = sol.certificate
        assert cert["source"] == "(U+V)/2"
        assert cert["err2"] == 0.0 and cert["err3"] == 0.0
        scale = max(1.0, abs(want["pobj"]), abs(want["dobj"]))
        for k in ("err1", "err1_inf", "err5", "err6"):
            assert _close(cert[k], want[k], 1e-10), (k, cert[k], want[k])
        for k in ("pobj", "dobj"):
            assert _close(cert[k], want[k], 1e-10, scale), (k, cert[k], want[k])
        assert abs(cert["err4"] - want["err4"]) <= 1e-8, (cert["err4"], want["err4"])
        for k, c in enumerate(sol.cones):
            row, col, val = sol.slack(k)
            Sk = want["S"][k].toarray()
            assert np.all(row >= col)
            sc = max(1.0, np.abs(Sk).max())
            assert np.abs(val - Sk[row, col]).max(initial=0.0) <= 1e-12 * sc, k
            if c.is_lp:
                assert len(val) == c.n and np.array_equal(row, np.arange(c.n))
            else:
                assert c.R.shape == (c.n, s.block_info(k)["rank"])
                assert np.array_equal(c.R, (c.U + c.V) / 2)
        # units: y = lambda / scaleObjHis (the solve's closing dual-infeasibility call has stored every dual update)
        lam = s.be.get_vec(host.VEC_LAMBDA)
        assert np.array_equal(sol.y, lam / res["scale_obj_his"])
        assert cert["scale_obj_his"] == res["scale_obj_his"]
        if name == "matcomp60":
            assert res["scale_obj_his"] == 5.0
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


@pytest.mark.parametrize("name", ["maxcut100", "rand120", "blk4x60", "sdplp40"])
def test_agrees_with_admm_report(name):
    path = common.instance_path(name)
    s, rho, e0 = _phase2(path)
    try:
        e1, cg, pobj, dobj = s.admm_steps(6, rho, e0)
        sol = s.solution(tol=0)
        # every fused step refreshes both figures from R = (U+V)/2: err1 = ||A(R R^T) - b||_2 / (1 + ||b||_1) and pobj = <C, R R^T>
        # (cal_obj with the UV pair averages first).  The solver keeps A(R R^T) by a recurrence between exact refreshes, so err1 is
        # compared to 1e-12 relative or 1e-16 absolute (the rounding of the O(1) constraint values it is the difference of).
        assert sol.certificate["err1"] == pytest.approx(e1, rel=1e-12, abs=1e-16)
        assert sol.certificate["pobj"] == pytest.approx(pobj, rel=1e-12, abs=1e-12)
    finally:
        s.close()


def _state(s):
    nb = s.nblk
    mats = [s.be.get_mat(w, k) for w in (host.MAT_U, host.MAT_V) for k in range(nb)]
    return mats + [s.be.get_vec(host.VEC_LAMBDA)]


@pytest.mark.parametrize("name", ["maxcut100", "rand120", "blk4x60", "sdplp40"])
def test_read_only_continuation(name):
    path = common.instance_path(name)
    K = 5
    runs = []
    for export in (True, False):
        s, rho, e0 = _phase2(path)
        try:
            a = s.admm_steps(K, rho, e0)
            if export:
                sol1 = s.solution()
                sol2 = s.solution()
                c1, c2 = sol1.certificate, sol2.certificate
                for k in ("err1", "err1_inf", "err4", "err5", "err6", "pobj", "dobj", "xs"):
                    assert np.array_equal(np.float64(c1[k]), np.float64(c2[k])), k  # determinism
                assert np.array_equal(sol1.y, sol2.y)
            b = s.admm_steps(K, rho, a[0])
            runs.append((a, b, _state(s)))
        finally:
            s.close()
    (a1, b1, st1), (a2, b2, st2) = runs
    assert a1 == a2 and b1 == b2
    for x, y in zip(st1, st2):
        assert np.array_equal(x, y)
    # after a whole solve (whose closing dual-infeasibility call has already stored the dual update)
    runs = []
    for export in (True, False):
        s = common.hip_session(path)
        try:
            s.solve()
            if export:
                s.solution()
            res = s.results()
            rho = min(res["admm_rho"], 5000.0)
            out = s.admm_steps(K, rho, res["constrVio1"])
            runs.append((out, _state(s)))
        finally:
            s.close()
    assert runs[0][0] == runs[1][0]
    for x, y in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(x, y)


def test_headline_size():
    import scipy.sparse as sp
    prob = instances.randsparse(20000, 5000, 3)
    d = os.path.join(os.environ.get("TMPDIR", "/tmp"), "lorads_cert_rand20000_%d.dat-s" % os.getpid())
    instances.write_sdpa(prob, d)
    try:
        s = common.hip_session(d, timesLogRank=4.0)
        try:
            s.alm_to_admm()
            s.be.init_constr(host.PAIR_UV)
            e0 = s.be.update_dimacs(host.PAIR_UV)
            s.admm_steps(3, 1.0, e0)
            sol = s.solution(tol=0)
        finally:
            s.close()
        m, b, dims, ent = read_sdpa(d)
        R = sol.cones[0].R
        assert R.shape[1] == 40
        e = np.array([(mat, i - 1, j - 1, v) for mat, blk, i, j, v in ent])
        mat, ii, jj, vv = e[:, 0].astype(int), e[:, 1].astype(int), e[:, 2].astype(int), e[:, 3]
        dots = np.einsum("ij,ij->i", R[ii], R[jj]) * np.where(ii == jj, 1.0, 2.0)
        ax = np.bincount(mat[mat > 0] - 1, weights=(vv * dots)[mat > 0], minlength=m)
        p = -float(np.sum((vv * dots)[mat == 0]))
        S = common.slack_matrices(prob, sol.y)[0]
        Sl = sp.tril(S).tocoo()
        xs = float(np.sum(Sl.data * np.einsum("ij,ij->i", R[Sl.row], R[Sl.col]) * np.where(Sl.row == Sl.col, 1.0, 2.0)))
        bb = np.asarray(b)
        dd = float(bb @ sol.y)
        cert = sol.certificate
        assert _close(cert["err1"], np.linalg.norm(ax - bb) / (1 + np.abs(bb).sum()), 1e-10)
        assert _close(cert["pobj"], p, 1e-10)
        assert _close(cert["err6"], xs / (1 + abs(p) + abs(dd)), 1e-10)
    finally:
        os.remove(d)


def test_cli_solution_file(tmp_path):
    path = common.instance_path("maxcut100")
    exe = os.path.join(host.LIB_DIR, "lorads")
    out = tmp_path / "sol.txt"
    plain = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    withf = subprocess.run([exe, path, "--solutionFile", str(out)], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and withf.returncode == 0, withf.stderr
    keep = lambda t: [ln for ln in t.splitlines() if not ln.startswith("phase 1:") and "Time" not in ln and " s " not in ln]  # noqa: E731
    assert keep(plain.stdout) == keep(withf.stdout)[:len(keep(plain.stdout))]
    assert "Certificate of the exported solution" in withf.stdout
    sol = read_solution(out)
    s = common.hip_session(path)
    try:
        s.solve()
        mine = s.solution()
        s.write_solution(tmp_path / "py.txt")
    finally:
        s.close()
    assert (tmp_path / "py.txt").read_bytes() == out.read_bytes()
    assert np.array_equal(sol.y, mine.y)
    assert np.array_equal(sol.cones[0].R, mine.cones[0].R)
