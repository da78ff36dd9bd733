"""The dual side of the device path -- the slack eigen-solve (csrc/hip/lanczos.inc) and the certificate (csrc/hip/solution.inc) --
against the model of tests/dual_model.py, at the edges of their kernels.

Every case sets a seeded state (set_mat, set_vec(VEC_LAMBDA), resize_rank on a session opened at timesLogRank = 1e-3) and runs no
solve.  The slack of most eigen-solve cases is prescribed entry for entry (instances.prescribed_slack), so its spectrum is known.

Bounds (none is taken from the device).
  lam_min      |theta_dev - theta_model(longdouble)| <= max(32 spread, 1e-14) ||S||_2, spread = the difference between the model in
               float64 and in longdouble on that case, relative to ||S||_2 (the rule of tests/test_one_launch_variants.py)
  matvecs      equal to the model's wherever the two precisions of the model agree on it (tests/test_dual_model.py recomputes the
               table: they agree on every edge size and closed-form case here, so no case is exempt from the count)
  sums         <C, X>, <S, X>, b . lambda, every A(X)_i - b_i and ||A(X) - b||_2^2: max(32 spread, 1e-14) times the model's sum of
               the absolute values of the terms; err1_inf, ||b||_inf and the LP minimum pick one element: exact.  The device returns
               the norm, not its square: squaring what a square root returned adds up to 4 eps ||.||^2, which the bound on the
               squared norm carries on top
  slack        every entry of get_slack to 1e-15 (|C_e| + sum_i |lambda_i a_i|)

Every test prints the ratio of each device error to its bound ("RATIO group value case") before it asserts; MEASURED (below) holds
the worst ratio per group of cases on the MI355X.  The nearest any case came to its bound is 0.94 of it, and all ratios above 0.3
belong to one kind of case: ncv = 2 (0.52 to 0.94) and ncv = 3 (0.40) at tol 1e-10 on the edge sizes from 255 on, which spend the
whole budget of 600 restarts.  A thick restart carries theta into the next projected matrix, so each restart adds its rounding: the
bound there is the 1e-14 ||S||_2 floor or a tenth above it, and the measured 1.0e-14 ||S||_2 is 0.08 eps ||S||_2 per restart.
Every other eigen-solve case stays below 0.3, every certificate sum and residual below 0.09.

Durations on the MI355X (`--durations=0`, setup + call + teardown; the models run inside the cases): 10.7 s for the file.
Per test function, all its cases together, and its slowest case:
  test_edge_sizes                                      5.7 s   1.67 s  [2047]
  test_dense_storage                                   1.2 s   0.80 s  [dense730]
  test_certificate_dense_and_other_kinds               0.9 s   0.68 s  [dense730]
  test_closed_form_spectra                             1.0 s   0.61 s  [clustered120]
  test_certificate_pattern_stride                      0.5 s   0.53 s  -
  test_more_cones_than_workers                         0.3 s   0.13 s  [eleven]
  test_certificate_lp_and_several_cones                0.2 s   0.12 s  [eleven]
  test_rows_with_an_empty_adjacency                    0.1 s   0.10 s  -
  test_eigen_solve_leaves_the_admm_state_alone         0.2 s   0.06 s  [mix4]
  test_certificate_ranks                               0.4 s   0.05 s  [1-maxcut100]
  test_cone_with_an_empty_pattern                      0.0 s   0.04 s  -
  test_lp_blocks                                       0.0 s   0.02 s  [sdplp200]
  test_certificate_with_a_pending_dual_update          0.0 s   0.02 s  -
  test_eigen_solve_leaves_the_phase1_state_alone       0.0 s   0.02 s  [rand120]
  test_restart_budget_exit                             0.0 s   0.01 s  [0]"""
import numpy as np
import pytest

from lorads_amd import host, instances
from tests import common
from tests import dual_cases as dc
from tests import dual_model as dm

pytestmark = pytest.mark.gpu

RR, UV = host.PAIR_RR, host.PAIR_UV
LD = dm.LD

# group: (worst error / bound measured on the MI355X, the case it was measured on)
MEASURED = {
    'edge sizes': (0.939, 'edge255 cone 0 ncv 2 tol 1e-10'),
    'closed-form spectra': (0.234, 'clustered120 cone 0 ncv 3 tol 1e-10'),
    'budget exit': (0.02, 'rand120/3 cone 0 ncv 9 tol 1e-10'),
    'empty rows': (0.0469, 'emptyrows70 cone 0 ncv 9 tol 1e-10'),
    'empty pattern': (0.0312, 'emptycone cone 0 ncv 3 tol 1e-10'),
    'slack entries': (0.284, 'denseac200 cone 0'),
    'dense storage': (0.0451, 'denseac200 cone 0 ncv 40 tol 1e-10'),
    'LP blocks': (0.0342, 'sdplp20 cone 0 ncv 40 tol 1e-10'),
    'several cones': (0.0812, 'mix4 cone 3 ncv 40 tol 1e-10'),
    'certificate ranks': (0.087, 'maxcut100 r 1 {} src 0 lam_min cone 0'),
    'certificate strides': (0.0351, 'rand4000 src 1 residual vector'),
    'certificate dense': (0.0499, 'densec300 src 0 lam_min cone 0'),
    'certificate LP': (0.05, 'sdplp20 positive src 0 lam_min cone 0'),
}


def _note(group, err, bound, case):
    """prints the ratio of a device error to its bound (what MEASURED is filled from)"""
    ratio = 0.0 if err == 0.0 else (float("inf") if bound == 0.0 else float(err) / float(bound))
    print("RATIO %s %.3g %s" % (group, ratio, case))
    return ratio


def _bound(spread, scale):
    """max(32 spread, 1e-14) scale with the spread given in absolute terms"""
    return max(32.0 * float(spread), 1e-14 * float(scale))


def _open(path, ranks=None, env=None):
    s = common.hip_session_with_env(path, env or {}, dict(timesLogRank=1e-3))
    if ranks is not None:
        s.be.resize_rank([ranks] * s.nblk if isinstance(ranks, int) else ranks)
    return s


_probs = {}


def _prob(path):
    """the instance of a file, parsed once per test process"""
    if path not in _probs:
        _probs[path] = dm.problem(path)
    return _probs[path]


def _norm2(Sl):
    """||S||_2 of a model slack: float64 eigenvalues of the model's own matrix (0 for the zero matrix); for a large sparse cone the
    extreme Ritz value of ARPACK, which lies inside the spectrum -- never more than ||S||_2, so never a wider bound"""
    if Sl.is_lp:
        return float(np.abs(Sl.diagonal()).max(initial=0.0))
    if Sl.n > 2100:
        import scipy.sparse as sp
        import scipy.sparse.linalg as sla
        off = Sl.row != Sl.col
        v = Sl.val.astype(np.float64)
        A = sp.csr_matrix((np.concatenate([v, v[off]]), (np.concatenate([Sl.row, Sl.col[off]]), np.concatenate([Sl.col, Sl.row[off]]))),
                          shape=(Sl.n, Sl.n))
        return float(abs(sla.eigsh(A, k=1, which="LM", tol=1e-6, return_eigenvectors=False)[0]))
    ev = np.linalg.eigvalsh(Sl.dense().astype(np.float64))
    return float(max(abs(ev[0]), abs(ev[-1])))


def _slacks(prob_or_path, lam):
    """per cone: (the longdouble slack, the float64 slack, ||S||_2)"""
    prob = _prob(prob_or_path) if isinstance(prob_or_path, str) else prob_or_path
    return [(a, b, _norm2(a)) for a, b in zip(dm.slack(prob, lam, LD), dm.slack(prob, lam, np.float64))]


def _models(slacks, ncv, tols, max_restarts=600):
    """per cone (None for an LP block): ({tol: result} longdouble, {tol: result} float64, ||S||_2, the longdouble slack)"""
    out = []
    for a, b, nrm in slacks:
        if a.is_lp:
            out.append((None, None, nrm, a))
        else:
            out.append((dm.lanczos(a, tols, ncv, max_restarts, LD), dm.lanczos(b, tols, ncv, max_restarts, np.float64), nrm, a))
    return out


def _check_eigs(group, case, s, prob_or_path, lam, ncvs, tols, max_restarts=600):
    """hip_dual_infeasibility against the model for every (ncv, tol): lam_min per cone, the product count, the returned sum.
    Returns {(ncv, tol): (device result, model results)}."""
    got, slacks = {}, _slacks(prob_or_path, lam)
    for ncv in ncvs:
        mods = _models(slacks, ncv, tols, max_restarts)
        for tol in tols:
            tot, lmin, nmv = s.hip_dual_infeasibility(tol, ncv, max_restarts)
            want_nmv, agree, sdp_sum, lp_sum, lp_mag, lp_cols = 0, True, 0.0, LD(0), 0.0, 0
            for k, (ld, f64, nrm, Sl) in enumerate(mods):
                if ld is None:
                    assert lmin[k] == 0.0
                    d = Sl.diagonal()
                    lp_sum += np.abs(np.minimum(d, 0)).sum()
                    lp_mag += float(Sl.mag[np.asarray(Sl.val < 0)].sum())
                    lp_cols += Sl.n
                    continue
                a, b = ld[tol], f64[tol]
                bound = _bound(abs(a.theta - b.theta), nrm)
                err = abs(lmin[k] - a.theta)
                _note(group, err, bound, "%s cone %d ncv %d tol %g: dev %.17g model %.17g (matvecs %d, %d restarts%s)" % (
                    case, k, ncv, tol, lmin[k], a.theta, a.matvecs, a.restarts, ", breakdown" if a.breakdown else ""))
                assert err <= bound, (case, k, ncv, tol, lmin[k], a, b, bound)
                want_nmv += a.matvecs
                agree = agree and a.matvecs == b.matvecs
                sdp_sum += abs(min(lmin[k], 0.0))
            if agree:
                assert nmv == want_nmv, (case, ncv, tol, "S x products", nmv, want_nmv)
            # the sum: the SDP cones' shares are the device's own lam_min, added in block order -- without an LP block the same
            # bits.  The LP columns' shares: each to the rounding of its entry (1e-15 of the terms' magnitudes), and any order of
            # adding N non-negative terms errs by at most (N - 1) eps times the sum.
            if lp_cols == 0:
                assert tot == sdp_sum, (case, ncv, tol, tot, sdp_sum)
            else:
                lp_bound = 1e-15 * lp_mag + lp_cols * dm.EPS * float(lp_sum) + 2 * dm.EPS * (sdp_sum + float(lp_sum))
                assert abs(tot - sdp_sum - float(lp_sum)) <= lp_bound, (case, ncv, tol, tot, sdp_sum, float(lp_sum))
            got[(ncv, tol)] = ((tot, lmin, nmv), mods)
    return got


def _generated(name, make):
    """a generated instance's file; the model takes the generator's own entries (the file holds their repr: the same values)"""
    if name not in _made:
        prob = make()
        _made[name] = common.generated_instance(name, make=lambda: prob)
        _probs[_made[name]] = dm.problem(prob)
    return _made[name]


_made = {}


def _prescribed(name, S):
    return _generated("dual_" + name, lambda: instances.prescribed_slack(S)), -np.diag(S)


# ---------------------------------------------------------------- eigen-solve: edge sizes
@pytest.mark.parametrize("n", dc.EDGE_SIZES)
def test_edge_sizes(built, n):
    """every ncv of NCVS (keep below and at its cap, m = n against m = ncv, the pinned / unpinned read-back at 126 / 127) at both
    tolerances; n <= ncv ends with the breakdown at j = n - 1 after exactly n products"""
    S = dc.edge_matrix(n)
    path, lam = _prescribed("edge%d" % n, S)
    s = _open(path)
    try:
        assert s.block_shape(0) == (n, 1) and s.hip_block_image(0)["n"] == n
        s.be.set_vec(host.VEC_LAMBDA, lam)
        row, col, val = s.hip_get_slack(0)
        # the objective (the off-diagonal part) is stored dense above 0.1 n (n + 1) / 2 entries: the tiny sizes; from n = 31 on the
        # pattern holds everything and k_spmv carries the whole product.  get_slack is S itself (the whole triangle of a dense cone).
        nc = np.count_nonzero(np.triu(S, 1))
        im = s.hip_block_image(0)
        assert im["dense_a"] == 0, im
        if n >= 31:
            assert im["dense_c"] == 0 and nc <= 0.1 * n * (n + 1) / 2, im
        assert np.array_equal(val, S[row, col]) and len(val) == (n * (n + 1) // 2 if im["dense_c"] else nc + n)
        got = _check_eigs("edge sizes", "edge%d" % n, s, path, lam, dc.NCVS, dc.TOLS)
        for (ncv, tol), ((tot, lmin, nmv), mods) in got.items():
            r = mods[0][0][tol]
            if n <= ncv:   # m = n: the Krylov space is everything
                assert r.breakdown and r.matvecs == n and nmv == n, (n, ncv, tol, r, nmv)
            else:
                assert r.m == ncv and nmv >= ncv
    finally:
        s.close()


# ---------------------------------------------------------------- eigen-solve: closed-form spectra
CLOSED = dc.closed_form()


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_form_spectra(built, name):
    S, steps = CLOSED[name]
    n = S.shape[0]
    path, lam = _prescribed(name, S)
    ev = np.linalg.eigvalsh(S)
    s = _open(path)
    try:
        s.be.set_vec(host.VEC_LAMBDA, lam)
        got = _check_eigs("closed-form spectra", name, s, path, lam, dc.NCVS, dc.TOLS)
        nrm = max(abs(ev[0]), abs(ev[-1]))
        for (ncv, tol), ((tot, lmin, nmv), mods) in got.items():
            r = mods[0][0][tol]
            m = min(ncv, n)
            if steps is not None and ncv >= steps:
                # the breakdown at j = steps - 1 ran (matvecs < m says so whenever steps < m), and the value is lambda_min
                assert r.breakdown and r.matvecs == steps
                assert nmv == steps and (steps == m or nmv < m), (name, ncv, tol, nmv)
                assert abs(lmin[0] - ev[0]) <= 64 * n * dm.EPS * nrm, (name, ncv, tol, lmin[0], ev[0])
            if name in ("plus3I_50", "minus3I_50", "zero_50"):
                assert nmv == 1 and lmin[0] == ev[0]
                assert tot == (3.0 if name == "minus3I_50" else 0.0)
            if name == "gram90x6" and not r.breakdown:
                # lambda_min = 0 (multiplicity 84): the stop rule's floor eps^(2/3) is what ends the run, or the budget
                assert r.res <= tol * dm.EPS23 or r.restarts == 600
            if name == "clustered120" and (ncv, tol) == (9, 1e-10):
                assert r.restarts == 600 and not r.breakdown and nmv == 9 + 600   # the budget exit: m + max_restarts (m - keep)
    finally:
        s.close()


# ---------------------------------------------------------------- eigen-solve: budget exit, empty rows
def _rand_lam(m, seed=5):
    return np.random.default_rng(seed).standard_normal(m)


@pytest.mark.parametrize("max_restarts", [0, 3])
def test_restart_budget_exit(built, max_restarts):
    path = common.instance_path("rand120")
    s = _open(path)
    try:
        lam = _rand_lam(s.m)
        s.be.set_vec(host.VEC_LAMBDA, lam)
        for ncv in (3, 9, 12):   # (at ncv = 40 the first sweep already meets 1e-10 on this slack: no budget exit)
            got = _check_eigs("budget exit", "rand120/%d" % max_restarts, s, path, lam, [ncv], [1e-10], max_restarts=max_restarts)
            (tot, lmin, nmv), mods = got[(ncv, 1e-10)]
            r = mods[0][0][1e-10]
            keep = min(8, ncv - 1)
            assert r.restarts == max_restarts and not r.breakdown and r.res > 1e-10 * max(dm.EPS23, abs(r.theta)), r  # the budget ended it
            assert nmv == ncv + max_restarts * (ncv - keep)
    finally:
        s.close()


def test_rows_with_an_empty_adjacency(built):
    """three rows (the first, the last, one inside) that no entry of C or of any A_i touches: k_spmv's rows without neighbours.
    With lambda = 0 the slack is C, positive definite on the other rows: lambda_min = 0 comes from the empty rows alone."""
    rows = [0, 33, 69]
    make = lambda: instances.randsparse_untouched_rows(70, 25, 2301, rows, c_edges=100, n_diag=2, n_off=3, r0=3)  # noqa: E731
    prob = make()
    assert not any(i - 1 in rows or j - 1 in rows for _, _, i, j, _ in prob["entries"])
    path = _generated("dual_emptyrows70", make)
    s = _open(path)
    try:
        assert s.hip_block_image(0)["n"] == 70
        for lam in (_rand_lam(s.m), np.zeros(s.m)):
            s.be.set_vec(host.VEC_LAMBDA, lam)
            row, col, val = s.hip_get_slack(0)
            assert not np.isin(row, rows).any() and not np.isin(col, rows).any()
            got = _check_eigs("empty rows", "emptyrows70", s, path, lam, [9, 40, 127], dc.TOLS)
            if not lam.any():
                for (ncv, tol), ((tot, lmin, nmv), mods) in got.items():
                    if tol == 1e-10:
                        assert abs(lmin[0]) <= 1e-10 * dm.EPS23 + 64 * 70 * dm.EPS * mods[0][2] and tot <= abs(lmin[0])
    finally:
        s.close()


def _with_empty_cone():
    p = instances.maxcut(20, 30, 2351)
    return dict(m=p["m"], blocks=[20, 5], b=p["b"], entries=p["entries"])


def test_cone_with_an_empty_pattern(built):
    """a cone that no entry of C or of any A_i touches (pu.ne = 0): k_spmv then reads the row pointers alone -- every array it is
    handed is allocated (DevPool allocates at least one element, build_adjacency n + 1 pointers) and none of the others is
    dereferenced.  Its slack is the zero matrix: one product, the breakdown at j = 0, lambda_min = 0, no share in any sum."""
    path = _generated("dual_emptycone", _with_empty_cone)
    s = _open(path)
    try:
        assert s.nblk == 2 and s.hip_block_image(1)["pattern_union"] == 0 and s.hip_block_image(1)["n"] == 5
        lam = _rand_lam(s.m)
        s.be.set_vec(host.VEC_LAMBDA, lam)
        got = _check_eigs("empty pattern", "emptycone", s, path, lam, [3, 40], dc.TOLS)
        for (ncv, tol), ((tot, lmin, nmv), mods) in got.items():
            assert lmin[1] == 0.0 and mods[1][0][tol].matvecs == 1 and mods[1][0][tol].breakdown
        R, U, V = _factors(s, 13)
        common.load_r_state(s.be, R, lam)
        _check_certificate("empty pattern", "emptycone", s, path, RR, R, lam, tol=1e-2)
    finally:
        s.close()


# ---------------------------------------------------------------- eigen-solve: dense storage, LP blocks, many cones
def _dense730():
    return instances.with_dense_constraints(instances.randsparse(730, 5, 2311, n_diag=2, n_off=3, r0=2, dense_c=True), 1, 2312)


DENSE = {
    "densec40": (None, 1, 0), "densea40": (None, 1, 3),   # (densea40: 100 entries of C against 82)
     "denseac200": (None, 1, 3), "densec300": (None, 1, 0),
    "dense730": (_dense730, 1, 1),                                                              # npad^2 = 736^2 > 2048 x 256
    "densec65": (lambda: instances.randsparse(65, 10, 2313, n_diag=1, n_off=2, r0=2, dense_c=True), 1, 0),
}
GOLDEN = {"densec40", "densea40", "rand120", "maxcut100", "blk4x60", "mix4", "theta30", "matcomp60", "sdplp40"}


def _path(name, make=None):
    if make is None:
        return common.instance_path(name) if name in GOLDEN else common.generated_instance(name)
    return _generated("dual_" + name, make)


@pytest.mark.parametrize("name", sorted(DENSE))
def test_dense_storage(built, name):
    make, dense_c, dense_a = DENSE[name]
    path = _path(name, make)
    s = _open(path)
    try:
        im = s.hip_block_image(0)
        assert im["dense_c"] == dense_c and im["dense_a"] == dense_a, im
        lam = _rand_lam(s.m)
        s.be.set_vec(host.VEC_LAMBDA, lam)
        _check_eigs("dense storage", name, s, path, lam, [40], dc.TOLS)
    finally:
        s.close()


def _lp_with_an_empty_column():
    """sdp_lp(20, 30, 3) whose last LP column has neither a cost nor a row: the LP pattern holds 22 of the 23 columns (pu.ne < n)"""
    p = instances.sdp_lp(20, 30, 3, 2322)
    return dict(p, entries=[e for e in p["entries"] if not (e[1] == 2 and e[2] == 23)])


LP_CASES = {"sdplp200": (lambda: instances.sdp_lp(200, 400, 150, 2321), 350), "sdplp20": (lambda: instances.sdp_lp(20, 30, 3, 2322), 23),
            "sdplp20gap": (_lp_with_an_empty_column, 23)}


@pytest.mark.parametrize("name", sorted(LP_CASES))
def test_lp_blocks(built, name):
    """the LP share of the sum (k_lp_dual) against the model, column by column through get_slack"""
    make, ncol = LP_CASES[name]
    path = _path(name, make)
    s = _open(path)
    try:
        assert s.nblk == 2 and s.block_shape(1) == (ncol, 1)
        lam = _rand_lam(s.m)
        s.be.set_vec(host.VEC_LAMBDA, lam)
        got = _check_eigs("LP blocks", name, s, path, lam, [40], dc.TOLS)
        (tot, lmin, nmv), mods = got[(40, 1e-10)]
        Sl = mods[1][3]
        row, col, val = s.hip_get_slack(1)
        assert np.array_equal(row, np.arange(ncol)) and np.array_equal(row, col)
        want, mag = Sl.diagonal(), np.zeros(ncol)
        mag[Sl.row] = Sl.mag
        err = np.abs(val - want.astype(np.float64))
        _note("slack entries", float((err / np.maximum(mag, 1e-300)).max()), 1e-15, name + " LP block")
        assert np.all(err <= 1e-15 * mag), (name, float(err.max()))
        assert (val < 0).any() and (val > 0).any()   # both branches of |min(s_j, 0)|
        share = tot - abs(min(lmin[0], 0.0))
        own = float(np.abs(np.minimum(val, 0.0)).sum())
        assert abs(share - own) <= (ncol + 2) * dm.EPS * own, (share, own)   # (any order of adding ncol non-negative terms)
    finally:
        s.close()


def _eleven():
    """eleven small cones of different sizes and kinds: more cones than the eight worker threads"""
    return instances.block_diag([
        instances.maxcut(20, 30, 2331), instances.randsparse(33, 12, 2332, c_edges=50, n_diag=2, n_off=3, r0=2),
        instances.matcomp(12, 11, 60, 2, 2333), instances.theta(15, 20, 2334), instances.maxcut(41, 70, 2335),
        instances.randsparse(26, 9, 2336, n_diag=1, n_off=2, r0=2, dense_c=True), instances.maxcut(9, 12, 2337),
        instances.randsparse(64, 20, 2338, c_edges=120, n_diag=2, n_off=3, r0=3), instances.maxcut(3, 2, 2339),
        instances.with_dense_constraints(instances.randsparse(24, 8, 2340, c_edges=40, n_diag=1, n_off=2, r0=2), 2, 2341),
        instances.maxcut(57, 100, 2342)])


@pytest.mark.parametrize("name", ["eleven", "blk4x60", "mix4"])
def test_more_cones_than_workers(built, monkeypatch, name):
    path = _path(name, _eleven if name == "eleven" else None)
    runs = []
    for threads in (None, "1"):
        if threads:
            monkeypatch.setenv("LORADS_LANCZOS_THREADS", threads)
        s = _open(path)
        try:
            if name == "eleven":
                assert s.nblk == 11
            lam = _rand_lam(s.m)
            s.be.set_vec(host.VEC_LAMBDA, lam)
            if threads is None:
                _check_eigs("several cones", name, s, path, lam, [40], dc.TOLS)
            a = s.hip_dual_infeasibility(1e-10, 40, 600)
            b = s.hip_dual_infeasibility(1e-10, 40, 600)
            assert a == b, "two calls in one session differ"
            runs.append(a)
        finally:
            s.close()
    assert runs[0] == runs[1], "LORADS_LANCZOS_THREADS=1 differs from the default"


# ---------------------------------------------------------------- certificate
def _key(row, col, n):
    return np.asarray(row, dtype=np.int64) * n + np.asarray(col, dtype=np.int64)


def _check_slack(case, s, slacks):
    """get_slack of every cone against the model, entry by entry at 1e-15 (|C_e| + sum_i |lambda_i a_i|); an entry of a dense cone
    outside the model's pattern is exactly zero"""
    vals = []
    for k, Sl in enumerate(slacks):
        row, col, val = s.hip_get_slack(k)
        assert np.all(row >= col)
        mk = _key(Sl.row, Sl.col, Sl.n)
        dk = _key(row, col, Sl.n)
        assert len(np.unique(dk)) == len(dk) and np.isin(mk, dk).all(), (case, k, "the model's entries are not all exported")
        pos = np.searchsorted(mk, dk)
        hit = (pos < len(mk)) & (mk[np.minimum(pos, len(mk) - 1)] == dk) if len(mk) else np.zeros(len(dk), dtype=bool)
        want, mag = np.zeros(len(dk), dtype=LD), np.zeros(len(dk))
        want[hit], mag[hit] = Sl.val[pos[hit]], Sl.mag[pos[hit]]
        err = np.abs((val.astype(LD) - want).astype(np.float64))
        if len(err):
            _note("slack entries", float((err[mag > 0] / mag[mag > 0]).max(initial=0.0)), 1e-15, "%s cone %d" % (case, k))
        assert np.all(err <= 1e-15 * mag), (case, k, float(err.max(initial=0.0)))
        vals.append(val)
    return vals


def _check_certificate(group, case, s, path, src, F, lam, tol=1e-8, ncv=40):
    """hip_certificate against the model at the factors F (per block; an LP block's column r gives x = r^2)"""
    prob = _prob(path)
    m, b, dims = prob["m"], prob["b"], prob["blocks"]
    R = [None if n < 0 else F[k] for k, n in enumerate(dims)]
    x = {k: F[k][:, 0] ** 2 for k, n in enumerate(dims) if n < 0}
    out, lmin, res, lamc = s.hip_certificate(src, tol, ncv, 600)
    assert np.array_equal(lamc, lam), (case, "the certificate's multipliers")
    a, c64 = dm.certificate(prob, R, x, lam, LD), dm.certificate(prob, R, x, lam, np.float64)
    for key, got, absk in (("cx", out[2], "cx_abs"), ("sx", out[4], "sx_abs"), ("bl", out[3], "bl_abs"), ("nrm2sq", out[7] ** 2, "nrm2sq")):
        bound = _bound(abs(a[key] - c64[key]), a[absk]) + (4 * dm.EPS * float(a[absk]) if key == "nrm2sq" else 0.0)  # (+ sqrt and square)
        err = abs(float(LD(got) - a[key]))
        _note(group, err, bound, "%s src %d %s: dev %.17g model %.17g" % (case, src, key, got, float(a[key])))
        assert err <= bound, (case, src, key, got, float(a[key]), bound)
    rb = np.maximum(32.0 * np.abs((a["res"] - c64["res"]).astype(np.float64)), 1e-14 * a["res_abs"].astype(np.float64))
    rerr = np.abs((res.astype(LD) - a["res"]).astype(np.float64))
    if m:
        _note(group, float((rerr / np.maximum(rb, 1e-300)).max()), 1.0, "%s src %d residual vector" % (case, src))
    assert np.all(rerr <= rb), (case, src, "A(X) - b", float((rerr / np.maximum(rb, 1e-300)).max()))
    # the figures that pick one element, and the divisions
    bb = np.asarray(b, dtype=np.float64)
    assert out[8] == np.abs(res).max(initial=0.0) and out[9] == np.abs(bb).max(initial=0.0) == a["binf"]
    assert out[1] == out[8] / (1 + out[9])
    assert abs(out[0] - out[7] / (1 + np.abs(bb).sum())) <= 8 * dm.EPS * out[0]
    # the slack and lambda_min per cone; the LP block's is min_j s_j over the exported values (0 at most where a column has no entry)
    vals = _check_slack(case, s, dm.slack(prob, lam, LD))
    tot, lmin_di, nmv_di = s.hip_dual_infeasibility(tol, ncv, 600)
    mods = _models(_slacks(prob, lam), ncv, [tol])
    want_nmv, agree = 0, True
    for k, (ld, f64, nrm, Sl) in enumerate(mods):
        if ld is None:
            assert lmin[k] == vals[k].min() and len(vals[k]) == Sl.n, (case, k, lmin[k])
            continue
        r, r64 = ld[tol], f64[tol]
        bound = _bound(abs(r.theta - r64.theta), nrm)
        _note(group, abs(lmin[k] - r.theta), bound, "%s src %d lam_min cone %d" % (case, src, k))
        assert abs(lmin[k] - r.theta) <= bound, (case, k, lmin[k], r)
        assert lmin[k] == lmin_di[k], (case, k, lmin[k], lmin_di[k])   # the same slack, the same process: the eigen-solve entry's bits
        want_nmv += r.matvecs
        agree = agree and r.matvecs == r64.matvecs
    assert out[5] == min(lmin)
    if agree:
        assert out[6] == want_nmv == nmv_di, (case, out[6], nmv_di, want_nmv)
    return out, lmin, res


def _factors(s, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(s.nblk):
        n, r = s.block_shape(k)
        out.append([rng.standard_normal((n, r)) / np.sqrt(max(r, 1)) for _ in range(3)])
    return [f[0] for f in out], [f[1] for f in out], [f[2] for f in out]


def _both_sources(group, case, s, path, lam, seed=9, tol=1e-8, ncv=40):
    """src = R on a phase-1 state, then src = (U + V) / 2 on an ADMM state of the same session"""
    R, U, V = _factors(s, seed)
    common.load_r_state(s.be, R, lam)
    _check_certificate(group, case, s, path, RR, R, lam, tol, ncv)
    common.load_uv_state(s.be, U, V, lam)
    _check_certificate(group, case, s, path, UV, [(u + v) / 2 for u, v in zip(U, V)], lam, tol, ncv)


RANKS = [1, 2, 3, 16, 18, 41, 130]   # scalar path (odd, unpadded); r / 2 beyond the eight lanes of cert_row_dot from 18 on


@pytest.mark.parametrize("name", ["rand120", "maxcut100"])
@pytest.mark.parametrize("r", RANKS)
def test_certificate_ranks(built, name, r):
    path = _path(name)
    for env in [{}] + ([{"LORADS_PAD_ODD_RANK": "0"}] if r % 2 else []):
        s = _open(path, ranks=r, env=env)
        try:
            # (the block image reports the logical rank, with or without the pad column, and the ABI exposes no padded rank: that the
            # unpadded run takes cert_row_dot's scalar path rests on the library reading LORADS_PAD_ODD_RANK when the context is
            # created, which hip_session_with_env arranges)
            assert s.block_shape(0)[1] == r and s.hip_block_image(0)["rank"] == r
            assert s.m < 256   # (few constraints: k_cert_close in one trip)
            _both_sources("certificate ranks", "%s r %d %s" % (name, r, env), s, path, _rand_lam(s.m))
        finally:
            s.close()


def test_certificate_pattern_stride(built):
    """rand4000, state set, not solved: more than 32768 union-pattern entries (k_cert_pat's second trip, k_cert_fin over 1024
    partials), m = 1000 (k_cert_close's stride)"""
    path = _path("rand4000")
    s = _open(path, ranks=4)
    try:
        im = s.hip_block_image(0)
        assert im["pattern_union"] > 32768 and s.m == 1000 and im["rank"] == 4, im
        _both_sources("certificate strides", "rand4000", s, path, _rand_lam(s.m), tol=1e-2)
    finally:
        s.close()


@pytest.mark.parametrize("name", ["densec300", "denseac200", "dense730", "densea40", "theta30", "matcomp60"])
def test_certificate_dense_and_other_kinds(built, name):
    """k_cert_dot at its 256-workgroup cap (npad > 256), the strides of k_cert_gram and k_dense_combine (n = 730), the
    per-constraint dots of dense A_i; and the slack of every other cone kind"""
    path = _path(name, DENSE[name][0] if name in DENSE else None)
    s = _open(path, ranks=3)
    try:
        if name in DENSE:
            im = s.hip_block_image(0)
            assert (im["dense_c"], im["dense_a"]) == DENSE[name][1:], im
        _both_sources("certificate dense", name, s, path, _rand_lam(s.m), tol=1e-2)
    finally:
        s.close()


@pytest.mark.parametrize("name", sorted(LP_CASES) + ["sdplp40", "eleven"])
def test_certificate_lp_and_several_cones(built, name):
    """k_cert_min over 350 and 23 values and get_slack of the LP block; the pu.ne < n clamp of lam_min on both sides: with every
    column in the pattern a positive minimum is returned as it is, with a column that has no entry (s_j = 0) it is clamped to 0"""
    path = _path(name, LP_CASES[name][0] if name in LP_CASES else _eleven if name == "eleven" else None)
    s = _open(path, ranks=None)
    try:
        lam = _rand_lam(s.m)
        _both_sources("certificate LP", name, s, path, lam, tol=1e-2)
        if name in LP_CASES:
            # multipliers that make every stored LP slack positive: min_j s_j over the pattern is what k_cert_min returns
            lam2 = -np.abs(lam)
            R, U, V = _factors(s, 10)
            common.load_r_state(s.be, R, lam2)
            out, lmin, res = _check_certificate("certificate LP", name + " positive", s, path, RR, R, lam2, tol=1e-2)
            row, col, val = s.hip_get_slack(1)
            if name == "sdplp20gap":
                assert s.hip_block_image(1)["pattern_union"] == 22 and val[22] == 0.0 and np.all(val[:22] > 0) and lmin[1] == 0.0
            else:
                assert s.hip_block_image(1)["pattern_union"] == len(val) and lmin[1] == val.min() > 0
    finally:
        s.close()


def test_certificate_with_a_pending_dual_update(built):
    """after an admm_step and a dual update that waits for a carrier, the certificate's multipliers are the updated ones (applied to
    a copy) and equal, bit for bit, what get_vec(VEC_LAMBDA) stores afterwards"""
    path = _path("rand120")
    s = _open(path, ranks=4)
    try:
        R, U, V = _factors(s, 12)
        lam = _rand_lam(s.m)
        common.load_uv_state(s.be, U, V, lam)
        rho = 1.5
        s.be.admm_step(rho, 0.0, 3)
        lam0, csum = s.be.get_vec(host.VEC_LAMBDA), s.be.get_vec(host.VEC_CONSTR_SUM)
        Ud, Vd = s.be.get_mat(host.MAT_U, 0), s.be.get_mat(host.MAT_V, 0)
        assert np.array_equal(lam0, lam)
        n0 = s.hip_launch_count()
        s.be.update_dual_var(rho)
        assert s.hip_launch_count() == n0   # it waits for a carrier: one cone that sees every constraint
        out, lmin, res, lamc = s.hip_certificate(UV, 1e-2, 40, 600)
        lam1 = s.be.get_vec(host.VEC_LAMBDA)
        assert np.array_equal(lamc, lam1)
        bb = _prob(path)["b"]
        want = lam0.astype(LD) + LD(rho) * (bb.astype(LD) - csum.astype(LD))
        scale = np.abs(lam0) + rho * (np.abs(bb) + np.abs(csum))
        assert not np.array_equal(lam1, lam0)
        assert np.all(np.abs((lamc.astype(LD) - want).astype(np.float64)) <= 4 * dm.EPS * scale)
        # ... and the certificate is the one of those multipliers at the step's factors
        _check_certificate("certificate ranks", "rand120 pending", s, path, UV, [(Ud + Vd) / 2], lam1, tol=1e-2)
    finally:
        s.close()


# ---------------------------------------------------------------- the eigen-solve leaves the solver's state alone
def _state(s):
    nb = s.nblk
    return [s.be.get_mat(w, k) for w in (host.MAT_U, host.MAT_V) for k in range(nb)] + \
        [s.be.get_vec(host.VEC_LAMBDA), s.be.get_vec(host.VEC_CONSTR_SUM)]


STATE_CASES = [("rand120", {"LORADS_OP_CW": "0"}), ("rand120", {"LORADS_OP_CW": "1"}), ("theta30", {}), ("maxcut100", {}),
               ("maxcut100", {"LORADS_PERSIST": "0"}), ("matcomp60", {}), ("densea40", {}), ("densec40", {}), ("sdplp40", {}), ("mix4", {})]


@pytest.mark.parametrize("name,env", STATE_CASES, ids=["%s%s" % (n, "".join("-%s=%s" % kv for kv in e.items())) for n, e in STATE_CASES])
def test_eigen_solve_leaves_the_admm_state_alone(built, name, env):
    """three admm_steps, hip_dual_infeasibility (which assembles the slack into the cone's own pattern values and dense scratch),
    three more steps: U, V, lambda, the constraint sums and every returned scalar are the bits of the same six steps without it"""
    path = _path(name)
    rho, runs = 1.5, []
    for call in (True, False):
        s = common.hip_session_with_env(path, env, {})
        try:
            U, V, lam = common.random_uv_state(s, 5)
            common.load_uv_state(s.be, U, V, lam)
            outs = []
            for i in range(6):
                if i == 3 and call:
                    tot, lmin, nmv = s.hip_dual_infeasibility()
                    assert nmv > 0 and np.isfinite(tot)
                outs.append(s.be.admm_step(rho, 1e-6, 8))
                s.be.update_dual_var(rho)
            runs.append((outs, _state(s)))
        finally:
            s.close()
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for x, y in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["rand120", "densea40"])
def test_eigen_solve_leaves_the_phase1_state_alone(built, name):
    """alm_front / alm_step around the call: R, the gradient, lambda, the constraint sums and the returned scalars"""
    path = _path(name)
    rho, runs = 0.5, []
    for call in (True, False):
        s = common.hip_session_with_env(path, {}, {})
        try:
            R, lam = common.random_r_state(s, 6)
            common.load_r_state(s.be, R, lam)
            be = s.be
            outs = [be.alm_cal_grad(rho)]
            front = be.alm_front(rho, 0)
            for i in range(4):
                if i == 2 and call:
                    tot, lmin, nmv = s.hip_dual_infeasibility()
                    assert nmv > 0 and np.isfinite(tot)
                tau = common.linesearch_tau(front[2])[0]
                o = be.alm_step(rho, tau, i + 1)
                front = (o[2], o[3], o[4])
                outs.append((tau, o))
            st = [be.get_mat(w, k) for w in (host.MAT_R, host.MAT_GRAD) for k in range(s.nblk)] + \
                [be.get_vec(host.VEC_LAMBDA), be.get_vec(host.VEC_CONSTR_SUM)]
            runs.append((outs, st))
        finally:
            s.close()
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for x, y in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(x, y)
