"""Spectrum / rank reduction without a GPU: the host's rank rule against numpy, the numpy model of the
device's Jacobi eigen-solve (tests/spectral_model.py) against numpy.linalg, the refusals that need no backend."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host
from tests import common, spectral_model
from tests.spectral_model import U

_dp = C.POINTER(C.c_double)


def _choose(lib, eig, tol, cap):
    eig = np.ascontiguousarray(eig, dtype=np.float64)
    lib.lrd_spectral_choose.argtypes = [_dp, C.c_int, C.c_double, C.c_int]
    return lib.lrd_spectral_choose(eig.ctypes.data_as(_dp), len(eig), float(tol), int(cap))


def test_rank_rule_against_numpy(built):
    lib = host.host_lib()
    rng = np.random.default_rng(7)
    for trial in range(300):
        rl = int(rng.integers(1, 60))
        eig = np.sort(10.0 ** rng.uniform(-18, 2, rl))[::-1].copy()
        if trial % 5 == 0:
            eig[rl // 2:] = 0.0
        if trial % 7 == 0:
            eig[-1] = -abs(eig[-1]) * 1e-3
        tol = float(10.0 ** rng.uniform(-14, -1))
        cap = int(rng.integers(-1, rl + 3))
        want = max(1, min(cap if cap > 0 else rl, int(np.sum(eig > tol * eig[0]))))
        assert _choose(lib, eig, tol, cap) == want == spectral_model.choose_rank(eig, tol, cap), (trial, eig, tol, cap)
    # ties at the threshold: an eigenvalue equal to tol * lambda_1 does not count
    eig = np.array([4.0, 2.0, 1.0, 1.0, 0.5])
    assert _choose(lib, eig, 0.25, 0) == 2
    assert _choose(lib, eig, 0.125, 0) == 4
    assert _choose(lib, eig, 0.0, 0) == 5
    assert _choose(lib, eig, 0.0, 3) == 3
    assert _choose(lib, eig, 2.0, 0) == 1      # nothing above the threshold: one column stays
    # lambda_1 = 0 (a zero factor) and below
    assert _choose(lib, np.zeros(6), 1e-12, 0) == 1
    assert _choose(lib, np.zeros(6), 0.0, 4) == 1
    assert _choose(lib, np.array([0.0, -1e-20]), 1e-12, 0) == 1
    assert _choose(lib, np.array([3.0]), 1e-12, 0) == 1


def _gram(order, deficient, seed):
    rng = np.random.default_rng(seed)
    k = order if not deficient else max(1, order - (2 * order) // 3)   # two thirds of the spectrum at zero
    F = rng.standard_normal((5 * order + 7, k)) @ rng.standard_normal((k, order)) if deficient else rng.standard_normal((5 * order + 7, order))
    return F.T @ F


@pytest.mark.parametrize("deficient", [False, True], ids=["full", "deficient"])
@pytest.mark.parametrize("order", [1, 2, 9, 10, 41, 128, 258])
def test_jacobi_model_against_numpy(order, deficient):
    G = _gram(order, deficient, 100 * order + deficient)
    lam, Q, sweeps = spectral_model.jacobi_eigh(G)
    m = order + (order & 1)
    want = np.linalg.eigvalsh(G)[::-1]
    l1 = max(abs(want[0]), abs(want[-1]))
    assert 1 <= sweeps <= spectral_model.MAX_SWEEPS
    assert np.all(np.diff(lam) <= 0)
    bound = 8 * sweeps * m * U
    err = np.abs(lam - want).max() / l1
    orth = np.abs(Q.T @ Q - np.eye(order)).max()
    res = np.abs(G @ Q - Q * lam).max() / l1
    print("order %d %s: sweeps %d, eig err %.2e, orth %.2e, residual %.2e of bound %.2e" % (order, "deficient" if deficient else "full",
                                                                                          sweeps, err, orth, res, bound))
    assert err <= bound
    assert orth <= bound
    assert res <= bound * max(1.0, np.sqrt(m))  # (a residual entry is a sum of m such terms)


def test_round_robin_covers_every_pair_once():
    for m in (2, 4, 10, 42):
        seen = set()
        for step in range(m - 1):
            pairs = spectral_model.round_robin(m, step)
            assert len({i for pq in pairs for i in pq}) == m   # disjoint
            seen.update(pairs)
        assert len(seen) == m * (m - 1) // 2


def test_oracle_session_cannot_compute_the_spectrum(oracle_lib):
    s = common.oracle_session(common.instance_path("theta30"))
    try:
        with pytest.raises(NotImplementedError):
            s.spectrum()
        with pytest.raises(NotImplementedError):
            s.compress_rank()
    finally:
        s.close()


@pytest.mark.parametrize("opt,val", [("--compressTol", "x"), ("--compressTol", "-1e-3"), ("--compressTol", "nan"), ("--compressRank", "0"),
                                     ("--compressRank", "2.5")])
def test_cli_refuses_bad_values_before_the_backend(built, opt, val):
    exe = os.path.join(host.LIB_DIR, "lorads")
    r = subprocess.run([exe, common.instance_path("theta30"), opt, val], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "bad value %s of %s" % (val, opt) in r.stderr
    assert "HIP backend" not in r.stderr


def test_table_mirror_has_the_pair(built):
    names = [f[0] for f in host.BackendStruct._fields_]
    assert names[-2:] == ["spectrum", "compress_rank"]
    lib = host.host_lib()
    lib.lrd_backend_sizeof.restype = C.c_size_t
    assert lib.lrd_backend_sizeof() == C.sizeof(host.BackendStruct)
    hip = C.CDLL(os.path.join(host.LIB_DIR, "liblorads_hip.so"))
    assert hasattr(hip, "lorads_hip_spectrum") and hasattr(hip, "lorads_hip_compress_rank")
