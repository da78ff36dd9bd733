"""The host routine that diagonalises the projected matrix of the slack eigen-solve (small_sym_eig, csrc/hip/lanczos.inc), alone,
on the CPU: its text is compiled into a small program of its own and held to numpy.linalg.eigvalsh on the matrices the Lanczos
process hands it -- tridiagonal, diagonal with an arrow and a tridiagonal tail (after a thick restart), repeated eigenvalues, zero --
at the orders the subspace sizes give (1, 2, 3, 8, 9, 40, 41, 127).

Bound: 32 eps ||T||_2 on every eigenvalue, on ||T y - theta y||_inf and on the orthonormality of Y -- LAPACK itself is within 15 eps
on these matrices; a rotation written out as two matrix products loses about m eps (40 to 1000 eps at m = 40 to 127)."""
import os
import subprocess

import numpy as np
import pytest

from tests import common

SRC = os.path.join(common.ROOT, "lorads_amd", "csrc", "hip", "lanczos.inc")
EPS = 2.220446049250313e-16

MAIN = r'''
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int m;
    while (fread(&m, sizeof(int), 1, f) == 1) {
        std::vector<double> A((size_t)m * m), th, Y;
        if (fread(A.data(), sizeof(double), A.size(), f) != A.size()) return 1;
        small_sym_eig(m, A, th, Y);
        fwrite(th.data(), sizeof(double), th.size(), stdout);
        fwrite(Y.data(), sizeof(double), Y.size(), stdout);
    }
    return 0;
}
'''


def _matrices():
    rng = np.random.default_rng(3)
    out = []
    for m in (1, 2, 3, 8, 9, 40, 41, 127):
        T = np.diag(rng.standard_normal(m))
        if m > 1:
            o = rng.standard_normal(m - 1)
            T += np.diag(o, 1) + np.diag(o, -1)
        out.append(("tridiagonal", T))
        T = np.diag(np.sort(rng.standard_normal(m)))
        if m > 1:
            k = min(8, m - 1)
            T[:k, k] = T[k, :k] = 1e-3 * rng.standard_normal(k)
            for j in range(k, m - 1):
                T[j, j + 1] = T[j + 1, j] = rng.standard_normal()
        out.append(("arrow", T))
        Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        T = (Q * np.repeat([-1.0, 2.0], [m // 2, m - m // 2])) @ Q.T
        out.append(("repeated", (T + T.T) / 2))
        out.append(("zero", np.zeros((m, m))))
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("small_sym_eig")
    text = open(SRC).read()
    fn = text[text.index("void small_sym_eig("):text.index("struct LanczosBufs")]
    (d / "eig.cpp").write_text("#include <algorithm>\n#include <cmath>\n#include <cstdio>\n#include <vector>\n" + fn + MAIN)
    subprocess.check_call(["g++", "-O2", "-std=c++17", str(d / "eig.cpp"), "-o", str(d / "eig")])
    mats = _matrices()
    with open(d / "in.bin", "wb") as f:
        for _, T in mats:
            f.write(np.int32(T.shape[0]).tobytes())
            f.write(np.ascontiguousarray(T, dtype=np.float64).tobytes())
    raw = np.frombuffer(subprocess.check_output([str(d / "eig"), str(d / "in.bin")]), dtype=np.float64)
    out, pos = [], 0
    for kind, T in mats:
        m = T.shape[0]
        out.append((kind, T, raw[pos:pos + m], raw[pos + m:pos + m + m * m].reshape(m, m)))   # row c of Y: eigenvector c
        pos += m + m * m
    assert pos == len(raw)
    return out


def test_against_eigvalsh(results):
    worst = 0.0
    for kind, T, th, Y in results:
        m = T.shape[0]
        ev = np.linalg.eigvalsh(T)
        nrm = max(abs(ev[0]), abs(ev[-1]))
        assert np.all(np.diff(th) >= 0), (kind, m, "not ascending")
        err = np.abs(th - ev).max()
        res = np.abs(Y @ T - th[:, None] * Y).max()
        orth = np.abs(Y @ Y.T - np.eye(m)).max()
        worst = max(worst, err / (EPS * nrm) if nrm else 0.0)
        assert err <= 32 * EPS * nrm and res <= 32 * EPS * nrm and orth <= 32 * EPS, (kind, m, err, res, orth, nrm)
    print("worst eigenvalue error: %.1f eps ||T||" % worst)
