"""Inputs of the dual-side tests (tests/test_dual_model.py on the CPU, tests/test_dual_edges.py on the device): slack matrices
prescribed entry for entry through instances.prescribed_slack, at the sizes where the kernels of csrc/hip/lanczos.inc change path
and with spectra known in closed form."""
import numpy as np

NCVS = [2, 3, 8, 9, 40, 126, 127]   # keep = min(8, m - 1) below and at its cap; the default; the pinned / unpinned read-back switch
TOLS = [1e-2, 1e-10]
# m = n and a breakdown at j = n - 1 | keep at its cap | k_spmv's 32 rows per workgroup | m = n against m = ncv = 40 |
# the 256 threads of k_basis_sub and k_scale_to_dev | the 2048 elements per trip of k_basis_dots
EDGE_SIZES = [1, 2, 3, 8, 9, 10, 31, 32, 33, 39, 40, 41, 255, 256, 257, 2047, 2048, 2049]


def edge_offdiagonals(n):
    """off-diagonal entries of edge_matrix(n): about three per row, but fewer than 0.08 n (n + 1) / 2 from n = 31 on -- the solver
    stores an objective with more than 0.1 n (n + 1) / 2 entries dense, and from there on k_spmv is to carry the whole product;
    the tiny sizes keep at least one coupling (and so a dense objective wherever the rule says)"""
    if n < 2:
        return 0
    cap = int(0.08 * n * (n + 1) / 2)
    return min(3 * n, n * (n - 1) // 2, cap if n >= 31 else max(1, cap))


def edge_matrix(n, seed=None):
    """seeded sparse symmetric matrix: a N(0, 1) diagonal and edge_offdiagonals(n) N(0, 1) entries above it (drawn with repetition:
    a few less)"""
    rng = np.random.default_rng(4200 + n if seed is None else seed)
    S = np.diag(rng.standard_normal(n))
    k = edge_offdiagonals(n)
    if k:
        i, j = rng.integers(0, n, size=k), rng.integers(0, n, size=k)
        v = rng.standard_normal(k)
        for a, b, x in zip(i.tolist(), j.tolist(), v.tolist()):
            if a != b:
                S[a, b] = S[b, a] = x
        if n <= 10 and not np.count_nonzero(np.triu(S, 1)):
            S[0, n - 1] = S[n - 1, 0] = float(v[0])
    return S


def block_repeat(blk, n):
    b = blk.shape[0]
    assert n % b == 0
    return np.kron(np.eye(n // b), blk)


def path_block(p):
    """adjacency matrix of the path on p points: eigenvalues 2 cos(k pi / (p + 1)), k = 1..p, all simple"""
    return np.diag(np.ones(p - 1), 1) + np.diag(np.ones(p - 1), -1)


def clustered_matrix(n=120, seed=77):
    """a triple smallest eigenvalue -1, then 29 eigenvalues 1e-3 apart from -1 + 1e-3 on, the rest spread over [0, 1], in a seeded
    orthogonal basis.  Forming Q diag(ev) Q^T rounds: a test takes the spectrum from numpy.linalg.eigvalsh of the matrix as
    stored, not from this recipe."""
    rng = np.random.default_rng(seed)
    ev = np.concatenate([[-1.0] * 3, -1.0 + 1e-3 * np.arange(1, 30), np.linspace(0.0, 1.0, n - 32)])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    S = (Q * ev) @ Q.T
    return (S + S.T) / 2


def gram_matrix(n=90, r=6, seed=78):
    G = np.random.default_rng(seed).standard_normal((n, r))
    S = G @ G.T
    return (S + S.T) / 2


# name: (matrix, number of steps after which the start vector's Krylov space is invariant, or None)
def closed_form():
    return {
        "two_by_two_64": (block_repeat(np.array([[1.0, 2.0], [2.0, 1.0]]), 64), 2),      # eigenvalues -1 and 3
        "path5_100": (block_repeat(path_block(5), 100), 5),
        "plus3I_50": (3.0 * np.eye(50), 1),
        "minus3I_50": (-3.0 * np.eye(50), 1),
        "zero_50": (np.zeros((50, 50)), 1),
        "gram90x6": (gram_matrix(), None),   # (seven distinct eigenvalues, but beta_6 is rounding of size eps ||S||: no sharp step)
        "clustered120": (clustered_matrix(), None),
        "path12_120": (block_repeat(path_block(12), 120), 12),
    }
