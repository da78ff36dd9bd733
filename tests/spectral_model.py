"""numpy restatement of the device's eigen-solve of a Gram matrix (lorads_amd/csrc/hip/spectral.inc:
k_spec_jacobi), written from the definition: cyclic Jacobi in the round-robin ("circle") ordering, m - 1 steps of m / 2 disjoint
plane rotations per sweep (m = the order rounded up to even), all rotations of a step computed from the matrix as the step found
it, a rotation skipped when |g_pq| <= 2^-53 ||G||_F (absolute), the run ended by the first sweep that rotates nothing, then the
eigenvalues sorted descending (ties: lower original index first) with their columns.  Also the rank rule of the host."""
import numpy as np

U = 2.0 ** -53
MAX_SWEEPS = 30


def round_robin(m, step):
    """the m / 2 disjoint pairs (p < q) of step `step` (0 .. m - 2) of the circle ordering on m (even) indices"""
    pairs = []
    for i in range(m // 2):
        if i == 0:
            a, b = m - 1, step
        else:
            a, b = (step + i) % (m - 1), (step - i) % (m - 1)
        pairs.append((min(a, b), max(a, b)))
    return pairs


def jacobi_eigh(G0):
    """(eigenvalues descending, eigenvectors as columns, sweeps) of the symmetric G0; raises when 30 sweeps all rotate"""
    G0 = np.asarray(G0, dtype=np.float64)
    rl = G0.shape[0]
    m = rl + (rl & 1)
    G = np.zeros((m, m))
    G[:rl, :rl] = G0
    Q = np.eye(m)
    thr = U * np.sqrt(np.sum(G * G))
    sweeps, rotated = 0, True
    while rotated:
        if sweeps == MAX_SWEEPS:
            raise RuntimeError("the Jacobi iteration still rotates after %d sweeps" % MAX_SWEEPS)
        rotated = False
        for step in range(m - 1):
            pq = np.array(round_robin(m, step))
            p, q = pq[:, 0], pq[:, 1]
            gpq = G[p, q]
            on = np.abs(gpq) > thr
            if not on.any():
                continue
            rotated = True
            p, q, gpq = p[on], q[on], gpq[on]
            tau = (G[q, q] - G[p, p]) / (2.0 * gpq)
            t = np.copysign(1.0, tau) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = t * c
            for M in (G, Q):  # columns p, q
                mp, mq = M[:, p].copy(), M[:, q].copy()
                M[:, p] = c * mp - s * mq
                M[:, q] = s * mp + c * mq
            gp, gq = G[p, :].copy(), G[q, :].copy()  # rows p, q
            G[p, :] = c[:, None] * gp - s[:, None] * gq
            G[q, :] = s[:, None] * gp + c[:, None] * gq
        sweeps += 1
    d = np.diag(G)[:rl]
    order = np.argsort(-d, kind="stable")
    return d[order], Q[:rl, :rl][:, order], sweeps


def choose_rank(eig, tol, cap):
    """max(1, min(cap, #{j : eig_j > tol eig_1})) for eig descending; cap <= 0: no cap"""
    eig = np.asarray(eig, dtype=np.float64)
    k = int(np.sum(eig > tol * eig[0])) if len(eig) else 0
    if cap > 0:
        k = min(k, cap)
    return max(1, k)
