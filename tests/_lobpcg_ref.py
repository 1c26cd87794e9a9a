"""NumPy restatement of the device LOBPCG eigensolver (pykrylov_amd.LOBPCG, csrc/mk_lobpcg.hip), operation by operation.
TEST INFRASTRUCTURE ONLY.

LOBPCG (Knyazev 2001) for the `nev` smallest ('SA') or largest ('LA') eigenvalues of a symmetric operator with a block of
`block` vectors, an optional preconditioner (``precon(r)``, an approximation of the inverse of `A`) and soft locking.  `A` is
anything with ``matvec`` (oracle.csr_ref.RefCsr).  ``dots(a, b)`` is the inner product: ``np.dot`` by default,
``oracle.gpu_order.stream_dot`` for the device's summation order -- every other operation rounds alike on both sides.  The
vectors are the ROWS of every array here.  The small problem (scaling, Cholesky factor, the two triangular solves, Jacobi)
is restated in the order of the library's host code; `_trlan_ref.jacobi_eigh` is the eigensolver of both.
"""
from collections import namedtuple
from math import sqrt

import numpy as np

from oracle import csr_ref
from tests._trlan_ref import jacobi_eigh, rotate

MAX_BLOCK = 16
PIVOT = 2.0 ** -26

LobpcgResult = namedtuple("LobpcgResult", "w X residNorms pairIters nconv converged breakdown restarts nMatvec nIter history "
                                          "anorm threshold residNorm block actives lockIters sweeps")


def default_block(n, nev):
    return min(MAX_BLOCK, n // 3, max(nev + 2, (3 * nev + 1) // 2))


def inv_norm(v, dots):
    """1 / ||v|| as the device forms it: a zero vector gives inf, the vector becomes NaN, and the next small problem fails its
    test on that diagonal entry (the fallback without P, or a breakdown)."""
    with np.errstate(all="ignore"):
        return np.float64(1.0) / np.sqrt(np.float64(dots(v, v)))


def gram(U, V, dots):
    """The entries on and above the diagonal of U V', each one inner product; the host mirrors them."""
    m = U.shape[0]
    G = np.zeros((m, m))
    for i in range(m):
        for j in range(i, m):
            G[i, j] = G[j, i] = dots(U[i], V[j])
    return G


def rayleigh_ritz(G, H):
    """The small generalised problem H c = theta G c: d = diag(G)^-1/2, Cholesky factor L of d G d with the pivot test
    v > 2^-26, T = L^-1 (d H d) L^-T symmetrised, Jacobi, C = d L^-T Z.  Returns (theta ascending, C, sweeps), or None when a
    pivot fails the test (NaN included)."""
    m = G.shape[0]
    dg = np.diag(G)
    if not np.all(dg > 0.0):
        return None
    d = 1.0 / np.sqrt(dg)
    Gs = (d[:, None] * G) * d[None, :]
    Hs = (d[:, None] * H) * d[None, :]
    L = np.zeros((m, m))
    for j in range(m):
        s = Gs[j:, j].copy()
        for k in range(j):
            s = s - L[j:, k] * L[j, k]
        if not s[0] > PIVOT:
            return None
        L[j, j] = sqrt(s[0])
        L[j + 1:, j] = s[1:] / L[j, j]

    def forward(B):                                              # L^-1 B, row by row
        Y = np.zeros((m, m))
        for i in range(m):
            r = B[i].copy()
            for k in range(i):
                r = r - L[i, k] * Y[k]
            Y[i] = r / L[i, i]
        return Y
    Tt = forward(forward(Hs).T.copy())                           # (L^-1 Hs L^-T)'
    T = 0.5 * (Tt + Tt.T)
    theta, Z, sweeps = jacobi_eigh(T)
    Q = np.zeros((m, m))
    for i in range(m - 1, -1, -1):                               # L' Q = Z
        r = Z[i].copy()
        for k in range(i + 1, m):
            r = r - L[k, i] * Q[k]
        Q[i] = r / L[i, i]
    return theta, d[:, None] * Q, sweeps


def lobpcg(A, nev, which="SA", block=None, abstol=0.0, reltol=1.0e-10, matvec_max=None, start=None, seed=1, precon=None,
           dots=np.dot):
    n = A.shape[0]
    nb = default_block(n, nev) if block is None else block
    if matvec_max is None:
        matvec_max = max(2 * n, nb)
    if which not in ("SA", "LA"):
        raise ValueError("which must be 'SA' or 'LA'")
    if not (1 <= nev <= nb <= MAX_BLOCK and nb <= n // 3):
        raise ValueError("needs 1 <= nev <= block <= min(%d, n // 3)" % MAX_BLOCK)
    if matvec_max < nb:
        raise ValueError("matvec_max below block")
    if which == "LA" and precon is not None:
        raise ValueError("a preconditioner approximates the inverse: it steers towards the smallest eigenvalues")
    sgn = 1.0 if which == "SA" else -1.0
    if start is None:
        X = np.stack([csr_ref.cell_field(np.arange(n), seed + j) - 1.0 for j in range(nb)])
    else:
        X = np.array(start, dtype=np.float64).reshape(nb, n)
    AX = np.stack([A.matvec(X[j]) for j in range(nb)])
    nMatvec = nb
    sweeps = restarts = nIter = 0
    breakdown = False
    G = gram(X, X, dots)
    rr = rayleigh_ritz(G, sgn * gram(X, AX, dots))
    if rr is None:                                               # the start block is (numerically) rank deficient
        breakdown = True
        dg = np.diag(G)
        theta = np.where(dg > 0.0, np.diag(sgn * gram(X, AX, dots)) / np.where(dg > 0.0, dg, 1.0), 0.0)
        anorm = float(np.max(np.abs(theta)))
    else:
        theta_all, C, sweeps = rr
        X, AX = rotate(X, C), rotate(AX, C)
        theta = theta_all.copy()
        anorm = float(np.max(np.abs(theta_all)))
    P = AP = None
    active = np.ones(nb, dtype=bool)
    pcols = np.zeros(0, dtype=np.int64)                          # the columns of X that the rows of P belong to
    history, actives = [], []
    first_met = np.full(nev, -1, dtype=np.int64)
    lock_iters = np.full(nb, -1, dtype=np.int64)                 # the iteration count at which a column left the active set
    while True:
        st = sgn * theta
        R = AX - st[:, None] * X
        rn = np.array([sqrt(dots(R[j], R[j])) for j in range(nb)])
        threshold = max(abstol, reltol * anorm)
        history.append(float(np.max(rn[:nev])))
        met = rn[:nev] <= threshold
        first_met[met & (first_met < 0)] = nIter
        converged = bool(met.all())
        if converged or breakdown:
            break
        lock_iters[active & ~(rn > threshold)] = nIter
        active = active & (rn > threshold)
        if not active.any():                                     # every column was locked, and a wanted one came back
            active = rn > threshold
            P = AP = None
            restarts += 1
        act = np.flatnonzero(active)
        na = len(act)
        if nMatvec + na > matvec_max:
            break
        if P is not None:                                        # a column that left the active set drops its P column
            keep = np.isin(pcols, act)
            P, AP = P[keep], AP[keep]
        W = np.stack([np.array(precon(R[j]), dtype=np.float64) if precon is not None else R[j].copy() for j in act])
        for k in range(na):
            w = W[k]
            for _ in range(2):
                h = [dots(X[i], w) for i in range(nb)]
                for i in range(nb):
                    w = w - h[i] * X[i]
            with np.errstate(all="ignore"):
                W[k] = inv_norm(w, dots) * w
        AW = np.stack([A.matvec(W[k]) for k in range(na)])
        nMatvec += na
        actives.append(na)
        S = np.concatenate([X, W] + ([P] if P is not None else []))
        AS = np.concatenate([AX, AW] + ([AP] if P is not None else []))
        G, H = gram(S, S, dots), sgn * gram(S, AS, dots)
        rr = rayleigh_ritz(G, H)
        if rr is None and P is not None:                         # drop P and solve the leading problem again
            restarts += 1
            m = nb + na
            S, AS = S[:m], AS[:m]
            rr = rayleigh_ritz(G[:m, :m], H[:m, :m])
        if rr is None:
            breakdown = True                                     # (X, theta and rn are the last iterate's)
            break
        theta_all, C, sweeps = rr
        anorm = max(anorm, float(np.max(np.abs(theta_all))))
        Cx = C[:, :nb]
        # a column of X that takes nothing from W and P (a locked vector that moved into an active place when the Ritz values
        # changed their order) has a P of exact zeros: it gets none
        pk = act[np.any(C[nb:, act] != 0.0, axis=0)]
        X, AX = rotate(S, Cx), rotate(AS, Cx)
        if len(pk):
            P, AP = rotate(S[nb:], C[nb:, pk]), rotate(AS[nb:], C[nb:, pk])
            for k in range(len(pk)):
                s = inv_norm(P[k], dots)
                with np.errstate(all="ignore"):
                    P[k], AP[k] = s * P[k], s * AP[k]
        else:
            P = AP = None
        pcols = pk
        theta = theta_all[:nb].copy()
        nIter += 1
    order = np.arange(nev) if which == "SA" else np.arange(nev)[::-1]
    return LobpcgResult((sgn * theta[:nev])[order], X[:nev][order].copy(), rn[:nev][order].copy(), first_met[order].copy(),
                        int(np.sum(met)), converged, breakdown, restarts, nMatvec, nIter, np.array(history), anorm, threshold,
                        history[-1], nb, actives, lock_iters, sweeps)
