"""NumPy restatement of the device thick-restart Lanczos bidiagonalisation (pykrylov_amd.ThickRestartSVD,
csrc/mk_trsvd.hip), operation by operation.  TEST INFRASTRUCTURE ONLY.

Thick-restart Golub-Kahan-Lanczos bidiagonalisation (Baglama and Reichel 2005) for the `nsv` largest ('LM') or smallest
('SM') singular triplets of a tall operator (nrows >= ncols): the short basis V is orthogonalised in full (classical
Gram-Schmidt, twice) at every step, the long basis U in full (`reorth='full'`) or against u_{j-1} alone
(`reorth='one-sided'`, Simon and Zha 2000).  `A` is anything with ``matvec`` and ``rmatvec`` (oracle.csr_ref.RefCsr).
``dots(a, b, site)`` is the inner product: ``np.dot`` by default; on the device the site ``SITE_UU`` -- <u, u> of a
one-sided step that is not the first behind a restart -- is summed in the row order of A's product kernel, every other
site in the order of the stream kernels (oracle.gpu_order.GpuDots).  Every other operation rounds alike on both sides.
`jacobi_svd` restates the library's host solver of the small problem; it is the only one the loop uses.
"""
from collections import namedtuple
from math import fabs, sqrt

import numpy as np

from oracle import csr_ref
from tests._trlan_ref import KT, MAX_NCV, default_keep, rotate      # noqa: F401  (the rotation kernel is TRLAN's)

MAX_SWEEPS = 40                  # SV_SWEEPS of csrc/mk_trsvd.hip
SKIP = 2.0 ** -6                 # a pair with d + SKIP |c| == d, d = sqrt(a) sqrt(b), is orthogonal enough (SV_SKIP)
SITE_UU = "trsvd.uu"

TrsvdResult = namedtuple("TrsvdResult", "s U V residNorms pairIters nconv converged breakdown nMatvec nIter cycles history "
                                        "anorm threshold residNorm residNorm0 ncv keep reorth sweeps")


def default_ncv(c, nsv):
    return min(c, MAX_NCV, max(2 * nsv + 1, 20))


def np_dots(a, b, site=None):
    return float(np.dot(a, b))


def jacobi_svd(B):
    """One-sided (Hestenes) Jacobi on a copy G of the square matrix B: row-cyclic pairs (p, q), p < q, of COLUMNS; with
    a = <g_p, g_p>, b = <g_q, g_q>, c = <g_p, g_q> (row index ascending, one multiply and one add per term) the pair is
    skipped when c == 0, when sqrt(a) + sqrt(b) equals one of the two (a column that is negligible against the other: what
    is left of a zero singular value) or when d + SKIP |c| == d for d = sqrt(a) sqrt(b); otherwise zeta = (b - a) / (2 c),
    t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), cs = 1 / sqrt(1 + t^2), sn = cs t, and columns p, q of G and of Y
    become cs g_p - sn g_q and sn g_p + cs g_q.  Ends after a sweep without rotations.  The singular values are the
    column norms, X the normalised columns; a column whose norm s has s_max + s == s_max is a zero singular value to
    working precision: s = 0 and its column of X is zero (for a zero matrix all of them).  Returns (s descending -- ties by
    index --, X, Y, sweeps) with B = X diag(s) Y'."""
    g = np.array(B, dtype=np.float64)
    m = g.shape[0]
    y = np.eye(m)
    for sweep in range(1, MAX_SWEEPS + 1):
        rotations = 0
        for p in range(m - 1):
            for q in range(p + 1, m):
                gp, gq = g[:, p].copy(), g[:, q].copy()
                # (np.cumsum adds strictly in sequence: the C loop's `a = a + gp[k] * gp[k]`, k ascending)
                a, b, c = (float(v) for v in np.cumsum(np.stack([gp * gp, gq * gq, gp * gq]), axis=1)[:, -1])
                if c == 0.0:
                    continue
                sa, sb = sqrt(a), sqrt(b)
                if sa + sb == sa or sa + sb == sb:               # one column is negligible against the other
                    continue
                d = sa * sb
                if d + SKIP * fabs(c) == d:
                    continue
                zeta = (b - a) / (2.0 * c)
                t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta))
                if zeta < 0.0:
                    t = -t
                cs = 1.0 / sqrt(1.0 + t * t)
                sn = cs * t
                g[:, p] = cs * gp - sn * gq
                g[:, q] = sn * gp + cs * gq
                yp, yq = y[:, p].copy(), y[:, q].copy()
                y[:, p] = cs * yp - sn * yq
                y[:, q] = sn * yp + cs * yq
                rotations += 1
        if rotations == 0:
            s = np.zeros(m)
            x = np.zeros((m, m))
            for i in range(m):
                s[i] = sqrt(float(np.cumsum(g[:, i] * g[:, i])[-1]))
            top = float(np.max(s))
            for i in range(m):
                if top + s[i] == top:                            # zero to working precision: s = 0 and no left vector
                    s[i] = 0.0
                else:
                    x[:, i] = g[:, i] / s[i]
            order = np.argsort(-s, kind="stable")
            return s[order].copy(), x[:, order].copy(), y[:, order].copy(), sweep
    raise RuntimeError("jacobi_svd: no convergence in %d sweeps" % MAX_SWEEPS)


def _orth_twice(w, W, ncol, dots):
    "D, U, D, U of mk_multicol.h against the rows 0 .. ncol - 1 of W, columns ascending."
    for _ in range(2):
        h = [dots(W[i], w, None) for i in range(ncol)]
        for i in range(ncol):
            w = w - h[i] * W[i]
    return w


def trsvd(A, nsv, which="LM", ncv=None, keep=None, abstol=0.0, reltol=1.0e-10, matvec_max=None, start=None, seed=1,
          reorth="full", dots=np_dots):
    """The loop on a tall operator (the class swaps a wide one first).  The rows of the returned U and V are the vectors."""
    R, C = A.shape
    if R < C:
        raise ValueError("the loop takes a tall operator; hand it the transpose and swap U and V")
    if ncv is None:
        ncv = default_ncv(C, nsv)
    if keep is None:
        keep = default_keep(nsv, ncv)
    if matvec_max is None:
        matvec_max = max(4 * C, 2 * ncv)
    if which not in ("LM", "SM") or reorth not in ("full", "one-sided"):
        raise ValueError("which must be 'LM' or 'SM', reorth 'full' or 'one-sided'")
    if not (1 <= nsv < ncv <= min(C, MAX_NCV)) or not (nsv <= keep < ncv):
        raise ValueError("needs 1 <= nsv < ncv <= min(ncols, %d) and nsv <= keep < ncv" % MAX_NCV)
    full = reorth == "full"
    m = ncv
    if start is None:
        start = csr_ref.cell_field(np.arange(C), seed) - 1.0
    start = np.ascontiguousarray(start, dtype=np.float64)
    b0 = sqrt(dots(start, start, None))
    V = np.zeros((m + 1, C))
    U = np.zeros((m, R))
    B = np.zeros((m, m))
    l = 0
    anorm = smax = beta = 0.0
    nMatvec = nIter = cycles = sweeps = 0
    history = []
    first_met = np.full(nsv, -1, dtype=np.int64)
    converged, breakdown, m_eff = False, 0, 0
    s = np.zeros(0)
    est = np.zeros(0)
    X = Y = np.zeros((0, 0))
    ok = np.isfinite(b0) and b0 > 0.0
    if not ok:
        breakdown = 3                                            # a start vector without a positive, finite norm
    else:
        V[0] = (1.0 / b0) * start
    while ok and nMatvec + 2 * (m - l) <= matvec_max:
        m_eff, breakdown = m, 0
        for j in range(l, m):
            u = A.matvec(V[j])
            nMatvec += 1
            if full:
                if j > 0:
                    u = _orth_twice(u, U, j, dots)
                uu = dots(u, u, None)
            elif j == l and l > 0:                               # the arrow: the first step behind a restart
                for i in range(l):
                    u = u - B[i, l] * U[i]
                uu = dots(u, u, None)
            else:
                if j > 0:
                    u = u - B[j - 1, j] * U[j - 1]
                uu = dots(u, u, SITE_UU)
            alpha = sqrt(uu)
            nIter += 1
            if not alpha > 2.0 ** -26 * smax:                    # A v_j lies in the span of U_{j-1}
                B[j, j] = 0.0
                U[j] = 0.0
                m_eff, breakdown = j + 1, 2
                break
            smax = alpha if alpha > smax else smax
            B[j, j] = alpha
            U[j] = (1.0 / alpha) * u
            w = A.rmatvec(U[j])
            nMatvec += 1
            w = _orth_twice(w, V, j + 1, dots)
            beta = sqrt(dots(w, w, None))
            if not beta > 2.0 ** -26 * smax:
                m_eff, breakdown = j + 1, 1
                break
            smax = beta if beta > smax else smax
            if j + 1 < m:
                B[j, j + 1] = beta
            V[j + 1] = (1.0 / beta) * w
        cycles += 1
        s, X, Y, sweeps = jacobi_svd(B[:m_eff, :m_eff])
        order = np.arange(m_eff) if which == "LM" else np.arange(m_eff)[::-1]
        est = np.zeros(m_eff) if breakdown else np.abs(beta * X[m_eff - 1])
        anorm = max(anorm, float(s[0]))
        threshold = max(abstol, reltol * anorm)
        nret = min(nsv, m_eff)
        wanted = order[:nret]
        resid = float(np.max(est[wanted]))
        history.append(resid)
        met = est[wanted] <= threshold
        first_met[:nret][met & (first_met[:nret] < 0)] = cycles
        converged = bool(nret == nsv and met.all())
        if converged or breakdown or nMatvec + 2 * (m - keep) > matvec_max:
            break
        kept = order[:keep]
        U[:keep] = rotate(U[:m], X[:, kept])
        V[:keep] = rotate(V[:m], Y[:, kept])
        V[keep] = V[m]
        B = np.zeros((m, m))
        for i in range(keep):
            B[i, i] = s[kept[i]]
            B[i, keep] = beta * X[m - 1, kept[i]]
        l = keep
    if cycles == 0:                                              # halted before the first step
        return TrsvdResult(np.zeros(0), np.zeros((0, R)), np.zeros((0, C)), np.zeros(0), np.zeros(0, dtype=np.int64), 0,
                           False, breakdown, 0, 0, 0, np.zeros(0), 0.0, 0.0, 0.0, b0, m, keep, reorth, 0)
    dsc = np.sort(wanted)                                        # the wanted triplets in descending order of s
    pos = {int(k): i for i, k in enumerate(wanted)}
    return TrsvdResult(s[dsc].copy(), rotate(U[:m_eff], X[:, dsc]), rotate(V[:m_eff], Y[:, dsc]), est[dsc].copy(),
                       np.array([first_met[pos[int(k)]] for k in dsc]), int(np.sum(est[wanted] <= threshold)), converged,
                       breakdown, nMatvec, nIter, cycles, np.array(history), anorm, threshold, resid, b0, m, keep, reorth,
                       sweeps)
