"""NumPy restatement of the device Chebyshev filter (pykrylov_amd.tools.cheb_filter, csrc/mk_chebfilt.hip) and of the filtered
cycle of the thick-restart Lanczos eigensolver (the block mk_params_filter, csrc/mk_trlan.hip), operation by operation.  TEST
INFRASTRUCTURE ONLY.

`A` is an oracle matrix (oracle.csr_ref.RefCsr): its ``matvec`` adds every row left to right in stored order, like every
product kernel of the library.  ``dots(a, b)`` is the inner product: ``np.dot`` by default, ``oracle.gpu_order.stream_dot``
(through ``gpu_order.GpuDots``) for the device's summation order -- every other operation rounds alike on both sides.  The
small eigenproblem and the rotation are those of tests/_trlan_ref.py.
"""
from collections import namedtuple
from math import acosh, fabs, sqrt

import numpy as np

from oracle import csr_ref
from tests import _lanczos_ref
from tests._trlan_ref import MAX_NCV, default_keep, default_ncv, jacobi_eigh, rotate

MAX_DEGREE = 128

FilteredResult = namedtuple("FilteredResult", "w X residNorms pairIters nconv converged breakdown nMatvec nIter cycles history "
                                              "anorm threshold residNorm residNorm0 ncv keep sweeps verified")


def coefficients(a, b, a0, degree):
    """``(c, e, p, q)`` of mk_filter_create: one rounding per operation, in the library's order."""
    a, b, a0 = float(a), float(b), float(a0)
    e = 0.5 * (b - a)
    c = 0.5 * (b + a)
    sigma = e / (a0 - c)
    tau = 2.0 / sigma
    p, q = np.zeros(degree), np.zeros(degree)
    p[0] = sigma / e
    for j in range(2, degree + 1):
        sigma_j = 1.0 / (tau - sigma)
        p[j - 1] = (2.0 * sigma_j) / e
        q[j - 1] = sigma * sigma_j
        sigma = sigma_j
    return c, e, p, q


def gershgorin(A):
    """``(min_r (a_rr - off_r), max_r (a_rr + off_r))``, off_r the sum of the moduli of the entries off the diagonal: each row
    added left to right in stored order from +0.0 (stored diagonal entries add up to a_rr)."""
    lo, hi = np.inf, -np.inf
    indptr, indices, data = A.indptr, A.indices, A.data
    for r in range(A.shape[0]):
        arr = off = 0.0
        for k in range(int(indptr[r]), int(indptr[r + 1])):
            v = float(data[k])
            if int(indices[k]) == r:
                arr = arr + v
            else:
                off = off + fabs(v)
        lo = min(lo, arr - off)
        hi = max(hi, arr + off)
    return lo, hi


def interval(A, a=None, b=None):
    "The interval as mk_filter_create resolves it: an end that is None is the Gershgorin end."
    if a is None or b is None:
        lo, hi = gershgorin(A)
        a = lo if a is None else a
        b = hi if b is None else b
    return float(a), float(b)


def apply(A, x, degree, a, b, a0, matvec=None):
    "``rho(A) x``: the steps of mk_filter_apply, each elementwise operation rounded on its own."
    mv = A.matvec if matvec is None else matvec
    c, e, p, q = coefficients(a, b, a0, degree)
    yprev, y = None, np.array(x, dtype=np.float64)
    for j in range(1, degree + 1):
        s = mv(y)
        u = c * y
        t = s - u
        yn = p[j - 1] * t
        if j > 1:
            v = q[j - 1] * yprev
            yn = yn - v
        yprev, y = y, yn
    return y


def rho(t, degree, a, b, a0):
    "The closed form ``T_d((t - c)/e) / T_d((a0 - c)/e)`` (cosh / cos forms of T_d; test arithmetic, not the library's)."
    e, c = 0.5 * (b - a), 0.5 * (b + a)

    def cheb(z):
        z = np.asarray(z, dtype=np.float64)
        out = np.empty_like(z)
        inside = np.abs(z) <= 1.0
        out[inside] = np.cos(degree * np.arccos(z[inside]))
        zo = z[~inside]
        out[~inside] = np.sign(zo) ** degree * np.cosh(degree * np.arccosh(np.abs(zo)))
        return out
    return cheb((np.asarray(t, dtype=np.float64) - c) / e) / cheb(np.array([(a0 - c) / e]))[0]


def degree_cap(a, b, a0):
    "tools.cheb_filter_degree_cap: the largest degree d with T_d(z0) <= 2**16, z0 = |a0 - c| / e; at least 1."
    z0 = abs(float(a0) - 0.5 * (float(b) + float(a))) / (0.5 * (float(b) - float(a)))
    return max(1, int(acosh(2.0 ** 16) / acosh(z0)))


def filter_for(A, nev, which="SA", degree=16, steps=None, seed=1, dots=None):
    """``(a, b, a0, pilot, d)`` as tools.cheb_filter_for chooses them: the cut at Ritz value nev (from the wanted end) of a pilot
    Lanczos run, the far end Gershgorin's, the reference point the extreme Ritz value moved outwards by its residual, and the
    degree ``min(degree, degree_cap(a, b, a0))``."""
    n = A.shape[0]
    pilot = _lanczos_ref.lanczos(A, steps=default_ncv(n, nev) if steps is None else steps, seed=seed, dots=dots)
    if len(pilot.ritz) < nev + 1:
        raise ValueError("the pilot run gave %d Ritz values, %d are needed" % (len(pilot.ritz), nev + 1))
    lo, hi = gershgorin(A)
    if which == "SA":
        a, b, a0 = float(pilot.ritz[nev]), hi, float(pilot.ritz[0] - pilot.residuals[0])
    else:
        a, b, a0 = lo, float(pilot.ritz[-1 - nev]), float(pilot.ritz[-1] + pilot.residuals[-1])
    if not a < b or a <= a0 <= b:
        raise ValueError("a0 = %r falls inside [%r, %r]" % (a0, a, b))
    return a, b, a0, pilot, min(int(degree), degree_cap(a, b, a0))


def trlan_filtered(A, nev, which, degree, a, b, a0, ncv=None, keep=None, abstol=0.0, reltol=1.0e-10, matvec_max=None,
                   start=None, seed=1, dots=np.dot):
    """The filtered cycle: thick-restart Lanczos on ``B = rho(A)`` for B's largest eigenvalues, B's estimates as a gate, the
    verification on `A` after the restart rotation.  `w` is theta_A ascending, `residNorms` the A-residuals, `pairIters` the
    cycle at which B's estimate of the pair first met the gate, `history` per cycle the largest A-residual where verified
    (`verified`: those cycles) and B's largest estimate otherwise, `anorm` / `threshold` those of A."""
    n = A.shape[0]
    if ncv is None:
        ncv = default_ncv(n, nev)
    if keep is None:
        keep = default_keep(nev, ncv)
    d = int(degree)
    if matvec_max is None:
        matvec_max = max(2 * n, ncv * d + nev)
    if which not in ("SA", "LA") or (a0 > b) != (which == "LA") or a <= a0 <= b:
        raise ValueError("which does not name the side a0 lies at")
    if not (1 <= nev < ncv <= min(n, MAX_NCV)) or not (nev <= keep < ncv) or not (1 <= d <= MAX_DEGREE):
        raise ValueError("needs 1 <= nev < ncv <= min(n, %d), nev <= keep < ncv, 1 <= degree <= %d" % (MAX_NCV, MAX_DEGREE))
    if matvec_max < ncv * d + nev:
        raise ValueError("matvec_max below ncv * degree + nev")
    m = ncv
    anorm_a = max(fabs(a), fabs(b), fabs(a0))
    thr_a = max(abstol, reltol * anorm_a)
    if start is None:
        start = csr_ref.cell_field(np.arange(n), seed) - 1.0
    start = np.ascontiguousarray(start, dtype=np.float64)
    b0 = sqrt(dots(start, start))
    V = np.zeros((m + 1, n))
    V[0] = (1.0 / b0) * start
    T = np.zeros((m, m))
    l = 0
    anorm = tmax = beta = 0.0
    nMatvec = nIter = cycles = 0
    history, verified = [], []
    first_met = np.full(nev, -1, dtype=np.int64)
    verifying = False
    cost = (m - keep) * d + nev
    while True:
        m_eff, breakdown = m, False
        for j in range(l, m):
            w = apply(A, V[j], d, a, b, a0)
            nMatvec += d
            h = np.array([dots(V[i], w) for i in range(j + 1)])
            for i in range(j + 1):
                w = w - h[i] * V[i]
            h2 = np.array([dots(V[i], w) for i in range(j + 1)])
            for i in range(j + 1):
                w = w - h2[i] * V[i]
                h[i] = h[i] + h2[i]
            alpha = float(h[j])
            T[j, j] = alpha
            tm = fabs(alpha)
            if nIter > 0:
                tm = tm + beta
            beta = sqrt(dots(w, w))
            tmax = tm if tm > tmax else tmax
            nIter += 1
            if not beta > 2.0 ** -26 * tmax:
                m_eff, breakdown = j + 1, True
                break
            if j + 1 < m:
                T[j, j + 1] = T[j + 1, j] = beta
            V[j + 1] = (1.0 / beta) * w
        cycles += 1
        theta, S, sweeps = jacobi_eigh(T[:m_eff, :m_eff])
        order = np.arange(m_eff)[::-1]                           # B's largest first, whatever `which` says
        est = np.zeros(m_eff) if breakdown else np.abs(beta * S[m_eff - 1])
        anorm = max(anorm, float(np.max(np.abs(theta))))
        gate_thr = max(abstol, reltol * anorm)
        nret = min(nev, m_eff)
        wanted = order[:nret]
        resid = float(np.max(est[wanted]))
        history.append(resid)
        met = est[wanted] <= gate_thr
        first_met[:nret][met & (first_met[:nret] < 0)] = cycles
        if nret == nev and met.all():
            verifying = True
        if breakdown:
            nx = nret
            V[:nret] = rotate(V[:m_eff], S[:, wanted])
        else:
            nx = nev
            kept = order[:keep]
            V[:keep] = rotate(V[:m], S[:, kept])
            V[keep] = V[m]
            T = np.zeros((m, m))
            for i in range(keep):
                T[i, i] = theta[kept[i]]
                T[i, keep] = T[keep, i] = beta * S[m - 1, kept[i]]
            l = keep
        converged = False
        if breakdown or verifying or nMatvec + cost > matvec_max:
            th = np.zeros(nx)
            res = np.zeros(nx)
            for i in range(nx):
                w = A.matvec(V[i])
                th[i] = dots(V[i], w)
                t = w - th[i] * V[i]
                res[i] = sqrt(dots(t, t))
            nMatvec += nx
            resid = float(np.max(res)) if nx else 0.0
            history[-1] = resid
            verified.append(cycles)
            nconv = int(np.sum(res <= thr_a))
            converged = bool(nx == nev and nconv == nev)
            if converged or breakdown or nMatvec + cost > matvec_max:
                break
    perm = np.argsort(th, kind="stable")
    return FilteredResult(th[perm].copy(), V[:nx][perm].copy(), res[perm].copy(), first_met[:nx][perm].copy(), nconv, converged,
                          breakdown, nMatvec, nIter, cycles, np.array(history), anorm_a, thr_a, resid, b0, m, keep, sweeps,
                          verified)
