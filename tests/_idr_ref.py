"""NumPy restatement of the device IDR(s) loop (pykrylov_amd.IDR, csrc/mk_idr.hip), operation by operation.
TEST INFRASTRUCTURE ONLY.

IDR(s) in its biorthogonal form (van Gijzen and Sonneveld, ACM TOMS 38, 2011) with right preconditioning.  `idr` is the
device's loop: the new g is made orthogonal to the earlier shadow vectors by ONE batch of s dots and a small triangular
solve.  `idr_textbook` is the paper's form, which orthogonalises against one shadow vector after the other; it is here
for comparison only.  `A` is anything with ``matvec`` (oracle.csr_ref.RefCsr).  ``dots(a, b)`` is the inner product:
``np.dot`` by default, ``oracle.gpu_order.stream_dot`` for the device's summation order -- every other operation rounds
alike on both sides; every accumulation runs over ascending columns.  ``precon``: None, or something applied as
``precon * v`` (``precon(v)`` if it has no ``__mul__``).
"""
from collections import namedtuple
from math import fabs, isfinite, sqrt

import numpy as np

from oracle import csr_ref

MAX_S = 32
KAPPA = 0.7

IdrResult = namedtuple("IdrResult", "x history nMatvec nIter cycles converged breakdown precon_calls residNorm residNorm0 s")


def shadow_rows(s, n, seed=1):
    """Row k is the hashed field of seed + k, moved to [-0.5, 0.5) (mk_cell_field - 1.0)."""
    return np.array([csr_ref.cell_field(np.arange(n), seed + k) - 1.0 for k in range(s)]).reshape(s, n)


def _start(A, b, guess, matvec_max, s, seed, shadow, abstol, reltol, dots):
    b = np.ascontiguousarray(b, dtype=np.float64)
    n = b.shape[0]
    if not 1 <= s <= MAX_S:
        raise ValueError("s must be 1 .. %d" % MAX_S)
    if shadow is None:
        s = min(int(s), n)
        P = shadow_rows(s, n, seed)
    else:
        P = np.ascontiguousarray(shadow, dtype=np.float64)
        s = P.shape[0]
    if matvec_max is None:
        matvec_max = 2 * n
    nMatvec = 0
    if guess is None:
        x = np.zeros(n)
        r = b.copy()
    else:
        x = np.array(guess, dtype=np.float64)
        r = b - A.matvec(x)
        nMatvec = 1
    normr = sqrt(dots(r, r))
    return n, s, P, matvec_max, nMatvec, x, r, normr, max(abstol, reltol * normr)


def _applier(precon, calls):
    def apply(v):
        if precon is None:
            return v
        calls[0] += 1
        y = precon * v if hasattr(precon, "__mul__") else precon(v)
        return np.ascontiguousarray(y, dtype=np.float64)
    return apply


def _omega(t, r, normr, dots):
    """om = <t,r> / <t,t>, enlarged to kappa / rho * om when rho = |<t,r>| / (||t|| ||r||) < kappa; None on breakdown."""
    tt, tr = dots(t, t), dots(t, r)
    with np.errstate(all="ignore"):
        om = np.float64(tr) / np.float64(tt)
        rho = np.float64(fabs(tr)) / np.float64(sqrt(tt) * normr) if tt >= 0.0 else np.float64("nan")
        if rho < KAPPA:
            om = om * (np.float64(KAPPA) / rho)
    om = float(om)
    if tt == 0.0 or om == 0.0 or not isfinite(om):
        return None
    return om


def idr(A, b, abstol=1.0e-8, reltol=1.0e-6, guess=None, matvec_max=None, s=4, seed=1, shadow=None, precon=None, dots=np.dot):
    n, s, P, matvec_max, nMatvec, x, r, normr, threshold = _start(A, b, guess, matvec_max, s, seed, shadow, abstol, reltol, dots)
    calls = [0]
    apply = _applier(precon, calls)
    resid0 = normr
    history = [normr]
    nIter = cycles = breakdown = 0
    G, U, M = np.zeros((s, n)), np.zeros((s, n)), np.eye(s)
    f, c, a = np.zeros(s), np.zeros(s), np.zeros(s)
    om = 1.0
    while normr > threshold and nMatvec < matvec_max:
        for i in range(s):
            f[i] = dots(P[i], r)
        stopped = False
        for k in range(s):
            for i in range(k, s):                                   # M[k:, k:] c = f[k:]
                t = f[i]
                for j in range(k, i):
                    t = t - M[i, j] * c[j]
                with np.errstate(all="ignore"):
                    c[i] = np.float64(t) / M[i, i]
            v = r
            u = np.zeros(n)
            with np.errstate(all="ignore"):
                for i in range(k, s):
                    v = v - c[i] * G[i]
                    u = u + c[i] * U[i]
                v = apply(v)
                u = u + om * v
            g = A.matvec(u)
            nMatvec += 1
            m = np.array([dots(P[i], g) for i in range(s)])
            with np.errstate(all="ignore"):
                for i in range(k):                                  # M[:k, :k] a = m[:k]
                    t = m[i]
                    for j in range(i):
                        t = t - M[i, j] * a[j]
                    a[i] = np.float64(t) / M[i, i]
                for i in range(k):
                    g = g - a[i] * G[i]
                    u = u - a[i] * U[i]
                for i in range(k, s):                               # M[k:, k] = m[k:] - M[k:, :k] a
                    t = m[i]
                    for j in range(k):
                        t = t - M[i, j] * a[j]
                    M[i, k] = t
            G[k], U[k] = g, u
            nIter += 1
            if M[k, k] == 0.0 or not isfinite(M[k, k]):             # x stays the last iterate
                breakdown = 1
                history.append(normr)
                stopped = True
                break
            with np.errstate(all="ignore"):
                beta = float(np.float64(f[k]) / M[k, k])
                r = r - beta * g
                x = x + beta * u
                normr = sqrt(dots(r, r))
                for i in range(k + 1, s):
                    f[i] = f[i] - beta * M[i, k]
            history.append(normr)
            if not normr > threshold or nMatvec >= matvec_max:
                stopped = True
                break
        if stopped:
            break
        v = apply(r)
        t = A.matvec(v)
        nMatvec += 1
        nIter += 1
        new_om = _omega(t, r, normr, dots)
        if new_om is None:
            breakdown = 2
            history.append(normr)
            break
        om = new_om
        with np.errstate(all="ignore"):
            r = r - om * t
            x = x + om * v
            normr = sqrt(dots(r, r))
        history.append(normr)
        cycles += 1
    return IdrResult(x, np.array(history), nMatvec, nIter, cycles, bool(normr <= threshold), breakdown, calls[0], normr,
                     resid0, s)


def idr_textbook(A, b, abstol=1.0e-8, reltol=1.0e-6, guess=None, matvec_max=None, s=4, seed=1, shadow=None, precon=None,
                 dots=np.dot):
    """The sequential biorthogonalisation of the paper: g is made orthogonal to p_0, p_1, .. one after the other, each
    coefficient from a dot with the g of that moment."""
    n, s, P, matvec_max, nMatvec, x, r, normr, threshold = _start(A, b, guess, matvec_max, s, seed, shadow, abstol, reltol, dots)
    calls = [0]
    apply = _applier(precon, calls)
    resid0 = normr
    history = [normr]
    nIter = cycles = breakdown = 0
    G, U, M = np.zeros((s, n)), np.zeros((s, n)), np.eye(s)
    om = 1.0
    while normr > threshold and nMatvec < matvec_max:
        f = np.array([dots(P[i], r) for i in range(s)])
        stopped = False
        for k in range(s):
            c = np.linalg.solve(M[k:, k:], f[k:])
            v = apply(r - c @ G[k:])
            u = c @ U[k:] + om * v
            g = A.matvec(u)
            nMatvec += 1
            nIter += 1
            for i in range(k):
                alpha = dots(P[i], g) / M[i, i]
                g = g - alpha * G[i]
                u = u - alpha * U[i]
            for i in range(k, s):
                M[i, k] = dots(P[i], g)
            G[k], U[k] = g, u
            if M[k, k] == 0.0 or not isfinite(M[k, k]):
                breakdown = 1
                history.append(normr)
                stopped = True
                break
            beta = f[k] / M[k, k]
            r = r - beta * g
            x = x + beta * u
            normr = sqrt(dots(r, r))
            f[k + 1:] = f[k + 1:] - beta * M[k + 1:, k]
            history.append(normr)
            if not normr > threshold or nMatvec >= matvec_max:
                stopped = True
                break
        if stopped:
            break
        v = apply(r)
        t = A.matvec(v)
        nMatvec += 1
        nIter += 1
        new_om = _omega(t, r, normr, dots)
        if new_om is None:
            breakdown = 2
            history.append(normr)
            break
        om = new_om
        r = r - om * t
        x = x + om * v
        normr = sqrt(dots(r, r))
        history.append(normr)
        cycles += 1
    return IdrResult(x, np.array(history), nMatvec, nIter, cycles, bool(normr <= threshold), breakdown, calls[0], normr,
                     resid0, s)
