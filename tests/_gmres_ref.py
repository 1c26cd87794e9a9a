"""NumPy restatement of the device GMRES(m) loop (pykrylov_amd.GMRES, csrc/mk_gmres.hip), operation by operation.
TEST INFRASTRUCTURE ONLY.

Restarted GMRES with right preconditioning; classical Gram-Schmidt, run twice per step unless ``reorth`` is false.  `A` is
anything with ``matvec`` (oracle.csr_ref.RefCsr).  ``dots(a, b)`` is the inner product: ``np.dot`` by default,
``oracle.gpu_order.stream_dot`` for the device's summation order -- every other operation rounds alike on both sides.
``precon``: None, or something applied as ``precon * v`` (``precon(v)`` if it has no ``__mul__``).
"""
from collections import namedtuple
from math import fabs, isfinite, sqrt

import numpy as np

MAX_RESTART = 128

GmresResult = namedtuple("GmresResult", "x history nMatvec nIter restarts converged precon_calls residNorm residNorm0 last_steps")


def gmres(A, b, abstol=1.0e-8, reltol=1.0e-6, guess=None, matvec_max=None, restart=30, reorth=True, precon=None, dots=np.dot):
    b = np.ascontiguousarray(b, dtype=np.float64)
    n = b.shape[0]
    if not 1 <= restart <= MAX_RESTART:
        raise ValueError("restart must be 1 .. %d" % MAX_RESTART)
    m = min(int(restart), n)
    if matvec_max is None:
        matvec_max = 2 * n
    calls = [0]

    def apply(v):
        if precon is None:
            return v
        calls[0] += 1
        y = precon * v if hasattr(precon, "__mul__") else precon(v)
        return np.ascontiguousarray(y, dtype=np.float64)

    nMatvec = nIter = restarts = last = 0
    if guess is None:
        x = np.zeros(n)
        r = b.copy()
    else:
        x = np.array(guess, dtype=np.float64)
        r = b - A.matvec(x)
        nMatvec = 1
    beta = sqrt(dots(r, r))
    resid0 = resid = beta
    threshold = max(abstol, reltol * resid0)
    history = [beta]
    converged = beta <= threshold
    V = np.zeros((m + 1, n))
    R = np.zeros((m, m))
    c, s, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
    while beta > threshold and nMatvec < matvec_max:                 # one cycle
        V[0] = (1.0 / beta) * r
        g[0] = beta
        j = 0
        stopped = False
        while j < m and nMatvec < matvec_max:
            w = A.matvec(apply(V[j]))
            nMatvec += 1
            h = np.array([dots(V[i], w) for i in range(j + 1)])
            for i in range(j + 1):
                w = w - h[i] * V[i]
            if reorth:
                h2 = np.array([dots(V[i], w) for i in range(j + 1)])
                for i in range(j + 1):
                    w = w - h2[i] * V[i]
                    h[i] = h[i] + h2[i]
            hn = sqrt(dots(w, w))
            a = h
            for i in range(j):
                t = c[i] * a[i] + s[i] * a[i + 1]
                a[i + 1] = c[i] * a[i + 1] - s[i] * a[i]
                a[i] = t
            with np.errstate(all="ignore"):
                rr = np.sqrt(np.float64(a[j] * a[j] + hn * hn))
                cj, sj = np.float64(a[j]) / rr, np.float64(hn) / rr
            gnext = -sj * g[j]
            est = fabs(gnext)
            history.append(float(est))
            nIter += 1
            resid = float(est)
            bad = not (isfinite(hn) and isfinite(rr) and isfinite(est)) or rr == 0.0
            if not bad:
                R[:j, j] = a[:j]
                R[j, j] = rr
                c[j], s[j] = cj, sj
                g[j + 1] = gnext
                g[j] = cj * g[j]
                j += 1
            last = j
            converged = (not bad) and est <= threshold
            if bad or est <= threshold or not hn > 0.0:
                stopped = True
                break
            if j < m:
                V[j] = (1.0 / hn) * w
        if j > 0:                                                    # the cycle end (nothing to add after a discarded first step)
            y = np.zeros(j)
            for i in range(j - 1, -1, -1):
                t = g[i]
                for k in range(i + 1, j):
                    t = t - R[i, k] * y[k]
                y[i] = t / R[i, i]
            u = np.zeros(n)
            for i in range(j):
                u = u + y[i] * V[i]
            x = x + apply(u)
        if stopped or nMatvec >= matvec_max:
            break
        r = b - A.matvec(x)
        nMatvec += 1
        beta = sqrt(dots(r, r))
        restarts += 1
        resid = beta
        converged = beta <= threshold
    return GmresResult(x, np.array(history), nMatvec, nIter, restarts, bool(converged), calls[0], resid, resid0, last)
