"""NumPy restatement of the device's multi-shift CG (csrc/mk_mscg.hip).   TEST INFRASTRUCTURE ONLY.

``(A + sigma_k I) x_k = b`` for every shift in the Krylov space of one: CG on `A` itself (``x0 = 0``, ``r = p = b``) and per
shift ``x_k``, ``p_k`` and ``zeta_k`` with ``r_k = zeta_k r`` (Frommer and Maass; Jegerlehner, hep-lat/9612014).  Every
elementwise update and every scalar expression rounds each operation on its own and in the device's order.  `A` is anything
with ``matvec`` (oracle.csr_ref.RefCsr).  ``dots(a, b, site)`` is the inner product; the site is "mscg.pq" for <p, A p>, which
the device forms in the product kernel, and a stream site ("mscg.rr0", "mscg.rr") for the others
(``oracle.gpu_order.GpuDots(n, ["mscg.pq"], geometry)`` reproduces the device's summation order; the default is ``np.dot``).

A shift whose ``|zeta_k| ||r||`` has reached the threshold is frozen after the updates of that pass: its ``x_k`` has the
pass's update, its ``p_k`` has not, and neither its vectors nor its scalars are touched again.  The loop ends when no shift
is active or at `matvec_max`; in the pass that ends it the ``x_k`` updates still run and no ``p`` is written."""
from collections import namedtuple
from math import isfinite, sqrt

import numpy as np

MscgResult = namedtuple("MscgResult", "xs x zeta residNorms shiftIters history history2 nMatvec nIter converged definite "
                                      "breakdown residNorm residNorm0 threshold r p ps")


def _np_dot(a, b, site):
    return float(np.dot(a, b))


def _bad(v):
    return v == 0.0 or not isfinite(v)


def mscg(A, b, shifts, abstol=1.0e-8, reltol=1.0e-6, matvec_max=None, check_curvature=True, dots=None):
    dots = dots or _np_dot
    b = np.ascontiguousarray(b, dtype=np.float64)
    n = b.shape[0]
    sig = [float(s) for s in shifts]
    ns = len(sig)
    if matvec_max is None:
        matvec_max = 2 * n
    xs = np.zeros((ns, n))
    ps = np.tile(b, (ns, 1))
    r, p = b.copy(), b.copy()
    zprev, zcur = [1.0] * ns, [1.0] * ns
    active = [True] * ns
    froze = [-1] * ns
    nMatvec = nIter = 0
    rr = float(dots(r, r, "mscg.rr0"))
    resid0 = sqrt(rr) if rr >= 0 else float("nan")
    resk = [resid0] * ns
    thr = max(abstol, reltol * resid0)
    history, history2 = [resid0], [resid0]
    definite, breakdown = True, 0

    def done():
        top = 0.0
        for v in resk:
            if v > top:
                top = v
        return MscgResult(xs, xs[0], np.array(zcur), np.array(resk), np.array(froze), np.array(history), np.array(history2),
                          nMatvec, nIter, not any(active), definite, breakdown, top, resid0, thr, r, p, ps)

    if resid0 <= thr:                                        # (a zero right-hand side: every x_k = 0 solves its system)
        active, froze = [False] * ns, [0] * ns
        return done()
    if nMatvec >= matvec_max:
        return done()
    if not rr > 0 or not isfinite(rr):
        breakdown = 2
        return done()
    alpha_prev, beta_prev = 1.0, 0.0
    while True:
        q = A.matvec(p)
        nMatvec += 1
        pq = float(dots(p, q, "mscg.pq"))
        if check_curvature and not pq > 0:
            definite, breakdown = False, 1
            return done()
        with np.errstate(all="ignore"):
            alpha = float(np.float64(rr) / np.float64(pq))
            znew, alk, broke = list(zcur), [0.0] * ns, False
            for k in range(ns):
                if not active[k]:
                    continue
                den = float((np.float64(zprev[k]) * alpha_prev) * (1.0 + np.float64(sig[k]) * alpha)
                            + (np.float64(alpha) * beta_prev) * (np.float64(zprev[k]) - zcur[k]))
                znew[k] = float(((np.float64(zcur[k]) * zprev[k]) * alpha_prev) / np.float64(den))
                alk[k] = float((np.float64(alpha) * znew[k]) / np.float64(zcur[k]))
                broke = broke or _bad(den) or _bad(znew[k])
            if broke:                                        # nothing is updated: every x_k is its last iterate
                breakdown = 2
                return done()
            r = r - alpha * q
        rr_new = float(dots(r, r, "mscg.rr"))
        resid = sqrt(rr_new) if rr_new >= 0 else float("nan")
        history.append(resid)
        nIter += 1
        entered = list(active)
        top = 0.0
        for k in range(ns):
            if not entered[k]:
                continue
            resk[k] = abs(znew[k]) * resid
            if resk[k] <= thr:
                active[k], froze[k] = False, nIter
            if resk[k] > top:
                top = resk[k]
            zprev[k], zcur[k] = zcur[k], znew[k]
        history2.append(top)
        go = any(active) and nMatvec < matvec_max
        if go and (not rr_new > 0 or not isfinite(rr_new)):
            breakdown, go = 2, False
        with np.errstate(all="ignore"):
            beta = float(np.float64(rr_new) / np.float64(rr))
            for k in range(ns):
                if not entered[k]:
                    continue
                pk = ps[k]
                xs[k] = xs[k] + alk[k] * pk
                if go and active[k]:
                    ratio = float(np.float64(zcur[k]) / np.float64(zprev[k]))
                    bk = beta * (ratio * ratio)
                    ps[k] = zcur[k] * r + bk * pk
            if not go:
                return done()
            p = r + beta * p
        rr, alpha_prev, beta_prev = rr_new, alpha, beta
