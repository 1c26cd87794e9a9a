"""NumPy restatement of the device's preconditioned CG (csrc/mk_pcg.hip).   TEST INFRASTRUCTURE ONLY.

The textbook loop, z = M r, p = z + beta p, with beta = <r,z>' / <r,z> (standard) or -alpha <q,z'> / <r,z> (flexible: the
Polak-Ribiere form <z', r' - r> / <r,z> without storing the old r).  Every elementwise update rounds each operation on its
own, as the device does.  `A` is anything with ``matvec`` (oracle.csr_ref.RefCsr).  ``dots(a, b, site)`` is the inner
product; the site is "pcg.pq" for <p, A p>, which the device forms in the product kernel, and a stream site for the others
(``oracle.gpu_order.GpuDots(n, ["pcg.pq"], geometry)`` reproduces the device's summation order; the default is ``np.dot``).
``precon``: None, or something applied as ``precon * v`` (``precon(v)`` if it has no ``__mul__``).  Without a
preconditioner z is r and <r,z> is <r,r>: no second inner product is formed."""
from collections import namedtuple
from math import isfinite, sqrt

import numpy as np

PcgResult = namedtuple("PcgResult", "x history nMatvec nIter converged definite breakdown precon_calls residNorm residNorm0 p")


def _np_dot(a, b, site):
    return float(np.dot(a, b))


def pcg(A, b, abstol=1.0e-8, reltol=1.0e-6, guess=None, matvec_max=None, precon=None, flexible=False, check_curvature=True,
        dots=None):
    dots = dots or _np_dot
    b = np.ascontiguousarray(b, dtype=np.float64)
    n = b.shape[0]
    if matvec_max is None:
        matvec_max = 2 * n
    calls = [0]

    def apply(v):
        calls[0] += 1
        y = precon * v if hasattr(precon, "__mul__") else precon(v)
        return np.ascontiguousarray(y, dtype=np.float64)

    nMatvec = nIter = 0
    if guess is None:
        x = np.zeros(n)
        r = b.copy()
    else:
        x = np.array(guess, dtype=np.float64)
        r = b - A.matvec(x)
        nMatvec = 1
    rr = float(dots(r, r, "pcg.rr0"))
    resid0 = resid = sqrt(rr) if rr >= 0 else float("nan")
    thr = max(abstol, reltol * resid0)
    history = [resid0]
    definite, breakdown = True, 0
    p = np.zeros(n)

    def done():
        return PcgResult(x, np.array(history), nMatvec, nIter, bool(resid <= thr), definite, breakdown, calls[0], resid, resid0, p)

    if resid0 <= thr or nMatvec >= matvec_max:
        return done()
    if precon is None:
        z, rz = r, rr
    else:
        z = apply(r)
        rz = float(dots(r, z, "pcg.rz0"))
    if not rz > 0 or not isfinite(rz):
        breakdown = 2
        return done()
    p = z.copy()
    while True:
        q = A.matvec(p)
        nMatvec += 1
        pq = float(dots(p, q, "pcg.pq"))
        if check_curvature and not pq > 0:
            definite, breakdown = False, 1
            return done()
        with np.errstate(all="ignore"):
            alpha = float(np.float64(rz) / np.float64(pq))
            x = x + alpha * p
            r = r - alpha * q
        rr = float(dots(r, r, "pcg.rr"))
        resid = sqrt(rr) if rr >= 0 else float("nan")
        history.append(resid)
        nIter += 1
        if resid <= thr or nMatvec >= matvec_max:
            return done()
        if precon is None:
            z, rz_new = r, rr
        else:
            z = apply(r)
            rz_new = float(dots(r, z, "pcg.rz"))
        qz = float(dots(q, z, "pcg.qz")) if flexible else 0.0
        if not rz_new > 0 or not isfinite(rz_new):
            breakdown = 2
            return done()
        beta = -(alpha * qz) / rz if flexible else rz_new / rz
        p = z + beta * p
        rz = rz_new
