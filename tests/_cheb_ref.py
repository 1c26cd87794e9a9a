"""NumPy restatement of the device Chebyshev polynomial preconditioner (pykrylov_amd/csrc/mk_cheb.hip), operation by
operation: the coefficients, the Gershgorin bound and the apply -- written with the oracle's CSR product and the elementwise
order of the device kernels, so that equal inputs give equal bits.  Test infrastructure only."""
import numpy as np

RATIO = 30.0          # default lmin = lmax / 30 (the convention of hypre and Ifpack2; not a tuned number)
MAX_DEGREE = 64


def coefficients(lmin, lmax, degree):
    """``(c0, c1, c2)`` of Saad's Alg. 12.1 in the order the library computes them, one rounding per operation."""
    lmin, lmax = float(lmin), float(lmax)
    theta = 0.5 * (lmax + lmin)
    delta = 0.5 * (lmax - lmin)
    sigma = theta / delta
    c0 = 1.0 / theta
    rho = 1.0 / sigma
    c1, c2 = np.empty(degree), np.empty(degree)
    for j in range(degree):
        rho_j = 1.0 / (2.0 * sigma - rho)
        c1[j] = rho_j * rho
        c2[j] = (2.0 * rho_j) / delta
        rho = rho_j
    return c0, c1, c2


def diagonal(A):
    """The stored diagonal entry of every row (the first one stored), NaN where none is stored."""
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    pos = np.flatnonzero(A.indices == rows)
    d = np.full(n, np.nan)
    d[rows[pos][::-1]] = A.data[pos][::-1]            # (the first stored one wins)
    return d


def gershgorin(A, scale_diag=False):
    """max_r sum_j |a_rj| (scaled: / |a_rr|), every row added left to right in stored order."""
    n = A.shape[0]
    start = A.indptr[:-1].astype(np.int64)
    length = np.diff(A.indptr).astype(np.int64)
    s = np.zeros(n)
    k = 0
    while True:
        live = length > k
        if not live.any():
            break
        s[live] = s[live] + np.abs(A.data[start[live] + k])
        k += 1
    if scale_diag:
        s = s / np.abs(diagonal(A))
    return float(s.max())


def interval(A, lmin=None, lmax=None, ratio=RATIO, scale_diag=False):
    lmax = gershgorin(A, scale_diag) if lmax is None else float(lmax)
    lmin = lmax / ratio if lmin is None else float(lmin)
    return lmin, lmax


def apply(A, r, degree, lmin, lmax, scale_diag=False, matvec=None):
    """z = p_k(A) r: the Chebyshev iteration for A z = r from z = 0 on [lmin, lmax] (scaled: for D^-1 A z = D^-1 r).
    `matvec`: the product (default the oracle's left-to-right CSR product of `A`)."""
    mv = A.matvec if matvec is None else matvec
    c0, c1, c2 = coefficients(lmin, lmax, degree)
    r = np.ascontiguousarray(r, dtype=np.float64)
    dinv = 1.0 / diagonal(A) if scale_diag else None
    res = dinv * r if scale_diag else r.copy()
    d = res * c0
    out = d.copy()
    for j in range(degree):
        s = mv(d)
        if scale_diag:
            s = dinv * s
        rv = res - s
        dn = c1[j] * d
        t = c2[j] * rv
        dn = dn + t
        out = out + dn
        d, res = dn, rv
    return out


class HostCheb(object):
    """The reference apply as an operator for the oracle's solvers (``precon * r``)."""

    def __init__(self, A, degree, lmin, lmax, scale_diag=False):
        self.A, self.args = A, (degree, lmin, lmax, scale_diag)
        self.shape = A.shape
        self.calls = 0

    def __mul__(self, r):
        self.calls += 1
        return apply(self.A, r, *self.args)

    __call__ = __mul__
