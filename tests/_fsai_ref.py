"""NumPy restatement of the device FSAI preconditioner (pykrylov_amd/csrc/mk_fsai.hip), operation by operation: the pattern
(the stored lower triangle, or that of a symbolic power), the per-row dense solve in the order the library documents
(include/mikrylov.h, mk_fsai_create) and the apply with the oracle's CSR product -- so that equal inputs give equal bits.
Test infrastructure only."""
import numpy as np

from oracle.csr_ref import RefCsr

MAX_ROW = 32


def lower_pattern(indptr, indices):
    """``(indptr, indices)`` of the stored entries (i, j) with j <= i, in stored order."""
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    keep = np.asarray(indices) <= rows
    ip = np.zeros(n + 1, dtype=np.int64)
    ip[1:] = np.cumsum(np.bincount(rows[keep], minlength=n))
    return ip, np.asarray(indices)[keep].astype(np.int64)


def boolean_power(indptr, indices, power):
    """Rows of the pattern of ``A**power`` as sorted lists, by repeated union of rows (plain Python sets)."""
    n = len(indptr) - 1
    rows = [list(map(int, indices[indptr[i]:indptr[i + 1]])) for i in range(n)]
    cur = rows
    for _ in range(power - 1):
        nxt = []
        for i in range(n):
            s = set()
            for j in cur[i]:
                s.update(rows[j])
            nxt.append(sorted(s))
        cur = nxt
    return cur


def power_pattern(indptr, indices, power):
    """``(indptr, indices)`` of the lower triangle of the pattern of ``A**power``."""
    if power == 1:
        return lower_pattern(indptr, indices)
    rows = boolean_power(indptr, indices, power)
    low = [[j for j in r if j <= i] for i, r in enumerate(rows)]
    ip = np.zeros(len(low) + 1, dtype=np.int64)
    ip[1:] = np.cumsum([len(r) for r in low])
    return ip, np.array([j for r in low for j in r], dtype=np.int64)


def _row(A_rows, P):
    """Row of G for the pattern columns P (ascending, the last one the row itself): gather, Cholesky, the last column of the
    inverse and the scaling -- every entry one sequential sum, one rounding per operation.  Returns (g, ok)."""
    m = len(P)
    sqrt = np.sqrt
    L = [[0.0] * (a + 1) for a in range(m)]
    for a in range(m):
        lookup = A_rows[P[a]]
        for b in range(a + 1):
            L[a][b] = lookup.get(P[b], 0.0)
    ok = True
    with np.errstate(all="ignore"):
        for b in range(m):
            s = np.float64(L[b][b])
            for k in range(b):
                s = s - np.float64(L[b][k]) * np.float64(L[b][k])
            if not (s > 0.0) or not np.isfinite(s):
                ok = False
            d = sqrt(s)
            L[b][b] = d
            for a in range(b + 1, m):
                s = np.float64(L[a][b])
                for k in range(b):
                    s = s - np.float64(L[a][k]) * np.float64(L[b][k])
                L[a][b] = s / d
        y = [np.float64(0.0)] * m
        y[m - 1] = np.float64(1.0) / L[m - 1][m - 1]
        for a in range(m - 1, -1, -1):
            s = y[a]
            for k in range(m - 1, a, -1):
                s = s - L[k][a] * y[k]
            y[a] = s / L[a][a]
        sd = sqrt(y[m - 1])
        return [v / sd for v in y], ok


def factor(A, pattern=None, power=1):
    """G as a RefCsr on `pattern` (default: the lower triangle of the pattern of ``A**power``).  Raises ValueError naming the
    smallest row whose dense solve breaks down."""
    n = A.shape[0]
    ip, ix = power_pattern(A.indptr, A.indices, power) if pattern is None else pattern
    ip, ix = np.asarray(ip, dtype=np.int64), np.asarray(ix, dtype=np.int64)
    longest = int(np.diff(ip).max()) if n else 0
    if longest > MAX_ROW:
        raise ValueError("row %d has %d entries" % (int(np.argmax(np.diff(ip) > MAX_ROW)), longest))
    # the lower part of every row of A as {column: value}
    A_rows = []
    for i in range(n):
        lo, hi = int(A.indptr[i]), int(A.indptr[i + 1])
        A_rows.append({int(c): v for c, v in zip(A.indices[lo:hi], A.data[lo:hi]) if c <= i})
    vals = np.empty(len(ix))
    for i in range(n):
        P = [int(c) for c in ix[ip[i]:ip[i + 1]]]
        assert P and P[-1] == i and all(P[k] < P[k + 1] for k in range(len(P) - 1)), "row %d of the pattern" % i
        g, ok = _row(A_rows, P)
        if not ok:
            raise ValueError("breakdown in row %d" % i)
        vals[ip[i]:ip[i + 1]] = g
    return RefCsr(ip, ix, vals, (n, n))


def apply(G, r):
    """z = G' (G r) with the oracle's left-to-right CSR product of G and of its transpose."""
    return G.transpose().matvec(G.matvec(r))


class HostFsai(object):
    """The reference apply as an operator for the oracle's solvers (``precon * r``)."""

    def __init__(self, G):
        self.G = G
        self.shape = G.shape
        self.calls = 0

    def __mul__(self, r):
        self.calls += 1
        return apply(self.G, r)

    __call__ = __mul__
