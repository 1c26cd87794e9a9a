"""CPU restatement of the incomplete factorizations ILU(0) / IC(0) and their triangular solves (pykrylov_amd/csrc/mk_ilu.hip,
include/mikrylov.h): the same operations in the same order, so that the device's factors and applies can be compared bit
for bit.  Python floats are IEEE doubles; each `a - b * c` rounds the product, then the difference, like the device
(-ffp-contract=off); division and sqrt are correctly rounded on both sides.

* `ilu0` / `ic0`: per-row reference of the factors (plain Python loops; small matrices).
* `levels`: the rows of each sweep by level (vectorised Kahn order; large matrices).
* `apply`: M^-1 r per level, vectorised over the level's rows, one column position at a time (large matrices).
* `apply_rows`: the same row by row (small matrices).
"""
import math

import numpy as np


def diag_positions(indptr, indices):
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    hit = np.flatnonzero(indices == rows)
    if hit.size != n:
        missing = np.setdiff1d(np.arange(n), rows[hit])
        raise ValueError('row %d stores no diagonal entry' % missing[0])
    return hit.astype(np.int64)


def ilu0(indptr, indices, data):
    """ILU(0), IKJ form: values on the pattern (L strictly lower, unit diagonal implied; U from the diagonal on)."""
    ip, ix = [int(v) for v in indptr], [int(v) for v in indices]
    w = [float(v) for v in data]
    dg = [int(v) for v in diag_positions(indptr, indices)]
    n = len(ip) - 1
    for i in range(n):
        p1 = ip[i + 1]
        for pk in range(ip[i], dg[i]):
            k = ix[pk]
            wk = w[pk] / w[dg[k]]
            w[pk] = wk
            p, q, qe = pk + 1, dg[k] + 1, ip[k + 1]
            while p < p1 and q < qe:
                if ix[p] == ix[q]:
                    w[p] = w[p] - wk * w[q]
                    p += 1
                    q += 1
                elif ix[p] < ix[q]:
                    p += 1
                else:
                    q += 1
        if w[dg[i]] == 0.0:
            raise ZeroDivisionError('zero pivot in row %d' % i)
    return np.array(w, dtype=np.float64)


def ic0(indptr, indices, data):
    """IC(0) on a symmetric pattern: L on the lower part and the diagonal, mirrored into the upper positions."""
    ip, ix = [int(v) for v in indptr], [int(v) for v in indices]
    w = [float(v) for v in data]
    dg = [int(v) for v in diag_positions(indptr, indices)]
    n = len(ip) - 1
    for i in range(n):
        p0 = ip[i]
        for pk in range(p0, dg[i]):
            k = ix[pk]
            s = w[pk]
            p, q = p0, ip[k]
            while p < pk and q < dg[k]:
                if ix[p] == ix[q]:
                    s = s - w[p] * w[q]
                    p += 1
                    q += 1
                elif ix[p] < ix[q]:
                    p += 1
                else:
                    q += 1
            w[pk] = s / w[dg[k]]
        d = w[dg[i]]
        for p in range(p0, dg[i]):
            d = d - w[p] * w[p]
        if not d > 0.0:
            raise ArithmeticError('breakdown in row %d' % i)
        w[dg[i]] = math.sqrt(d)
    for i in range(n):                                       # U = L^T
        for p in range(dg[i] + 1, ip[i + 1]):
            j = ix[p]
            lo, hi = ip[j], dg[j]
            q = lo + int(np.searchsorted(ix[lo:hi], i))
            w[p] = w[q]
    return np.array(w, dtype=np.float64)


def levels(indptr, indices, forward=True):
    """List of row arrays, one per level of the sweep (rows ascending within a level)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    dep = (indices < rows) if forward else (indices > rows)
    r, c = rows[dep], indices[dep]                           # row r waits for row c
    count = np.bincount(r, minlength=n)
    order = np.argsort(c, kind='stable')                     # dependents of each row, as a CSR over c
    waiters = r[order]
    start = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))])
    out = []
    front = np.flatnonzero(count == 0)
    while front.size:
        out.append(front)
        lens = start[front + 1] - start[front]
        if lens.sum() == 0:
            break
        pos = np.repeat(start[front] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(lens.sum())
        hit = waiters[pos]
        dec = np.bincount(hit, minlength=n)
        count -= dec
        cand = np.unique(hit)
        front = cand[count[cand] == 0]
    return out


RUN_MAX = 2048       # levels of one fused run (MK_ILU_RUN_MAX, csrc/mk_ilu.hip)
BLOCK = 256          # rows per workgroup


def plan(level_widths, fuse, run_max=RUN_MAX):
    """The launches of one sweep as mk_ilu_plan lays them out: a list of (first level, one past the last level, workgroups).
    A level of more than `fuse` rows is a launch of its own over ceil(rows / 256) workgroups; consecutive levels of at most
    `fuse` rows each are one launch of ONE workgroup, cut after `run_max` levels; `fuse` = 0: one launch per level."""
    out = []
    L, n = 0, len(level_widths)
    while L < n:
        if fuse > 0 and level_widths[L] <= fuse:
            e = L + 1
            while e < n and e - L < run_max and level_widths[e] <= fuse:
                e += 1
            out.append((L, e, 1))
            L = e
        else:
            out.append((L, L + 1, max(1, -(-int(level_widths[L]) // BLOCK))))
            L += 1
    return out


def apply(indptr, indices, vals, r, kind='ilu0', lev=None):
    """y = M^-1 r level by level (vectorised over a level's rows); the order of every row's subtractions is the column
    order, as on the device.  `lev` = (levels(forward), levels(backward)) to reuse an analysis."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    dg = diag_positions(indptr, indices)
    fw, bw = lev if lev is not None else (levels(indptr, indices, True), levels(indptr, indices, False))
    t = np.array(r, dtype=np.float64, copy=True)
    for R in fw:
        p0, ln = indptr[R], dg[R] - indptr[R]
        s = t[R]
        for k in range(int(ln.max()) if R.size else 0):
            m = ln > k
            p = p0[m] + k
            s[m] = s[m] - vals[p] * t[indices[p]]
        if kind == 'ic0':
            s = s / vals[dg[R]]
        t[R] = s
    for R in bw:
        p0, ln = dg[R] + 1, indptr[R + 1] - dg[R] - 1
        s = t[R]
        for k in range(int(ln.max()) if R.size else 0):
            m = ln > k
            p = p0[m] + k
            s[m] = s[m] - vals[p] * t[indices[p]]
        t[R] = s / vals[dg[R]]
    return t


def apply_rows(indptr, indices, vals, r, kind='ilu0'):
    """The same as `apply`, row by row in plain Python."""
    ip, ix = [int(v) for v in indptr], [int(v) for v in indices]
    v = [float(x) for x in vals]
    dg = [int(x) for x in diag_positions(indptr, indices)]
    n = len(ip) - 1
    t = [float(x) for x in r]
    for i in range(n):
        s = t[i]
        for p in range(ip[i], dg[i]):
            s = s - v[p] * t[ix[p]]
        t[i] = s / v[dg[i]] if kind == 'ic0' else s
    for i in range(n - 1, -1, -1):
        s = t[i]
        for p in range(dg[i] + 1, ip[i + 1]):
            s = s - v[p] * t[ix[p]]
        t[i] = s / v[dg[i]]
    return np.array(t, dtype=np.float64)


def factors_dense(indptr, indices, vals, kind='ilu0'):
    """(L, U) as dense arrays (small matrices): ILU(0) L unit lower; IC(0) L lower with its diagonal, U = L^T."""
    n = len(indptr) - 1
    F = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    F[rows, indices] = vals
    if kind == 'ic0':
        L = np.tril(F)
        return L, L.T.copy()
    return np.tril(F, -1) + np.eye(n), np.triu(F)


class HostIlu(object):
    """A factor as a HOST preconditioner (``precon * r``): the reference apply of the given values -- what the solver's
    callback path runs.  `symmetric` so that MINRES' check of the preconditioner treats it like the device object."""

    def __init__(self, indptr, indices, vals, kind='ilu0', vectorised=False):
        self.indptr, self.indices, self.vals, self.kind = indptr, indices, vals, kind
        self.vectorised = vectorised
        self.lev = (levels(indptr, indices, True), levels(indptr, indices, False)) if vectorised else None
        n = len(indptr) - 1
        self.shape = (n, n)
        self.symmetric = kind == 'ic0'
        self.calls = 0

    def __mul__(self, r):
        self.calls += 1
        if self.vectorised:
            return apply(self.indptr, self.indices, self.vals, r, self.kind, self.lev)
        return apply_rows(self.indptr, self.indices, self.vals, r, self.kind)
