"""NumPy restatement of the device smoothed-aggregation AMG preconditioner (pykrylov_amd/csrc/mk_amg.hip), operation by
operation in the order the library documents (include/mikrylov.h, mk_amg_create): diagonal and Gershgorin bound, strength,
MIS(2) roots from hashed keys, the two aggregation passes, the smoothed prolongator, the Galerkin product as two
expand-sort-compress products, the dense coarse inverse and the V(1,1)-cycle -- so that equal inputs give equal bits.  No SciPy.
Test infrastructure only."""
import numpy as np

from oracle.csr_ref import from_coo
from tests import _cheb_ref

MAX_LEVELS = 16
MAX_COARSE = 1024
U = np.uint64


def h30(idx, seed):
    """Top 30 bits of the splitmix64 word the library's cell field is made of, for cell numbers `idx`."""
    with np.errstate(over="ignore"):
        z = (np.asarray(idx).astype(U) + U(1)) * U(0x9E3779B97F4A7C15) + U(seed)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        z = z ^ (z >> U(31))
    return z >> U(34)


def _rows_of(A):
    return np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))


def check_diagonal(A, level=0):
    d = _cheb_ref.diagonal(A)
    bad = np.flatnonzero(~(d > 0.0) | ~np.isfinite(d))
    if bad.size:
        raise ValueError("row %d of level %d has no positive diagonal entry" % (int(bad[0]), level))
    return d


def strength(A, d, theta):
    """Boolean per stored entry: j != i, v != 0 and v * v > ((theta * theta) * d_i) * d_j."""
    rows, cols, v = _rows_of(A), A.indices.astype(np.int64), A.data
    theta2 = float(theta) * float(theta)
    return (cols != rows) & (v != 0.0) & (v * v > (theta2 * d[rows]) * d[cols])


def mis2(A, strong, seed):
    """``(state, rounds)``: state 2 for the roots, 0 for the rest, after synchronous rounds of two maximum propagations."""
    n = A.shape[0]
    rows, cols = _rows_of(A)[strong], A.indices.astype(np.int64)[strong]
    idx = np.arange(n, dtype=U)
    body = (h30(idx, seed) << U(32)) | idx
    state = np.ones(n, dtype=U)
    rounds = 0
    while (state == U(1)).any():
        key = (state << U(62)) | body
        m1 = key.copy()
        np.maximum.at(m1, rows, key[cols])
        m2 = m1.copy()
        np.maximum.at(m2, rows, m1[cols])
        und = state == U(1)
        goin = und & (m2 == key)
        goout = und & ~goin & ((m2 >> U(62)) == U(2))
        state = state.copy()
        state[goin] = U(2)
        state[goout] = U(0)
        rounds += 1
    return state, rounds


def _pick(A, cand, value, todo):
    """Per row in `todo`: `value` at the candidate entry with the largest |a_ij|, the first in stored order on ties; -1 without
    candidates."""
    n = A.shape[0]
    start, length = A.indptr[:-1].astype(np.int64), np.diff(A.indptr).astype(np.int64)
    absv = np.abs(A.data)
    best = np.full(n, -1, dtype=np.int64)
    bv = np.full(n, -1.0)
    k = 0
    while True:
        live = np.flatnonzero(todo & (length > k))
        if not live.size:
            break
        pos = start[live] + k
        upd = cand[pos] & (absv[pos] > bv[live])
        best[live[upd]] = value[pos[upd]]
        bv[live[upd]] = absv[pos[upd]]
        k += 1
    return best


def aggregate(A, strong, state):
    """``(agg, nagg)`` by the two passes of the library."""
    cols = A.indices.astype(np.int64)
    root = state == U(2)
    rootnum = np.cumsum(root) - root
    agg1 = _pick(A, strong & root[cols], rootnum[cols], ~root)
    agg1[root] = rootnum[root]
    agg = _pick(A, strong & (agg1[cols] >= 0), agg1[cols], agg1 < 0)
    agg[agg1 >= 0] = agg1[agg1 >= 0]
    return agg, int(root.sum())


def prolongator(A, d, agg, nagg, omega, lmax):
    """P = T - (omega / lmax) D^-1 (A T): per row the list (agg(i), 1.0), (agg(j), (-((omega / lmax) * dinv_i)) * a_ij) ...,
    compressed by the rule of mk_csr_from_coo."""
    n = A.shape[0]
    rows, cols = _rows_of(A), A.indices.astype(np.int64)
    ow = float(omega) / float(lmax)
    c = -(ow * (1.0 / d))
    lr = np.concatenate([np.arange(n, dtype=np.int64), rows])       # (stable sort: T's entry stays ahead within a row)
    lc = np.concatenate([agg, agg[cols]])
    lv = np.concatenate([np.ones(n), c[rows] * A.data])
    return from_coo(lr, lc, lv, (n, nagg))


def product(X, Y):
    """C = X Y by expansion in row order and compression; also the number of expanded entries."""
    xr, xi, xv = _rows_of(X), X.indices.astype(np.int64), X.data
    yp = Y.indptr.astype(np.int64)
    cnt = yp[xi + 1] - yp[xi]
    total = int(cnt.sum())
    first = np.cumsum(cnt) - cnt
    pos = np.arange(total, dtype=np.int64) - np.repeat(first, cnt) + np.repeat(yp[xi], cnt)
    rows = np.repeat(xr, cnt)
    vals = np.repeat(xv, cnt) * Y.data[pos]
    return from_coo(rows, Y.indices.astype(np.int64)[pos], vals, (X.shape[0], Y.shape[1])), total


def dense_inverse(A):
    """Explicit inverse of a small SPD level through the Cholesky recurrence of the FSAI block, column by column; None when a
    pivot is not positive and finite."""
    n = A.shape[0]
    L = A.to_dense()
    with np.errstate(all="ignore"):
        for b in range(n):
            s = L[b, b]
            for k in range(b):
                s = s - L[b, k] * L[b, k]
            if not (s > 0.0) or not np.isfinite(s):
                return None
            ld = np.sqrt(s)
            L[b, b] = ld
            col = L[b + 1:, b].copy()
            for k in range(b):
                col = col - L[b + 1:, k] * L[b, k]
            L[b + 1:, b] = col / ld
        Y = np.zeros((n, n))
        E = np.eye(n)
        for a in range(n):                                          # L y = e_c for every column c at once
            s = E[a].copy()
            for k in range(a):
                s = s - L[a, k] * Y[k]
            Y[a] = s / L[a, a]
        X = np.zeros((n, n))
        for a in range(n - 1, -1, -1):                              # L' x = y
            s = Y[a].copy()
            for k in range(n - 1, a, -1):
                s = s - L[k, a] * X[k]
            X[a] = s / L[a, a]
    return X


class Hierarchy(object):
    """What `build` returns: `levels` (dicts with A, P, R, agg, lmax, rounds, nagg, expanded_ap, expanded_rap), `inverse`
    (None: the coarsest level is solved by its smoother alone), `degree`, `ratio`."""

    def __init__(self, levels, inverse, degree, ratio):
        self.levels, self.inverse, self.degree, self.ratio = levels, inverse, degree, ratio
        self.shape = levels[0]["A"].shape
        self.calls = 0

    @property
    def operator_complexity(self):
        return sum(lv["A"].nnz for lv in self.levels) / float(self.levels[0]["A"].nnz)

    @property
    def grid_complexity(self):
        return sum(lv["A"].shape[0] for lv in self.levels) / float(self.shape[0])

    def smooth(self, l, b):
        lv = self.levels[l]
        return _cheb_ref.apply(lv["A"], b, self.degree, lv["lmax"] / self.ratio, lv["lmax"], scale_diag=True)

    def cycle(self, l, b):
        lv = self.levels[l]
        if l == len(self.levels) - 1:
            if self.inverse is None:
                return self.smooth(l, b)
            s = np.zeros(len(b))
            for c in range(len(b)):
                s = s + self.inverse[:, c] * b[c]
            return s
        x = self.smooth(l, b)
        r = b - lv["A"].matvec(x)
        ec = self.cycle(l + 1, lv["R"].matvec(r))
        x = x + lv["P"].matvec(ec)
        r = b - lv["A"].matvec(x)
        return x + self.smooth(l, r)

    def __mul__(self, r):
        self.calls += 1
        return self.cycle(0, np.ascontiguousarray(r, dtype=np.float64))

    __call__ = __mul__


def build(A, theta=0.0, degree=1, ratio=4.0, omega=4.0 / 3.0, coarse_max=256, max_levels=10, seed=1):
    levels = []
    Al = A
    while True:
        l = len(levels)
        n = Al.shape[0]
        d = check_diagonal(Al, l)
        lmax = _cheb_ref.gershgorin(Al, scale_diag=True)
        lv = {"A": Al, "P": None, "R": None, "agg": None, "lmax": lmax, "rounds": 0, "nagg": 0, "state": None,
              "strong": None, "expanded_ap": 0, "expanded_rap": 0}
        levels.append(lv)
        last = n <= coarse_max or l + 1 >= max_levels
        if not last:
            strong = strength(Al, d, theta)
            state, rounds = mis2(Al, strong, seed)
            agg, nagg = aggregate(Al, strong, state)
            lv.update(rounds=rounds, nagg=nagg, state=state, strong=strong)
            last = nagg >= n
        if last:
            break
        P = prolongator(Al, d, agg, nagg, omega, lmax)
        R = P.transpose()
        AP, e1 = product(Al, P)
        Al, e2 = product(R, AP)
        lv.update(P=P, R=R, agg=agg, expanded_ap=e1, expanded_rap=e2)
    inverse = dense_inverse(levels[-1]["A"]) if levels[-1]["A"].shape[0] <= coarse_max else None
    return Hierarchy(levels, inverse, degree, ratio)


def pcg(A, b, M=None, rtol=1e-10, maxit=5000):
    """Textbook preconditioned CG from x = 0 to ||r|| <= rtol ||b||; returns ``(x, iterations)``."""
    x = np.zeros_like(b)
    r = b.copy()
    z = r if M is None else M * r
    p = z.copy()
    rz = float(r @ z)
    stop = rtol * float(np.linalg.norm(b))
    it = 0
    while float(np.linalg.norm(r)) > stop and it < maxit:
        Ap = A.matvec(p)
        alpha = rz / float(p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        z = r if M is None else M * r
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
    return x, it
