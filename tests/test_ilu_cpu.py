"""The CPU restatement of ILU(0) / IC(0) (tests/_ilu_ref.py) checked against dense linear algebra, and the argument checks
of `tools.ilu0` / `tools.ic0` that run before any device is touched."""
import os

import numpy as np
import pytest

from oracle import csr_ref
from tests import _ilu_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tridiag(n, seed=0):
    rng = np.random.default_rng(seed)
    lo, up = -1.0 - rng.random(n - 1), -1.0 - rng.random(n - 1)
    d = 4.0 + rng.random(n)
    rows = np.concatenate([np.arange(n), np.arange(1, n), np.arange(n - 1)])
    cols = np.concatenate([np.arange(n), np.arange(n - 1), np.arange(1, n)])
    return csr_ref.from_coo(rows, cols, np.concatenate([d, lo, up]), (n, n))


def dense_lu(D):
    n = len(D)
    L, U = np.eye(n), D.copy()
    for k in range(n):
        for i in range(k + 1, n):
            L[i, k] = U[i, k] / U[k, k]
            U[i, :] -= L[i, k] * U[k, :]
    return L, np.triu(U)


def test_ilu0_is_the_exact_lu_of_a_tridiagonal_matrix():
    A = tridiag(60)
    v = ref.ilu0(A.indptr, A.indices, A.data)
    L, U = ref.factors_dense(A.indptr, A.indices, v)
    Ld, Ud = dense_lu(A.to_dense())
    assert np.allclose(L, Ld, rtol=1e-14, atol=1e-15) and np.allclose(U, Ud, rtol=1e-14, atol=1e-15)
    x = np.random.default_rng(1).standard_normal(60)
    for fn in (ref.apply, ref.apply_rows):
        y = fn(A.indptr, A.indices, v, A.matvec(x))
        assert np.max(np.abs(y - x)) <= 1e-13 * np.max(np.abs(x))
    assert np.array_equal(ref.apply(A.indptr, A.indices, v, x), ref.apply_rows(A.indptr, A.indices, v, x))


def test_ic0_is_the_cholesky_factor_of_a_tridiagonal_matrix():
    A = csr_ref.poisson1d(50)
    v = ref.ic0(A.indptr, A.indices, A.data)
    L, U = ref.factors_dense(A.indptr, A.indices, v, 'ic0')
    assert np.allclose(L, np.linalg.cholesky(A.to_dense()), rtol=1e-14, atol=1e-15)
    assert np.array_equal(U, L.T)
    x = np.random.default_rng(2).standard_normal(50)
    y = ref.apply(A.indptr, A.indices, v, A.matvec(x), 'ic0')
    assert np.max(np.abs(y - x)) <= 1e-13 * np.max(np.abs(x))
    assert np.array_equal(y, ref.apply_rows(A.indptr, A.indices, v, A.matvec(x), 'ic0'))


def test_ilu0_reproduces_A_on_its_pattern_jpwh991():
    A = csr_ref.read_matrix_market(os.path.join(GOLDEN, "jpwh_991.mtx"))
    v = ref.ilu0(A.indptr, A.indices, A.data)
    L, U = ref.factors_dense(A.indptr, A.indices, v)
    D = A.to_dense()
    LU = L @ U
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    assert np.allclose(LU[rows, A.indices], D[rows, A.indices], rtol=0, atol=1e-12 * np.abs(D).max())
    x = np.random.default_rng(3).standard_normal(A.shape[0])
    assert np.array_equal(ref.apply(A.indptr, A.indices, v, x), ref.apply_rows(A.indptr, A.indices, v, x))


def test_ic0_matches_its_definition_on_1138bus():
    A = csr_ref.read_matrix_market(os.path.join(GOLDEN, "1138bus.mtx"))
    v = ref.ic0(A.indptr, A.indices, A.data)
    L, _ = ref.factors_dense(A.indptr, A.indices, v, 'ic0')
    D = A.to_dense()
    LLt = L @ L.T
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    assert np.allclose(LLt[rows, A.indices], D[rows, A.indices], rtol=0, atol=1e-10 * np.abs(D).max())


def test_level_counts_of_the_issue_matrices():
    from pykrylov_amd import gallery
    ip, ix, _, _ = gallery.random_diagdom_csr(10 ** 6)
    fw, bw = ref.levels(ip, ix, True), ref.levels(ip, ix, False)
    assert (len(fw), len(bw)) == (17, 18)
    assert sum(len(r) for r in fw) == 10 ** 6 and max(len(r) for r in fw + bw) == 200028
    ip, ix, _, _ = gallery.poisson2d_csr(1000)
    assert len(ref.levels(ip, ix, True)) == 1999 and len(ref.levels(ip, ix, False)) == 1999


def test_levels_order_rows_by_their_dependencies():
    A = csr_ref.read_matrix_market(os.path.join(GOLDEN, "jpwh_991.mtx"))
    for fwd in (True, False):
        lev = np.zeros(A.shape[0], dtype=np.int64)
        for k, R in enumerate(ref.levels(A.indptr, A.indices, fwd)):
            assert np.all(np.diff(R) > 0)
            lev[R] = k + 1
        order = range(A.shape[0]) if fwd else range(A.shape[0] - 1, -1, -1)
        for i in order:
            c = A.indices[A.indptr[i]:A.indptr[i + 1]]
            c = c[c < i] if fwd else c[c > i]
            assert lev[i] == 1 + (lev[c].max() if c.size else 0)


def test_reference_errors():
    A = csr_ref.from_coo(np.array([0, 1]), np.array([1, 0]), np.array([1.0, 1.0]), (2, 2))
    with pytest.raises(ValueError, match="row 0"):
        ref.ilu0(A.indptr, A.indices, A.data)
    Z = csr_ref.from_coo(np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]), np.array([0.0, 1.0, 1.0, 0.0]), (2, 2))
    with pytest.raises(ZeroDivisionError, match="row 0"):
        ref.ilu0(Z.indptr, Z.indices, Z.data)
    B = csr_ref.from_coo(np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]), np.array([1.0, 2.0, 2.0, 1.0]), (2, 2))
    with pytest.raises(ArithmeticError, match="row 1"):
        ref.ic0(B.indptr, B.indices, B.data)


class _Shape(object):
    def __init__(self, shape, symmetric=False):
        self.shape, self.symmetric = shape, symmetric


def test_tools_refuse_a_non_square_operator_before_touching_a_device(monkeypatch):
    from pykrylov_amd import _lib, tools

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "init", no_device)
    for fn in (tools.ilu0, tools.ic0):
        with pytest.raises(ValueError, match="square"):
            fn(_Shape((5, 4), symmetric=True))
    with pytest.raises(ValueError, match="symmetric"):
        tools.ic0(_Shape((4, 4), symmetric=False))
