"""GMRES(m) without a device: the NumPy restatement of the device loop (tests/_gmres_ref.py) minimises the residual over the
Krylov space, converges on the nonsymmetric test matrices with an estimate that tracks the true residual, handles the edge
cases, and gains from Jacobi preconditioning; the host-side checks of `pykrylov_amd.GMRES` run before any device is touched."""
import ctypes
import os

import numpy as np
import pytest

from oracle import csr_ref, gpu_order
from tests import _gmres_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def convdiff(m, c):
    """poisson2d(m) with +c / -c added to the east / west entry of each row."""
    A = csr_ref.poisson2d(m)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    data = A.data.copy()
    data[A.indices == rows + 1] += c
    data[A.indices == rows - 1] -= c
    return csr_ref.RefCsr(A.indptr, A.indices, data, A.shape)


_MAT = {}


def matrix(name):
    if name not in _MAT:
        if name == "jpwh_991":
            _MAT[name] = csr_ref.read_matrix_market(os.path.join(GOLDEN, "jpwh_991.mtx"))
        elif name == "random_diagdom_1e4":
            _MAT[name] = csr_ref.random_diagdom(10 ** 4)
        elif name == "convdiff_25":
            _MAT[name] = convdiff(25, 0.5)
        elif name == "convdiff_8":
            _MAT[name] = convdiff(8, 0.7)
        else:
            raise KeyError(name)
    return _MAT[name]


def true_resid(A, b, x):
    return float(np.linalg.norm(b - A.matvec(x)))


@pytest.mark.parametrize("reorth", [True, False], ids=["cgs2", "cgs1"])
def test_every_iterate_minimises_the_residual_over_the_krylov_space(reorth):
    A = matrix("convdiff_8")
    n = A.shape[0]
    D = A.to_dense()
    b = 1.0 + np.random.default_rng(4).random(n)
    K = np.zeros((n, 12))
    for j in range(1, 13):
        K[:, j - 1] = b if j == 1 else D @ K[:, j - 2]
        K[:, :j] = np.linalg.qr(K[:, :j])[0]                        # an orthonormal basis of span{b, A b, .., A^(j-1) b}
        y = np.linalg.lstsq(D @ K[:, :j], b, rcond=None)[0]
        best = float(np.linalg.norm(b - D @ (K[:, :j] @ y)))
        got = ref.gmres(A, b, reltol=0.0, abstol=0.0, matvec_max=j, restart=12, reorth=reorth, dots=gpu_order.stream_dot)
        assert got.nMatvec == j and len(got.history) == j + 1 and got.nIter == j and got.restarts == 0
        res = true_resid(A, b, got.x)
        print("j=%2d  min %.6e  |resid - min| / min %.2e  |est - resid| / resid %.2e"
              % (j, best, abs(res - best) / best, abs(got.history[-1] - res) / res))
        assert abs(res - best) <= 1e-8 * best
        assert abs(got.history[-1] - res) <= 1e-10 * res


@pytest.mark.parametrize("restart", [5, 9, 17, 30])
@pytest.mark.parametrize("name", ["jpwh_991", "random_diagdom_1e4", "convdiff_25"])
def test_convergence(name, restart):
    A = matrix(name)
    n = A.shape[0]
    b = A.matvec(1.0 + np.random.default_rng(4).random(n))
    got = ref.gmres(A, b, reltol=1e-10, restart=restart, matvec_max=20 * n)
    assert got.converged
    h = got.history
    assert np.all(h[1:] < h[:-1])
    res = true_resid(A, b, got.x)
    print("%s restart=%d: %d products, %d restarts, |est - resid| / resid %.2e"
          % (name, restart, got.nMatvec, got.restarts, abs(h[-1] - res) / res))
    assert abs(h[-1] - res) <= 1e-4 * res
    assert got.nMatvec == got.nIter + got.restarts


def test_edge_cases():
    A = csr_ref.poisson1d(3)
    got = ref.gmres(A, np.array([1.0, 2.0, 3.0]), restart=10)
    assert got.nIter == 3 and got.nMatvec == 3 and got.converged and got.restarts == 0
    assert np.allclose(A.matvec(got.x), [1.0, 2.0, 3.0], rtol=0, atol=1e-13)
    A = csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, 2.5), (5, 5))
    b = np.arange(1.0, 6.0)
    got = ref.gmres(A, b, restart=10)
    assert got.nIter == 1 and got.converged and got.history[-1] <= 1e-15 * got.history[0] and np.allclose(got.x, b / 2.5, rtol=1e-15)
    A = csr_ref.from_coo(np.arange(1), np.arange(1), np.full(1, 2.0), (1, 1))
    got = ref.gmres(A, np.array([3.0]), restart=4)
    assert got.nIter == 1 and got.converged and got.x[0] == 1.5
    got = ref.gmres(csr_ref.poisson1d(3), np.zeros(3), restart=10)
    assert got.nMatvec == 0 and got.nIter == 0 and got.converged and not got.x.any() and list(got.history) == [0.0]


def test_matvec_max_is_never_exceeded():
    A = matrix("jpwh_991")
    b = A.matvec(np.ones(A.shape[0]))
    for mm in (1, 4, 5, 6, 11, 12):                                  # inside a cycle, at a cycle end, after a restart product
        got = ref.gmres(A, b, reltol=1e-14, restart=5, matvec_max=mm)
        assert got.nMatvec == mm and not got.converged
        assert got.restarts == mm // 6 and got.nIter == mm - got.restarts


def test_jacobi_preconditioning_saves_products():
    from pykrylov_amd import DiagonalOperator
    A = matrix("jpwh_991")
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    d = np.zeros(n)
    d[rows[rows == A.indices]] = A.data[rows == A.indices]
    b = A.matvec(1.0 + np.random.default_rng(4).random(n))
    plain = ref.gmres(A, b, reltol=1e-10, restart=20, matvec_max=20 * n)
    jac = ref.gmres(A, b, reltol=1e-10, restart=20, matvec_max=20 * n, precon=DiagonalOperator(1.0 / d))
    print("jpwh_991, restart=20: %d products plain, %d with Jacobi" % (plain.nMatvec, jac.nMatvec))
    assert plain.converged and jac.converged and jac.nMatvec < plain.nMatvec
    assert jac.precon_calls - jac.nIter - jac.restarts in (0, 1) and plain.precon_calls == 0
    assert abs(jac.history[-1] - true_resid(A, b, jac.x)) <= 1e-4 * jac.history[-1]


def test_params_and_kind():
    from pykrylov_amd import _lib
    assert _lib.MK_GMRES == 11 and _lib.MK_GMRES_MAX_RESTART == 128
    names = [f[0] for f in _lib.MkParams._fields_]
    assert names[-2:] == ["restart", "reorth"]
    assert _lib.MkParams.restart.size == 4 and _lib.MkParams.reorth.size == 4
    assert _lib.MkParams.reorth.offset == _lib.MkParams.restart.offset + 4
    assert ctypes.sizeof(_lib.MkParams) == _lib.MkParams.restart.offset + 8
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mikrylov.h")).read()
    assert "MK_GMRES = 11" in hdr and "#define MK_GMRES_MAX_RESTART 128" in hdr


def test_host_checks_come_before_the_device():
    from pykrylov_amd import GMRES, LinearOperator

    class Partitioned(object):
        shape = (8, 8)
        local_size = 4

        @property
        def handle(self):
            raise AssertionError("the library was touched")

    with pytest.raises(NotImplementedError, match="row-partitioned"):
        GMRES(Partitioned()).solve(np.ones(4))
    op = LinearOperator(6, 6, matvec=lambda v: 1 / 0)
    for bad in (0, 129, -3, 2.5, True, None):
        with pytest.raises(ValueError, match="restart must be an integer from 1 to 128"):
            GMRES(op).solve(np.ones(6), restart=bad)
    with pytest.raises(ValueError, match="square"):
        GMRES(LinearOperator(6, 5, matvec=lambda v: v)).solve(np.ones(5))
    s = GMRES(op, abstol=1e-9, reltol=1e-7)
    assert (s.abstol, s.reltol, s.precon, s.restarts, s.precon_route, s.acronym) == (1e-9, 1e-7, None, 0, "none", "GMRES")
