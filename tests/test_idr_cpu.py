"""IDR(s) without a device: the NumPy restatement of the device loop (tests/_idr_ref.py), which takes all s dots of a step in
one batch, converges like the sequential biorthogonalisation of the paper and in fewer products than GMRES(30) where the
restarts hurt; it never exceeds its budget, handles the small cases and reports a zero pivot; the constants and the new
entry point are in the header, the ctypes table and the library; the host-side checks of `pykrylov_amd.IDR` run before any
device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import csr_ref
from tests import _gmres_ref as gref
from tests import _idr_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(GOLDEN))

_MAT = {}


def matrix(name):
    if name not in _MAT:
        if name == "jpwh_991":
            _MAT[name] = csr_ref.read_matrix_market(os.path.join(GOLDEN, "jpwh_991.mtx"))
        elif name == "random_diagdom_1e4":
            _MAT[name] = csr_ref.random_diagdom(10 ** 4)
        elif name == "poisson2d_12":
            _MAT[name] = csr_ref.poisson2d(12)
        elif name == "poisson2d_100":
            _MAT[name] = csr_ref.poisson2d(100)
        else:
            raise KeyError(name)
    return _MAT[name]


def rhs_of(A):
    return A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))


def unit_rhs_with_an_exact_step(n, factor, seed=1):
    """e_j for the first j at which the first IDR step on `factor` * I is exact.  With r = e_j both dots of the step have
    one term, f = p_j and M_00 = fl(factor p_j), so beta = fl(p_j / fl(factor p_j)), and r - beta (factor r) is exactly zero
    iff fl(beta factor) == 1: a property of the hashed p_j alone, evaluated here in plain arithmetic."""
    p = ref.shadow_rows(1, n, seed)[0]
    for j in range(n):
        if (p[j] / (factor * p[j])) * factor == 1.0:
            return np.eye(n)[j]
    raise AssertionError("no entry of the first shadow vector makes the step exact")


@pytest.mark.parametrize("s", [1, 2, 4, 8, 9, 16])
@pytest.mark.parametrize("name", ["jpwh_991", "random_diagdom_1e4", "poisson2d_12"])
def test_batched_dots_converge_like_the_textbook_form(name, s):
    """The same number of products (all 18 cases agreed exactly when this was written, so no slack of one is given)."""
    A = matrix(name)
    b = rhs_of(A)
    got = ref.idr(A, b, reltol=1e-10, abstol=1e-300, s=s)
    book = ref.idr_textbook(A, b, reltol=1e-10, abstol=1e-300, s=s)
    res = [float(np.linalg.norm(b - A.matvec(r.x)) / np.linalg.norm(b)) for r in (got, book)]
    print("%s s=%d: %d products batched, %d sequential; true relative residuals %.2e, %.2e"
          % (name, s, got.nMatvec, book.nMatvec, res[0], res[1]))
    assert got.converged and book.converged and got.breakdown == 0
    assert got.nMatvec == book.nMatvec
    assert max(res) <= 1e-10
    assert got.nIter == got.nMatvec and len(got.history) == got.nMatvec + 1 and got.s == s


def test_fewer_products_than_restarted_gmres():
    A = matrix("poisson2d_100")
    b = rhs_of(A)
    got = ref.idr(A, b, reltol=1e-10, abstol=1e-300, s=4)
    gm = gref.gmres(A, b, reltol=1e-10, abstol=1e-300, restart=30, matvec_max=20 * A.shape[0])
    print("poisson2d(100): IDR(4) %d products, GMRES(30) %d" % (got.nMatvec, gm.nMatvec))
    assert got.converged and gm.converged and got.nMatvec < gm.nMatvec


@pytest.mark.parametrize("mm", [1, 3, 4, 5, 6, 9, 10, 11])
def test_matvec_max_is_never_exceeded(mm):
    """s = 4, a cycle of five products: inside a cycle, at its last inner step, at the dimension-reduction product, after it."""
    A = matrix("random_diagdom_1e4")
    got = ref.idr(A, rhs_of(A), reltol=1e-14, s=4, matvec_max=mm)
    assert got.nMatvec == mm and not got.converged and len(got.history) == mm + 1
    assert got.cycles == mm // 5 and got.nIter == mm


@pytest.mark.parametrize("s", [1, 4, 8])
def test_small_cases(s):
    """1 x 1 and 2.5 I take one product.  On 2.5 I the residual after it is exactly zero when beta comes out as fl(0.4), which
    depends on the roundings of the two dots: with b = (1, .., 5) the restatement leaves 6.8e-16 (9e-17 of ||b||), with the
    unit vector chosen by `unit_rhs_with_an_exact_step` exactly 0.  Both are run; the exact case asserts the zero."""
    A = csr_ref.from_coo(np.arange(1), np.arange(1), np.full(1, 2.0), (1, 1))
    got = ref.idr(A, np.array([3.0]), s=s)
    assert got.nMatvec == 1 and got.converged and got.x[0] == 1.5 and got.s == 1
    A = csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, 2.5), (5, 5))
    b = unit_rhs_with_an_exact_step(5, 2.5)
    got = ref.idr(A, b, s=s)
    assert got.nMatvec == 1 and got.converged and got.history[-1] == 0.0 and got.s == min(s, 5)
    assert np.array_equal(got.x, b / 2.5)
    got = ref.idr(A, np.arange(1.0, 6.0), s=s)                      # a general right-hand side: zero to rounding
    assert got.nMatvec == 1 and got.converged


def test_s_is_clamped_to_n():
    A = csr_ref.poisson1d(3)
    b = np.array([1.0, 2.0, 3.0])
    got = ref.idr(A, b, s=4)
    assert got.s == 3 and got.nMatvec == 3 and got.converged and got.cycles == 0
    assert np.allclose(A.matvec(got.x), b, rtol=0, atol=1e-13)
    got = ref.idr(A, np.zeros(3), s=4)
    assert got.nMatvec == 0 and got.converged and not got.x.any() and list(got.history) == [0.0]


def test_a_zero_pivot_is_reported():
    A = csr_ref.from_coo(np.arange(4), np.arange(4), np.ones(4), (4, 4))
    e = np.eye(4)
    guess = np.array([0.0, 0.5, -1.0, 2.0])
    got = ref.idr(A, e[0] + guess, s=1, shadow=e[1:2], guess=guess)
    assert got.breakdown == 1 and not got.converged and got.nMatvec == 2 and got.nIter == 1
    assert np.array_equal(got.x, guess) and len(got.history) == 2
    got = ref.idr(A, e[0], s=1, shadow=e[1:2])
    assert got.breakdown == 1 and not got.converged and got.nMatvec == 1 and not got.x.any()


def test_jacobi_preconditioning_keeps_the_true_residual():
    from pykrylov_amd import DiagonalOperator
    A = matrix("jpwh_991")
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    d = np.zeros(n)
    d[rows[rows == A.indices]] = A.data[rows == A.indices]
    b = rhs_of(A)
    got = ref.idr(A, b, reltol=1e-10, s=4, precon=DiagonalOperator(1.0 / d))
    assert got.converged and got.precon_calls == got.nMatvec
    # right preconditioning: r is x's residual, up to the rounding of some 70 updates (1e-12 relative is generous)
    assert np.linalg.norm(b - A.matvec(got.x)) <= 1.01 * 1e-10 * got.residNorm0


def test_constants_and_the_setter():
    from pykrylov_amd import _lib
    assert _lib.MK_IDR == 12 and _lib.MK_IDR_MAX_S == 32
    hdr = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    assert "MK_IDR = 12" in hdr and "#define MK_IDR_MAX_S 32" in hdr
    res, args = _lib.PROTOTYPES["mk_solver_set_idr"]
    assert res is ctypes.c_int and len(args) == 4 and args[2] is ctypes.c_uint64
    so = os.path.join(ROOT, "pykrylov_amd", "libmikrylov.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert any(ln.split()[-1] == "mk_solver_set_idr" and ln.split()[1] == "T" for ln in out.splitlines())
    assert ctypes.sizeof(_lib.MkParams) == _lib.MkParams.restart.offset + 8          # mk_params did not change
    assert [f[0] for f in _lib.MkParams._fields_][-2:] == ["restart", "reorth"]


def test_host_checks_come_before_the_device():
    from pykrylov_amd import IDR, LinearOperator

    class Partitioned(object):
        shape = (8, 8)
        local_size = 4

        @property
        def handle(self):
            raise AssertionError("the library was touched")

    with pytest.raises(NotImplementedError, match="row-partitioned"):
        IDR(Partitioned()).solve(np.ones(4))
    op = LinearOperator(6, 6, matvec=lambda v: 1 / 0)
    for bad in (0, 33, -3, 2.5, True, None):
        with pytest.raises(ValueError, match="s must be an integer from 1 to 32"):
            IDR(op).solve(np.ones(6), s=bad)
    with pytest.raises(ValueError, match="square"):
        IDR(LinearOperator(6, 5, matvec=lambda v: v)).solve(np.ones(5))
    for bad in (np.ones((3, 6)), np.ones((4, 5)), np.ones(6), np.ones((4, 6, 1))):
        with pytest.raises(ValueError, match="shadow has shape"):
            IDR(op).solve(np.ones(6), s=4, shadow=bad)
    with pytest.raises(TypeError, match="complex"):
        IDR(op).solve(np.ones(6), s=4, shadow=np.ones((4, 6), dtype=complex))
    s = IDR(op, abstol=1e-9, reltol=1e-7)
    assert (s.abstol, s.reltol, s.precon, s.cycles, s.breakdown, s.precon_route, s.acronym) == (1e-9, 1e-7, None, 0, 0, "none", "IDR")
