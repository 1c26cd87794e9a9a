"""CPU-only checks of the Chebyshev polynomial preconditioner: the entry points are declared, bound and exported; the
argument checks of `tools.chebyshev` run before any device is touched; the NumPy restatement (tests/_cheb_ref.py) equals the
explicitly evaluated polynomial, and its residual polynomial obeys the Chebyshev bound."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import csr_ref
from tests import _cheb_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ("mk_cheb_create", "mk_cheb_destroy", "mk_cheb_apply", "mk_cheb_info", "mk_cheb_coefficients",
                "mk_solver_set_precon_cheb", "mk_solver_set_lls_precon_cheb")


def test_entry_points_are_declared_bound_and_exported():
    from pykrylov_amd import _lib
    text = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {f for f in re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", text) if "cheb" in f}
    assert declared == set(ENTRY_POINTS)
    assert {f for f in _lib.PROTOTYPES if "cheb" in f} == set(ENTRY_POINTS)
    assert not any("lbfgs" in f for f in ENTRY_POINTS)
    assert "#define MK_CHEB_MAX_DEGREE 64" in text and "#define MK_CHEB_INFO_LEN 8" in text
    assert (_lib.MK_CHEB_MAX_DEGREE, _lib.MK_CHEB_INFO_LEN, ref.MAX_DEGREE) == (64, 8, 64)
    lib = _lib.load()                                            # loading needs no GPU
    so = os.path.join(ROOT, "pykrylov_amd", "libmikrylov.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "Tt"}
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in exported, name


def _fake_csr(shape, symmetric=True, local_size=None):
    """A CsrOperator shell without a device behind it: what the argument checks look at."""
    from pykrylov_amd.linop import CsrOperator
    op = object.__new__(CsrOperator)
    op.__dict__.update(_shape=shape, _symmetric=symmetric, _nargout=shape[0], _nargin=shape[1])
    if local_size is not None:
        op.local_size = local_size
    return op


def test_argument_errors_are_raised_without_a_device(monkeypatch):
    from pykrylov_amd import LinearOperator, _lib, tools

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "init", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    host = LinearOperator(4, 4, matvec=lambda v: v, symmetric=True)
    with pytest.raises(TypeError, match="CSR"):
        tools.chebyshev(host)                                    # not a CsrOperator
    with pytest.raises(TypeError):
        tools.chebyshev(np.eye(4).tolist())
    with pytest.raises(ValueError, match="symmetric"):
        tools.chebyshev(_fake_csr((4, 4), symmetric=False))
    with pytest.raises(ValueError, match="square"):
        tools.chebyshev(_fake_csr((5, 4)))
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        tools.chebyshev(_fake_csr((4, 4), local_size=2))
    ok = _fake_csr((4, 4))
    for degree in (0, 65, 2.5, -1, True, None):
        with pytest.raises(ValueError, match="degree"):
            tools.chebyshev(ok, degree=degree)
    for lmin, lmax in ((2.0, 2.0), (3.0, 2.0)):                  # lmin >= lmax
        with pytest.raises(ValueError, match="lmin < lmax"):
            tools.chebyshev(ok, lmin=lmin, lmax=lmax)
    for lmin in (0.0, -1.0, float("nan"), float("inf")):         # lmin <= 0, not finite
        with pytest.raises(ValueError, match="lmin"):
            tools.chebyshev(ok, lmin=lmin, lmax=2.0)
        with pytest.raises(ValueError, match="lmin"):
            tools.chebyshev(ok, lmin=lmin)
    for lmax in (0.0, -2.0, float("inf")):
        with pytest.raises(ValueError, match="lmax"):
            tools.chebyshev(ok, lmax=lmax)
    for ratio in (1.0, 0.5, float("nan")):
        with pytest.raises(ValueError, match="ratio"):
            tools.chebyshev(ok, ratio=ratio)


def test_the_class_is_exported_like_the_factorizations():
    import pykrylov_amd
    from pykrylov_amd import tools
    assert issubclass(tools.ChebyshevPreconditioner, pykrylov_amd.LinearOperator)
    assert hasattr(pykrylov_amd, "ChebyshevPreconditioner") == hasattr(pykrylov_amd, "IluPreconditioner")


def _dense_spd(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.concatenate([[lo, hi], lo + (hi - lo) * rng.random(n - 2)])
    return (Q * lam) @ Q.T, lam


def _p_closed_form(lam, degree, lmin, lmax):
    """p_k(t) = (1 - T_{k+1}(sigma - t / delta) / T_{k+1}(sigma)) / t: k steps after the initial direction leave the
    residual polynomial of degree k + 1 (Saad, section 12.3), evaluated here by the recurrence of T alone."""
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    return (1.0 - _cheb_T(degree + 1, (theta - lam) / delta) / _cheb_T(degree + 1, theta / delta)) / lam


@pytest.mark.parametrize("degree", [1, 2, 5, 8])
def test_reference_apply_is_the_polynomial_of_the_matrix(degree):
    """On a dense SPD matrix with known extreme eigenvalues given as the interval, the iteration equals p_k(A) r with p_k
    evaluated explicitly on the spectrum (A = Q diag(lam) Q') to 1e-12 relative."""
    n, lo, hi = 40, 0.5, 7.0
    D, lam = _dense_spd(n, lo, hi, seed=degree)
    lam, Q = np.linalg.eigh(D)
    r = np.random.default_rng(100 + degree).standard_normal(n)
    A = csr_ref.from_coo(np.repeat(np.arange(n), n), np.tile(np.arange(n), n), D.reshape(-1), (n, n))
    got = ref.apply(A, r, degree, lo, hi)
    want = Q @ (_p_closed_form(lam, degree, lo, hi) * (Q.T @ r))
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
    # ... and it approximates A^-1 r as the bound below promises: ||r - A z|| <= max|1 - t p_k(t)| ||r||
    bound = 1.0 / _cheb_T(degree + 1, (hi + lo) / (hi - lo))
    assert np.linalg.norm(r - D @ got) <= bound * (1 + 1e-10) * np.linalg.norm(r)
    # Jacobi scaling: the same iteration for D^-1 A z = D^-1 r; D^-1 A = D^-1/2 (Q diag(mu) Q') D^1/2
    w = 1.0 / np.sqrt(np.diag(D))
    mu, Q = np.linalg.eigh(D * w[:, None] * w[None, :])
    z = ref.apply(A, r, degree, mu[0], mu[-1], scale_diag=True)
    want = w * (Q @ (_p_closed_form(mu, degree, mu[0], mu[-1]) * (Q.T @ (w * r))))
    assert np.linalg.norm(z - want) <= 1e-12 * np.linalg.norm(want)


def _cheb_T(k, x):
    """Chebyshev polynomial of the first kind by its recurrence T_{j+1} = 2 x T_j - T_{j-1}."""
    a, b = 1.0, x
    if k == 0:
        return a
    for _ in range(k - 1):
        a, b = b, 2.0 * x * b - a
    return b


@pytest.mark.parametrize("k", range(1, 9))
def test_residual_polynomial_obeys_the_chebyshev_bound_on_the_diagonal_matrix(k):
    """The `diagonal` matrix of tests/test_gpu_ilu.py (entries in [1, 2]) with lmin = 1, lmax = 2: sigma = 3, and k steps
    after the initial direction give the residual polynomial T_{k+1}(3 - 2t) / T_{k+1}(3) of degree k + 1.  Hence
    max_i |1 - lambda_i p_k(lambda_i)| <= 1 / T_{k+1}(3), which is below the 1 / T_k(3) this test is asked to hold --
    both are asserted.  The bounds are derived (Saad, section 12.3), not measured."""
    n = 300
    lam = 1.0 + np.random.default_rng(5).random(n)
    A = csr_ref.from_coo(np.arange(n), np.arange(n), lam, (n, n))
    z = ref.apply(A, np.ones(n), k, 1.0, 2.0)                    # z_i = p_k(lambda_i)
    worst = float(np.max(np.abs(1.0 - lam * z)))
    assert worst <= (1.0 / _cheb_T(k, 3.0)) * (1 + 1e-10), (k, worst)
    assert worst <= (1.0 / _cheb_T(k + 1, 3.0)) * (1 + 1e-10), (k, worst)


def test_gershgorin_and_default_interval():
    A = csr_ref.poisson2d(12)
    assert ref.gershgorin(A) == 8.0 and ref.gershgorin(A, scale_diag=True) == 2.0
    assert ref.interval(A) == (8.0 / 30.0, 8.0) and ref.interval(A, lmax=6.0, ratio=10.0) == (6.0 / 10.0, 6.0)
    B = csr_ref.read_matrix_market(os.path.join(ROOT, "tests", "golden", "1138bus.mtx"))
    D = np.abs(B.to_dense())
    assert abs(ref.gershgorin(B) - D.sum(axis=1).max()) <= 1e-12 * D.sum(axis=1).max()
    dg = np.diag(B.to_dense())
    assert np.array_equal(ref.diagonal(B), dg)
    assert abs(ref.gershgorin(B, True) - (D.sum(axis=1) / np.abs(dg)).max()) <= 1e-12 * 2.0
