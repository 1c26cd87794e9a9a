"""CPU-only checks of the device Lanczos spectrum estimate: the entry point is declared, bound and exported; the argument
checks of `tools.lanczos` and of ``tools.chebyshev(interval='lanczos')`` run before any device is touched; the NumPy
restatement (tests/_lanczos_ref.py) brackets the spectrum of the test matrices as computed by dense (or ARPACK) eigenvalue
solvers."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import csr_ref
from tests import _cheb_ref, _lanczos_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported():
    import ctypes
    from pykrylov_amd import _lib, tools
    text = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {f for f in re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", text) if "lanczos" in f}
    assert declared == {"mk_csr_lanczos"}
    assert {f for f in _lib.PROTOTYPES if "lanczos" in f} == {"mk_csr_lanczos"}
    assert "#define MK_LANCZOS_INFO_LEN 5" in text and _lib.MK_LANCZOS_INFO_LEN == 5
    restype, argtypes = _lib.PROTOTYPES["mk_csr_lanczos"]
    assert restype is ctypes.c_int and len(argtypes) == 9 and argtypes[3] is ctypes.c_uint64
    lib = _lib.load()                                            # loading needs no GPU
    so = os.path.join(ROOT, "pykrylov_amd", "libmikrylov.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "Tt"}
    assert hasattr(lib, "mk_csr_lanczos") and "mk_csr_lanczos" in exported
    assert callable(tools.lanczos) and hasattr(tools, "LanczosResult")
    import pykrylov_amd
    assert hasattr(pykrylov_amd, "lanczos") == hasattr(pykrylov_amd, "chebyshev")    # exported where chebyshev is


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
    for call in (tools.lanczos, lambda op: tools.chebyshev(op, interval="lanczos")):
        with pytest.raises(TypeError, match="CSR"):
            call(host)                                           # not a CsrOperator
        with pytest.raises(TypeError):
            call(np.eye(4).tolist())
        with pytest.raises(ValueError, match="symmetric"):
            call(_fake_csr((4, 4), symmetric=False))
        with pytest.raises(ValueError, match="square"):
            call(_fake_csr((5, 4)))
        with pytest.raises(NotImplementedError, match="row-partitioned"):
            call(_fake_csr((4, 4), local_size=2))
    ok = _fake_csr((4, 4))
    for steps in (0, -1, 2.5, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="steps"):
            tools.lanczos(ok, steps=steps)
        with pytest.raises(ValueError, match="steps"):
            tools.chebyshev(ok, interval="lanczos", steps=steps)
    for seed in (-1, 2 ** 64, 1.5, None, False):
        with pytest.raises(ValueError, match="seed"):
            tools.lanczos(ok, seed=seed)
        with pytest.raises(ValueError, match="seed"):
            tools.chebyshev(ok, interval="lanczos", seed=seed)
    for start in (np.ones(3), np.ones((4, 1)), np.array([1.0, np.nan, 0.0, 0.0]), np.array([1.0, np.inf, 0.0, 0.0]), np.zeros(4)):
        with pytest.raises(ValueError, match="start"):
            tools.lanczos(ok, start=start)
    with pytest.raises(ValueError, match="no rows"):
        tools.lanczos(_fake_csr((0, 0)))
    for interval in ("Lanczos", "ritz", None, 3):
        with pytest.raises(ValueError, match="interval"):
            tools.chebyshev(ok, interval=interval)
    with pytest.raises(ValueError, match="both given"):
        tools.chebyshev(ok, interval="lanczos", lmin=1.0, lmax=2.0)
    # the checks of the other arguments still come first and still need no device
    with pytest.raises(ValueError, match="degree"):
        tools.chebyshev(ok, degree=0, interval="lanczos")
    with pytest.raises(ValueError, match="lmax"):
        tools.chebyshev(ok, lmax=-1.0, interval="lanczos")
    with pytest.raises(ValueError, match="ratio"):
        tools.chebyshev(ok, ratio=1.0, interval="lanczos")


# ------------------------------------------------------------------ the restatement brackets the spectrum
MATRICES = ("poisson2d_12", "poisson2d_100", "1138bus", "varcoef_20_20_5", "diagonal", "poisson3d_8", "poisson1d_3", "2.5I_5")


def matrix(name):
    if name == "poisson2d_12":
        return csr_ref.poisson2d(12)
    if name == "poisson2d_100":
        return csr_ref.poisson2d(100)
    if name == "1138bus":
        return csr_ref.read_matrix_market(os.path.join(ROOT, "tests", "golden", "1138bus.mtx"))
    if name == "varcoef_20_20_5":
        return csr_ref.poisson3d_varcoef(20, 20, 5)
    if name == "diagonal":                                       # the 300-row `diagonal` matrix of test_gpu_ilu.ref_matrix
        n = 300
        d = 1.0 + np.random.default_rng(5).random(n)
        return csr_ref.from_coo(np.arange(n), np.arange(n), d, (n, n))
    if name == "poisson3d_8":
        return csr_ref.poisson3d(8)
    if name == "poisson1d_3":
        return csr_ref.poisson1d(3)
    if name == "2.5I_5":
        return csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, 2.5), (5, 5))
    raise KeyError(name)


_SPECTRUM = {}


def extremes(name, scaled):
    """(lambda_min, lambda_max) of the matrix (scaled: of D^-1/2 A D^-1/2), computed once: numpy.linalg.eigvalsh of the dense
    matrix, scipy.sparse.linalg.eigsh for poisson2d_100 (10^4 rows)."""
    key = (name, scaled)
    if key not in _SPECTRUM:
        A = matrix(name)
        n = A.shape[0]
        data = A.data
        if scaled:
            w = 1.0 / np.sqrt(_cheb_ref.diagonal(A))
            rows = np.repeat(np.arange(n), np.diff(A.indptr))
            data = w[rows] * A.data * w[A.indices]
        if name == "poisson2d_100":
            import scipy.sparse as sp
            from scipy.sparse.linalg import eigsh
            M = sp.csr_matrix((data, A.indices, A.indptr), shape=A.shape)
            hi = eigsh(M, k=1, which="LA", tol=0, ncv=64, return_eigenvectors=False)[0]
            lo = eigsh(M.tocsc(), k=1, sigma=0.0, which="LM", tol=0, return_eigenvectors=False)[0]
        else:
            D = np.zeros((n, n))
            D[np.repeat(np.arange(n), np.diff(A.indptr)), A.indices] = data
            lam = np.linalg.eigvalsh(D)
            lo, hi = lam[0], lam[-1]
        _SPECTRUM[key] = (float(lo), float(hi))
    return _SPECTRUM[key]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("steps", [10, 20])
@pytest.mark.parametrize("name", MATRICES)
def test_ritz_values_lie_in_the_spectrum_and_the_bound_is_an_upper_bound(name, steps, scaled):
    """np.dot order, seed 1: every Ritz value lies inside [lambda_min (1 - 1e-12), lambda_max (1 + 1e-12)] and
    bounds[1] >= lambda_max (1 - 1e-12).  (The slack is for the exactly converged cases: on the 3-row matrix the bound comes
    out as lambda_max (1 - 1e-16).)"""
    A = matrix(name)
    lo, hi = extremes(name, scaled)
    res = ref.lanczos(A, steps=steps, scale_diag=scaled, seed=1)
    print("%s steps %d scaled %d: m = %d, ritz [%.15g, %.15g], bound %.15g, spectrum [%.15g, %.15g], bound / lmax - 1 = %.3g"
          % (name, steps, scaled, res.steps, res.ritz[0], res.ritz[-1], res.bounds[1], lo, hi, res.bounds[1] / hi - 1.0))
    assert lo > 0
    assert np.all(res.ritz >= lo * (1 - 1e-12)) and np.all(res.ritz <= hi * (1 + 1e-12))
    assert res.bounds[1] >= hi * (1 - 1e-12)
    assert res.bounds[0] == res.ritz[0] and res.bounds[1] == res.ritz[-1] + res.residuals[-1]
    assert len(res.alpha) == res.steps == len(res.beta) - 1 <= min(steps, A.shape[0])


def test_breakdown_and_clamping_of_the_restatement():
    """m comes out as 1 for 2.5 I and for the Jacobi-scaled diagonal matrix (exact breakdown: the stop test), as 3 for
    poisson1d(3) (m = min(steps, n))."""
    assert ref.lanczos(matrix("2.5I_5")).steps == 1
    assert ref.lanczos(matrix("2.5I_5"), scale_diag=True).steps == 1
    assert ref.lanczos(matrix("diagonal"), scale_diag=True).steps == 1
    assert ref.lanczos(matrix("diagonal")).steps == 10
    assert ref.lanczos(matrix("poisson1d_3"), steps=10).steps == 3
    r = ref.lanczos(matrix("2.5I_5"))
    assert r.alpha[0] == 2.5 or abs(r.alpha[0] - 2.5) <= 4 * np.finfo(float).eps * 2.5


def test_start_vector_is_the_cell_field_less_one():
    v = ref.start_vector(1000, 1)
    assert np.array_equal(v, csr_ref.cell_field(np.arange(1000), 1) - 1.0)
    assert v.min() >= -0.5 and v.max() < 0.5 and not np.array_equal(v, ref.start_vector(1000, 2))
    A = matrix("poisson2d_12")
    a = ref.lanczos(A, steps=5, start=v[:144])
    b = ref.lanczos(A, steps=5, seed=1)
    assert np.array_equal(a.alpha, b.alpha) and np.array_equal(a.beta, b.beta)
