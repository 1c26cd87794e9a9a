"""Device LOBPCG (pykrylov_amd.LOBPCG, csrc/mk_lobpcg.hip) bit for bit against the NumPy restatement (tests/_lobpcg_ref.py) in
the device's summation order.  The Gram kernel alone, through the probe hook of the solver kind, against
``gpu_order.stream_dot`` entry by entry: one row, two, the odd tail, one full workgroup's pairs, more than one grid stride;
column counts that do not fill a tile, in both tile shapes and composed of multi-dot launches.  The loop: an odd n on both ends
of the spectrum, the preconditioner routes, irregular rows, two storage formats, soft locking, a matrix-free operator, start
blocks from the host and from the device, the refusals of the C ABI.  Floats are compared as bit patterns throughout."""
import ctypes
import os

import numpy as np
import pytest

from oracle import csr_ref, gpu_order
from tests import _lobpcg_ref as ref
from test_gpu_ilu import device_op, same
from test_gpu_lanczos import fmt_of, set_format

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_MAT, _GRAM = {}, {}


def matrix(name):
    if name not in _MAT:
        _MAT[name] = {"varcoef_7_5_3": lambda: csr_ref.poisson3d_varcoef(7, 5, 3),
                      "poisson2d_20": lambda: csr_ref.poisson2d(20),
                      "1138bus": lambda: csr_ref.read_matrix_market(os.path.join(GOLDEN, "1138bus.mtx"))}[name]()
    return _MAT[name]


def restate(A, nev, precon=None, **kw):
    return ref.lobpcg(A, nev, precon=precon, dots=gpu_order.stream_dot, **kw)


def solve(op, nev, precon=None, reltol=1e-10, abstol=0.0, **kw):
    from pykrylov_amd import LOBPCG
    s = LOBPCG(op, reltol=reltol, abstol=abstol, precon=precon)
    res = s.solve(nev, **kw)
    s.last_active = int(res.aux[2])
    return s


def counts(r):
    return (r.nMatvec, r.nIter, r.nconv, bool(r.converged), bool(r.breakdown), r.restarts, r.block, r.sweeps)


def check_bits(s, want, what):
    assert counts(s) == counts(want), (what, counts(s), counts(want))
    assert same(s.residHistory, want.history), what
    assert same(s.w, want.w) and same(s.residNorms, want.residNorms), what
    assert np.array_equal(s.pairIters, want.pairIters), what
    assert same(s.X, want.X), what
    assert same(s.anorm, want.anorm) and same(s.threshold, want.threshold) and same(s.residNorm, want.residNorm), what


# ---------------------------------------------------------------------------------------------- the Gram kernel alone
def gram_reference(n, m):
    """U (48 x n, or 17 x n for the long one) and the entries on and above the diagonal of U U' by stream_dot, once per n."""
    if n not in _GRAM:
        cols = 17 if n > 10000 else 48
        U = np.random.default_rng(n).standard_normal((cols, n))
        G = np.zeros((cols, cols))
        for i in range(cols):
            for j in range(i, cols):
                G[i, j] = G[j, i] = gpu_order.stream_dot(U[i], U[j])
        _GRAM[n] = (U, G)
    U, G = _GRAM[n]
    return U[:m], G[:m, :m]


def gram_probe(n, U, window):
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    m = U.shape[0]
    op = device_op(csr_ref.from_coo(np.arange(n), np.arange(n), np.ones(n), (n, n)), True)
    with DeviceRun(op, _lib.MK_LOBPCG, np.ascontiguousarray(U).reshape(m * n), abstol=0.0, reltol=0.0, matvec_max=1,
                   restart=1, window=window, eig=(1, m, 0, 0, 1)) as run:
        run.setup()
        res = run.finish()
        assert res.halted and res.aux[1] == m and res.nMatvec == 0
        G = run.vector(0).reshape(m, m)
    op.free()
    return G


@pytest.mark.parametrize("window", [4, 8, 1, 0], ids=["tile4", "tile8", "composed", "auto"])
@pytest.mark.parametrize("n", [1, 2, 105, 512, 70001])
def test_gram_kernel_has_the_bits_of_the_stream_dot(n, window):
    for m in (3, 8, 9, 17, 48):
        if (n > 10000 and m > 17) or (window in (0, 1) and m not in (9, 48, 17)):
            continue
        U, want = gram_reference(n, m)
        got = gram_probe(n, U, window)
        assert same(got, want), (n, m, window, np.max(np.abs(got - want)))


# ---------------------------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("which", ["SA", "LA"])
def test_bits_on_an_odd_n(which):
    """n = 105: less than one workgroup and the tail lane; format 0 and the builder's format give the same eigenpairs."""
    A = matrix("varcoef_7_5_3")
    kw = dict(which=which, block=4)
    want = restate(A, 2, **kw)
    assert want.converged and want.nIter >= 10
    for fmt in (0, -1):
        op = device_op(A, True)
        if fmt >= 0:
            set_format(op, fmt)
        s = solve(op, 2, **kw)
        check_bits(s, want, (which, fmt))
        assert s.precon_route == "none"
        assert s.workspace_bytes >= 8 * 13 * 4 * (105 + 1 + 2)
        if fmt == 0:
            assert fmt_of(op) == 0
        op.free()


def _precon(kind, op, A):
    import pykrylov_amd
    from pykrylov_amd import tools
    if kind == "amg":
        return tools.amg(op, coarse_max=32), "amg"
    if kind == "cheb":
        return tools.chebyshev(op, degree=3), "cheb"
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    d = np.zeros(n)
    d[rows[rows == A.indices]] = A.data[rows == A.indices]
    return pykrylov_amd.DiagonalOperator(1.0 / (d + np.arange(n) / n)), "diag"


class Twin(object):
    "The same preconditioner called back on the host."

    def __init__(self, M):
        self.M, self.calls = M, 0
        self.shape = M.shape

    def __mul__(self, v):
        self.calls += 1
        return self.M * v


@pytest.mark.parametrize("kind", ["amg", "cheb", "diag"])
def test_preconditioner_routes(kind):
    A = matrix("poisson2d_20")
    op = device_op(A, True)
    M, route = _precon(kind, op, A)
    kw = dict(which="SA", block=8, matvec_max=400)
    apply = (lambda r: M.diag * r) if kind == "diag" else (lambda r: M * r)
    want = restate(A, 4, precon=apply, **kw)
    s = solve(op, 4, precon=M, **kw)
    check_bits(s, want, kind)
    assert s.precon_route == route and s.nIter >= 5
    if kind == "amg":
        assert s.converged and s.nIter < 25                      # (67 iterations without it)
        ev = np.linalg.eigvalsh(A.to_dense())
        assert np.max(np.abs(s.w - ev[:4])) <= 1e-12 * ev[-1] and abs(s.w[1] - s.w[2]) <= 1e-12 * ev[-1]   # the double pair
    twin = Twin(M)
    t = solve(op, 4, precon=twin, **kw)
    assert t.precon_route == "host" and twin.calls == t.nMatvec - t.block
    check_bits(t, want, kind + " called back on the host")
    if kind != "diag":
        M.free()
    op.free()


def test_irregular_rows_with_amg_capped():
    """1138bus: parity only, the cap stops the run."""
    from pykrylov_amd import tools
    A = matrix("1138bus")
    op = device_op(A, True)
    M = tools.amg(op)
    kw = dict(which="SA", block=8, matvec_max=200)
    want = restate(A, 4, precon=lambda r: M * r, **kw)
    s = solve(op, 4, precon=M, **kw)
    check_bits(s, want, "1138bus")
    assert not s.converged and s.nMatvec <= 200 and s.nMatvec + s.last_active > 200
    M.free()
    op.free()


def test_soft_locking_on_the_device():
    """A guard column converges before a wanted one: the run goes on with fewer active columns."""
    from pykrylov_amd import tools
    A = matrix("poisson2d_20")
    op = device_op(A, True)
    M = tools.amg(op, coarse_max=32)
    kw = dict(which="SA", block=4)
    want = restate(A, 2, precon=lambda r: M * r, **kw)
    s = solve(op, 2, precon=M, **kw)
    check_bits(s, want, "soft locking")
    assert want.converged and min(want.actives) < 4
    assert s.last_active == want.actives[-1] and s.nMatvec == 4 + sum(want.actives)
    M.free()
    op.free()


def test_matrix_free_operator():
    from pykrylov_amd import LinearOperator
    A = matrix("varcoef_7_5_3")
    n = A.shape[0]
    kw = dict(which="SA", block=4, matvec_max=60)
    want = restate(A, 2, **kw)
    calls = [0]

    def mv(v):
        calls[0] += 1
        return A.matvec(v)
    s = solve(LinearOperator(n, n, matvec=mv, symmetric=True), 2, **kw)
    check_bits(s, want, "matrix free")
    assert calls[0] == s.nMatvec and not s.converged


def test_start_blocks_and_a_second_solve():
    import pykrylov_amd
    from pykrylov_amd import _lib
    A = matrix("varcoef_7_5_3")
    n = A.shape[0]
    op = device_op(A, True)
    X0 = np.cos(np.outer(np.arange(1, 5), np.arange(n))) + np.arange(4)[:, None]
    kw = dict(which="LA", block=4, matvec_max=60)
    want = restate(A, 2, start=X0, **kw)
    s = solve(op, 2, start=X0, **kw)
    check_bits(s, want, "host start")
    d = _lib.DeviceArray.from_numpy(X0.reshape(-1))
    check_bits(solve(op, 2, start=d, **kw), want, "device start")
    assert same(d.to_numpy(), X0.reshape(-1))
    d.free()
    other = restate(A, 2, seed=5, **kw)
    assert not same(other.history, want.history)
    s.solve(2, seed=5, **kw)
    check_bits(s, other, "second solve")
    # two equal columns: the Cholesky pivot test fails at once, the run ends with finite numbers
    X0[1] = X0[0]
    b = solve(op, 2, start=X0, **kw)
    check_bits(b, restate(A, 2, start=X0, **kw), "rank-deficient start")
    assert b.breakdown and not b.converged and b.nIter == 0 and np.all(np.isfinite(b.w))
    # the wrapper
    w, X = pykrylov_amd.lobpcg(op, k=2, which="SA", tol=1e-10)
    full = restate(A, 2, which="SA")
    assert same(w, full.w) and same(X, full.X.T)
    with pytest.raises(RuntimeError, match="converged"):
        pykrylov_amd.lobpcg(op, k=2, which="SA", maxiter=20)
    op.free()


def test_refusals_and_clean_up():
    from pykrylov_amd import _lib, LOBPCG
    from pykrylov_amd.generic import DeviceRun
    A = matrix("varcoef_7_5_3")
    n = A.shape[0]
    op = device_op(A, True)
    lib = _lib.init()
    h = ctypes.c_void_p()

    def block(nev, nb, which=0, keep=0, size=None, restart=0):
        b = _lib.MkParamsEig()
        b.base.struct_size = ctypes.sizeof(_lib.MkParamsEig) if size is None else size
        b.base.kind, b.base.abstol, b.base.reltol, b.base.matvec_max, b.base.restart = _lib.MK_LOBPCG, 0.0, 1e-10, 200, restart
        b.nev, b.ncv, b.which, b.keep, b.seed = nev, nb, which, keep, 1
        return b

    def create(b):
        return lib.mk_solver_create(op.handle, ctypes.byref(b.base), ctypes.byref(h))
    for b in (block(2, 4, size=ctypes.sizeof(_lib.MkParamsEig) + 8), block(0, 4), block(5, 4), block(2, 17), block(2, 36),
              block(2, 4, keep=1), block(2, 4, which=2), block(1, 49, restart=1), block(1, 4, restart=2)):
        assert create(b) == -2                                                               # MK_ERR_ARG
    short = _lib.MkParams(struct_size=ctypes.sizeof(_lib.MkParams), kind=_lib.MK_LOBPCG, abstol=0.0, reltol=1e-10, matvec_max=200)
    assert lib.mk_solver_create(op.handle, ctypes.byref(short), ctypes.byref(h)) == -2
    sh = _lib.MkParamsShifts()
    sh.base.struct_size, sh.base.kind, sh.base.matvec_max, sh.nsigma = ctypes.sizeof(_lib.MkParamsShifts), _lib.MK_LOBPCG, 200, 1
    assert lib.mk_solver_create(op.handle, ctypes.byref(sh.base), ctypes.byref(h)) == -2
    # a good block: a guess at set-up; the preconditioner setters work; destroy
    assert create(block(2, 4)) == 0
    d = _lib.DeviceArray.from_numpy(np.ones(4 * n))
    assert lib.mk_solver_setup(h, d.ptr, d.ptr) == -2
    assert lib.mk_solver_set_precon_diag(h, d.ptr) == 0
    assert lib.mk_solver_set_precon_csr(h, op.handle) == 0
    assert lib.mk_solver_set_precon_csr(h, None) == 0
    assert lib.mk_solver_setup(h, None, None) == 0
    _lib.check(lib.mk_solver_destroy(h))
    few = block(2, 4)
    few.base.matvec_max = 3
    assert create(few) == 0
    assert lib.mk_solver_setup(h, None, None) == -2
    _lib.check(lib.mk_solver_destroy(h))
    # a partitioned handle: the C call refuses, the class raises before it creates anything
    _lib.check(lib.mk_csr_set_row_block(op.handle, 1))
    assert create(block(2, 4)) == -5                                                         # MK_ERR_UNSUPPORTED
    _lib.check(lib.mk_csr_set_row_block(op.handle, 0))
    op.local_size = n // 2
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        LOBPCG(op).solve(2)
    del op.local_size
    # finish twice, iterate after the halt, close twice
    want = restate(A, 2, which="SA", block=4)
    run = DeviceRun(op, _lib.MK_LOBPCG, None, abstol=0.0, reltol=1e-10, matvec_max=2 * n, eig=(2, 4, 0, 0, 1))
    run.setup()
    assert run.iterate(1) == 1                                   # one pass is one iteration
    res = run.finish()
    assert not res.halted and res.itn == 1 and res.aux[0] == 1 and res.aux[1] == 4 and res.nMatvec == 4 + want.actives[0]
    while not res.halted:
        run.iterate(1 << 20)
        res = run.finish()
    assert res.converged and res.nMatvec == want.nMatvec
    X = np.stack([run.vector(i) for i in range(2)])
    assert same(X, want.X) and same(run.x(), want.X[0])
    run.finish()
    assert run.iterate(3) == 0
    run.finish()
    assert same(np.stack([run.vector(i) for i in range(2)]), X) and same(run.history(), want.history)
    assert same(run.vector(2).reshape(2, 3)[:, 0], want.w)
    p, ln = ctypes.c_void_p(), ctypes.c_int64()
    assert lib.mk_solver_vector(run.handle, 3, ctypes.byref(p), ctypes.byref(ln)) == -2
    run.close()
    run.close()
    d.free()
    op.free()
    op.free()
