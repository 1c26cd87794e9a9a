"""Device Chebyshev polynomial preconditioner (pykrylov_amd.tools.chebyshev, csrc/mk_cheb.hip): set-up and applies bit for
bit against the NumPy restatement (tests/_cheb_ref.py) in every storage format met here, solves with the object on the
device bit for bit against the same solves whose preconditioner is the object called back on the host, that it
preconditions, lifetimes and errors.  Floats are compared as bit patterns throughout."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref, gpu_order, krylov_ref as kr
from tests import _cheb_ref as ref
from test_gpu_ilu import _solve, device_op, ref_matrix, same

pytestmark = pytest.mark.gpu

MATRICES = ("poisson2d_100", "1138bus", "varcoef_20_20_5", "diagonal", "poisson2d_12")
DEGREES = (1, 2, 5)


def matrix(name):
    return csr_ref.poisson2d(12) if name == "poisson2d_12" else ref_matrix(name)


def fmt_of(op):
    from pykrylov_amd import _lib
    fmt = ctypes.c_int32()
    _lib.check(_lib.init().mk_csr_format_info(op.handle, ctypes.byref(fmt), None, None, None, None))
    return fmt.value


def set_format(op, fmt):
    from pykrylov_amd import _lib
    _lib.check(_lib.init().mk_csr_set_format(op.handle, fmt))


_REF = {}


def reference(name):
    """Per matrix, computed once: the matrix, an input vector, and for (degree, scaled) the default interval and the apply."""
    if name not in _REF:
        A = matrix(name)
        x = np.random.default_rng(11).standard_normal(A.shape[0])
        want = {}
        for scaled in (False, True):
            lmin, lmax = ref.interval(A, scale_diag=scaled)
            for k in DEGREES:
                want[k, scaled] = (lmin, lmax, ref.apply(A, x, k, lmin, lmax, scaled))
        _REF[name] = (A, x, want)
    return _REF[name]


@pytest.mark.parametrize("name", MATRICES)
def test_setup_bits(name):
    """`coefficients` and the default `interval` (Gershgorin bound on the device, lmax / 30) equal the reference bit for bit,
    with and without scale_diag; so do a given lmax, a given interval and another ratio."""
    from pykrylov_amd import tools
    A, _, want = reference(name)
    op = device_op(A, True)
    for scaled in (False, True):
        for k in (1, 4, 64):
            M = tools.chebyshev(op, degree=k, scale_diag=scaled)
            lmin, lmax = want[1, scaled][:2]
            assert M.interval == (lmin, lmax) and lmin == lmax / 30.0, (name, scaled, M.interval, (lmin, lmax))
            c0, c1, c2 = M.coefficients
            r0, r1, r2 = ref.coefficients(lmin, lmax, k)
            assert c0 == r0 and same(c1, r1) and same(c2, r2) and len(c1) == len(c2) == k
            info = M.info
            assert (info["rows"], info["degree"], info["scaled"], info["launches"]) == (A.shape[0], k, int(scaled), 1 + k)
            assert info["bytes"] >= (4 if scaled else 3) * 8 * A.shape[0] and info["lmin_default"] == info["lmax_default"] == 1
            assert M.degree == k and M.symmetric and M.shape == A.shape
            M.free()
        gb = ref.gershgorin(A, scaled)
        for kw, iv in ((dict(lmax=3.0), (3.0 / 30.0, 3.0)), (dict(lmin=0.25, lmax=5.5), (0.25, 5.5)),
                       (dict(ratio=10.0), (gb / 10.0, gb)), (dict(lmin=0.125), (0.125, gb)),
                       (dict(lmax=7.0, ratio=4.0), (7.0 / 4.0, 7.0))):
            M = tools.chebyshev(op, degree=3, scale_diag=scaled, **kw)
            assert M.interval == iv, (name, kw, M.interval, iv)
            c0, c1, c2 = M.coefficients
            r0, r1, r2 = ref.coefficients(iv[0], iv[1], 3)
            assert c0 == r0 and same(c1, r1) and same(c2, r2)
            M.free()
    op.free()


@pytest.mark.parametrize("fmt", [0, -1], ids=["format0", "default_format"])
@pytest.mark.parametrize("name", MATRICES)
def test_apply_bits(name, fmt):
    """`M * x` and mk_cheb_apply (out of place: the input unchanged; in place) equal the reference byte for byte, degree 1, 2
    and 5, scaled and not, on the plain CSR kernel (format 0) and in the format the builder chooses.  (MK_SPMV_FORMAT is read
    once per process, so the format is forced per matrix, by mk_csr_set_format, which overrides it.)"""
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    A, x, want = reference(name)
    op = device_op(A, True)
    if fmt >= 0:
        set_format(op, fmt)
    d_in, d_out = _lib.DeviceArray.from_numpy(x), _lib.DeviceArray(A.shape[0])
    for (k, scaled), (lmin, lmax, z) in want.items():
        M = tools.chebyshev(op, degree=k, scale_diag=scaled)
        assert same(M * x, z), (name, fmt, k, scaled)
        d_in.upload(x)
        _lib.check(lib.mk_cheb_apply(M.handle, d_in.ptr, d_out.ptr))
        assert same(d_out.to_numpy(), z) and same(d_in.to_numpy(), x), (name, fmt, k, scaled)
        M.apply_device(d_in, d_in)
        assert same(d_in.to_numpy(), z), (name, fmt, k, scaled)
        M.free()
    if fmt == 0:
        assert fmt_of(op) == 0
    d_in.free()
    d_out.free()
    op.free()


@pytest.mark.parametrize("fmt", [9, 10, 11])
def test_apply_bits_on_the_march_formats(fmt):
    """Small 3-D Poisson matrices forced into the brick-march formats, the way tests/test_gpu_pencil.py does it: 9 and 10
    run the steps as the pipelined march kernel with res[r], out[r] prefetched (a chunk of 7 planes: one pipelined round and a
    leftover plane); 11 -- a CG solver's format -- has no kernel for this epilogue and takes the CSR gather kernel on the same
    arrays.  Same bits each time."""
    from pykrylov_amd import tools
    # (format 9 keeps a value dictionary: constant coefficients; 10 and 11 stream the values of a matrix without one)
    A = csr_ref.poisson3d(128, 8, 7) if fmt == 9 else csr_ref.poisson3d_varcoef(128, 8, 7)
    x = np.random.default_rng(3).standard_normal(A.shape[0])
    op = device_op(A, True)
    set_format(op, fmt)
    assert same(op * x, A.matvec(x)) and fmt_of(op) == fmt
    for k, scaled in ((1, False), (5, False), (4, True)):
        lmin, lmax = ref.interval(A, scale_diag=scaled)
        M = tools.chebyshev(op, degree=k, scale_diag=scaled)
        assert M.interval == (lmin, lmax)
        assert same(M * x, ref.apply(A, x, k, lmin, lmax, scaled)), (fmt, k, scaled)
        M.free()
    assert fmt_of(op) == fmt
    op.free()


def _host_twin(M):
    from pykrylov_amd import LinearOperator
    n = M.shape[0]
    calls = [0]

    def mv(v):
        calls[0] += 1
        return M * v
    return LinearOperator(n, n, matvec=mv, symmetric=True), calls


@pytest.mark.parametrize("name,scaled", [("poisson2d_100", False), ("poisson2d_100", True), ("1138bus", True)])
@pytest.mark.parametrize("solver", ["cg", "bicgstab", "cgs", "tfqmr", "minres", "symmlq"])
def test_solver_with_the_device_object_matches_the_callback_path(solver, name, scaled):
    """precon=M on the device route against the same object called back on the host: iteration counts, histories and x
    byte-identical.  The loops stop inside a batch of enqueued passes (16, 32, ... passes are enqueued between two reads of
    the status word), so the applies enqueued after the stop are part of what is compared: they must change nothing."""
    from pykrylov_amd import tools
    A = matrix(name)
    op = device_op(A, True)
    rhs = A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))
    M = tools.chebyshev(op, degree=3, scale_diag=scaled)
    host, calls = _host_twin(M)
    k0, h0, x0 = _solve(solver, op, rhs, M)
    k1, h1, x1 = _solve(solver, op, rhs, host)
    assert calls[0] > 1 and k0 > 1
    assert k0 == k1 and same(h0, h1) and same(x0, x1), (solver, name, k0, k1)
    M.free()
    op.free()


def test_solver_route_is_cheb_and_a_budget_stop_inside_a_batch_changes_nothing():
    """DeviceRun names the route; a solve stopped by its budget after 5 products (inside the first batch of 16 passes)
    leaves the vectors of the callback path, whose callback is not invoked once the loop has halted."""
    from pykrylov_amd import _lib, tools
    from pykrylov_amd.generic import DeviceRun, HostPrecon
    A = matrix("poisson2d_100")
    op = device_op(A, True)
    rhs = A.matvec(np.ones(A.shape[0]))
    M = tools.chebyshev(op, degree=2)
    host, _ = _host_twin(M)
    out = []
    for p in (M, HostPrecon(host)):
        run = DeviceRun(op, _lib.MK_BICGSTAB, rhs, None, precon_diag=p, abstol=0.0, reltol=0.0, matvec_max=5)
        assert run.precon_kind == ("cheb" if p is M else "host")
        run.run()
        vecs = [run.x()]
        for k in range(2):
            try:
                vecs.append(run.vector(k))
            except Exception:
                break
        out.append(vecs)
        run.close()
    assert len(out[0]) == len(out[1]) and all(same(a, b) for a, b in zip(out[0], out[1]))
    M.free()
    op.free()


@pytest.mark.parametrize("side", ["M", "N"])
@pytest.mark.parametrize("tag", ["small", "odd"])
@pytest.mark.parametrize("solver", ["lsqr", "lsmr"])
def test_least_squares_with_the_device_object_matches_the_callback_path(solver, tag, side):
    """The object as M (nrows(A) entries) and as N (ncols(A) entries) of LSQR / LSMR on the tall matrices of
    tests/test_gpu_lls_device_precon.py: every result of the solve byte-identical to the same object behind a plain function
    (called back on the host), and `precon_route` reads 'cheb'."""
    from pykrylov_amd import tools
    from test_gpu_lls import op_from
    from test_gpu_lls_device_precon import problem, record, through_callbacks, tridiag
    A, b = problem(tag)
    k = A.shape[0] if side == "M" else A.shape[1]
    T = op_from(tridiag(k, 1 if side == "M" else 2), symmetric=True)
    P = tools.chebyshev(T, degree=3)
    kw = {side: P}
    extra = {} if tag == "small" else {"itnlim": 25}
    dev, route, got = record(solver, A, b, kw, **extra)
    calls = {}
    host, route_h, _ = record(solver, A, b, through_callbacks(kw, calls), **extra)
    other = "N" if side == "M" else "M"
    assert route == {side: "cheb", other: "none"} and route_h == {side: "host", other: "none"}
    assert calls[side] > 1 and got["itn"] > 1
    assert dev == host, (solver, tag, side, [k for k in dev if dev[k] != host[k]])
    with pytest.raises(ValueError, match="shape"):
        record(solver, A, b, {other: P}, itnlim=2)               # the other side has another size
    P.free()
    T.free()


def test_it_preconditions_minres_on_poisson2d_100(monkeypatch):
    """MINRES on poisson2d_100, rtol = 1e-10, right-hand side of ones, degree 4, default interval: as many iterations as
    the CPU restatement of MINRES preconditioned by the reference apply, and fewer than without a preconditioner.  Counted
    on the CPU when this test was written: 38 with the preconditioner, 170 without (the same with np.dot and with the
    device's summation order) -- degree 4 with the default interval does reduce the count."""
    from pykrylov_amd import Minres, tools
    A = matrix("poisson2d_100")
    n = A.shape[0]
    rhs = np.ones(n)
    op = device_op(A, True)
    M = tools.chebyshev(op, degree=4)
    s = Minres(op)
    s.solve(rhs, precon=M, show=False, check=False, etol=0.0, rtol=1e-10)
    s0 = Minres(op)
    s0.solve(rhs, show=False, check=False, etol=0.0, rtol=1e-10)
    monkeypatch.setattr(kr, "_sq", lambda a: a * a)              # the reference's pow(x, 2) is not always x*x
    red = kr.Reductions(gpu_order.GpuDots(n, gpu_order.SPMV_SITES["minres"]))
    lmin, lmax = ref.interval(A)
    want = kr.minres(A, rhs, precon=ref.HostCheb(A, 4, lmin, lmax), check=False, etol=0.0, rtol=1e-10, red=red)
    print("MINRES poisson2d_100: itn %d with chebyshev(4), oracle %d, %d without" % (s.itn, want["itn"], s0.itn))
    assert want["itn"] == 38
    assert s.itn == want["itn"] and s.istop == want["istop"] == 1
    assert s.itn < s0.itn and s0.itn == 170
    M.free()
    op.free()


def test_lifetimes():
    """free() while a solver holds the object, then solve again: same bits; free() twice; apply after free(): ValueError;
    freeing the matrix first is deferred, as for ilu0 (the object keeps it alive)."""
    import pykrylov_amd
    from pykrylov_amd import _lib, tools
    from pykrylov_amd.generic import DeviceRun
    A, x, want = reference("poisson2d_100")
    op = device_op(A, True)
    rhs = A.matvec(np.ones(A.shape[0]))
    M = tools.chebyshev(op, degree=2, scale_diag=True)
    s_ref = pykrylov_amd.BiCGSTAB(op, precon=M, reltol=1e-10)
    s_ref.solve(rhs, matvec_max=400)
    run = DeviceRun(op, _lib.MK_BICGSTAB, rhs, None, precon_diag=M, abstol=1e-8, reltol=1e-10, matvec_max=400)
    M.free()                                                    # the solver still holds the object ...
    M.free()                                                    # (twice: nothing happens)
    with pytest.raises(ValueError, match="freed"):
        M * x
    with pytest.raises(ValueError, match="freed"):
        M.handle
    op.free()                                                   # ... and the object the matrix
    res = run.run()
    xs = run.x()
    assert res.nMatvec == s_ref.nMatvec and same(xs, s_ref.x)
    assert run.iterate(5) == 0 and same(run.x(), xs)            # halted: further passes change nothing
    run.close()
    # the matrix freed first: the object still applies
    op = device_op(A, True)
    M = tools.chebyshev(op, degree=5)
    op.free()
    assert same(M * x, want[5, False][2])
    M.free()


def test_errors():
    from pykrylov_amd import CsrOperator, _lib, tools
    N = CsrOperator(np.array([0, 1, 2]), np.array([1, 0]), np.array([1.0, 1.0]), (2, 2), symmetric=True)
    with pytest.raises(_lib.MkError, match="row 0 has no usable diagonal"):
        tools.chebyshev(N, scale_diag=True)
    M = tools.chebyshev(N, degree=1)                            # unscaled: no diagonal is needed
    assert M.interval == (1.0 / 30.0, 1.0)
    M.free()
    # a missing diagonal in row 5 and a stored zero in row 3 of a 2-D Laplacian: the smallest such row is named
    A = csr_ref.poisson2d(12)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep = ~((rows == 5) & (A.indices == 5))
    data = np.where((rows == 3) & (A.indices == 3), 0.0, A.data)
    B = csr_ref.from_coo(rows[keep], A.indices[keep], np.where(keep, data, 0.0)[keep], A.shape)
    assert B.nnz == A.nnz - 1                                   # (from_coo keeps the stored zero)
    Bop = device_op(B, True)
    with pytest.raises(_lib.MkError, match="row 3 has no usable diagonal"):
        tools.chebyshev(Bop, scale_diag=True)
    S = Bop + Bop                                               # a composite: no arrays of its own
    with pytest.raises(_lib.MkError, match="to_csr_arrays"):
        tools.chebyshev(S)
    # a row-partitioned operator (what the package recognises one by: `local_size`)
    Bop.local_size = B.shape[0] // 2
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        tools.chebyshev(Bop)
    del Bop.local_size
    lib = _lib.init()
    h = ctypes.c_void_p()
    for degree, lmin, lmax in ((0, 0.0, 0.0), (65, 0.0, 0.0), (2, 2.0, 1.0), (2, float("nan"), 1.0), (2, 1.0, float("inf"))):
        assert lib.mk_cheb_create(Bop.handle, degree, lmin, lmax, 0, ctypes.byref(h)) == -2, (degree, lmin, lmax)   # MK_ERR_ARG
    for o in (S, Bop, N):
        o.free()
