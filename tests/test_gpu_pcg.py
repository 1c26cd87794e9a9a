"""Device PCG (pykrylov_amd.PCG, csrc/mk_pcg.hip) bit for bit against the NumPy restatement (tests/_pcg_ref.py) in the device's
summation order: standard and flexible, no preconditioner and a diagonal one, format 0 and the builder's format; equal to
`CG` without a preconditioner, fused march passes included; the grid-stride loop; every preconditioner route against the same
object called back on the host; that AMG shortens the run; a preconditioner that changes at every call; every way the run
can halt; breakdowns; a matrix-free operator; the C ABI.  Floats are compared as bit patterns throughout."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref, gpu_order
from tests import _pcg_ref as ref
from test_gpu_ilu import device_op, ref_matrix, same
from test_gpu_lanczos import _host_twin, fmt_of, set_format
from test_pcg_cpu import Changing

pytestmark = pytest.mark.gpu

_MAT, _RHS, _REF = {}, {}, {}


def matrix(name):
    if name not in _MAT:
        if name.startswith("poisson2d_"):
            _MAT[name] = csr_ref.poisson2d(int(name[10:]))
        elif name == "neg_poisson2d_12":
            A = matrix("poisson2d_12")
            _MAT[name] = csr_ref.RefCsr(A.indptr, A.indices, -A.data, A.shape)
        elif name == "2.5I_5":
            _MAT[name] = csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, 2.5), (5, 5))
        elif name == "march_const":
            _MAT[name] = csr_ref.poisson3d(128, 8, 7)
        else:
            _MAT[name] = ref_matrix(name)
    return _MAT[name]


def rhs_of(name):
    if name not in _RHS:
        A = matrix(name)
        _RHS[name] = A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))
    return _RHS[name]


def jacobi(A):
    import pykrylov_amd
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    d = np.zeros(n)
    d[rows[rows == A.indices]] = A.data[rows == A.indices]
    return pykrylov_amd.DiagonalOperator(1.0 / d)


def reference(name, op, precon=None, **kw):
    """The restatement in the summation order of `op`'s launches, once per (matrix, launch geometry, arguments); a
    preconditioner is a diagonal, keyed by its bytes."""
    geo = gpu_order.launch_geometry(op)
    key = (name, geo, None if precon is None else np.asarray(precon.diag).tobytes()) \
        + tuple(sorted((k, v if np.isscalar(v) or v is None else np.asarray(v).tobytes()) for k, v in kw.items()))
    if key not in _REF:
        A = matrix(name)
        b = kw.pop("rhs", None)
        _REF[key] = ref.pcg(A, rhs_of(name) if b is None else b, precon=precon,
                            dots=gpu_order.GpuDots(A.shape[0], ["pcg.pq"], geo), **kw)
    return _REF[key]


def solve(op, b, precon=None, reltol=1e-6, abstol=1e-8, **kw):
    from pykrylov_amd import PCG
    s = PCG(op, reltol=reltol, abstol=abstol, precon=precon)
    s.solve(b, **kw)
    return s


def check_bits(s, want, what):
    got = (s.nMatvec, s.nIter, s.converged, s.definite, s.breakdown)
    assert got == (want.nMatvec, want.nIter, want.converged, want.definite, want.breakdown), (what, got, want[2:7])
    assert same(s.residHistory, want.history), what
    assert same(s.x, want.x), what
    assert same(s.residNorm, want.residNorm) and same(s.residNorm0, want.residNorm0), what


@pytest.mark.parametrize("flexible", [False, True], ids=["standard", "flexible"])
@pytest.mark.parametrize("route", ["none", "diag"])
@pytest.mark.parametrize("name", ["poisson2d_12", "poisson2d_31", "1138bus"])
def test_bits(name, route, flexible):
    """Less than one workgroup, an odd n (the tail lane), five tiles with irregular rows; on the plain CSR kernel and in the
    builder's format."""
    A = matrix(name)
    M = jacobi(A) if route == "diag" else None
    kw = dict(reltol=1e-10, matvec_max=60, flexible=flexible)
    for fmt in (0, -1):
        op = device_op(A, True)
        if fmt >= 0:
            set_format(op, fmt)
        got = solve(op, rhs_of(name), precon=M, **kw)
        check_bits(got, reference(name, op, M, **kw), (name, route, flexible, fmt))
        assert got.precon_route == route and got.flexible == flexible and got.nIter >= 40
        if fmt == 0:
            assert fmt_of(op) == 0
        op.free()


def _cg(op, b, **kw):
    from pykrylov_amd import CG
    s = CG(op, reltol=1e-10)
    s.solve(b, **kw)
    return s


def _equal_to_cg(op, b, **kw):
    c = _cg(op, b, **kw)
    p = solve(op, b, reltol=1e-10, **kw)
    assert p.nMatvec == c.nMatvec and p.converged == c.converged and p.nMatvec > 2
    assert same(p.residHistory, c.residHistory) and same(p.x, c.x)
    assert same(p.residNorm, c.residNorm) and p.definite and p.breakdown == 0
    return p


def test_equal_to_cg_without_a_preconditioner():
    op = device_op(matrix("poisson2d_12"), True)
    p = _equal_to_cg(op, rhs_of("poisson2d_12"))
    assert p.converged
    guess = 1.0 + np.arange(op.shape[0]) / op.shape[0]
    p = _equal_to_cg(op, rhs_of("poisson2d_12"), guess=guess)
    assert p.converged and p.nMatvec == p.nIter + 1
    op.free()
    op = device_op(matrix("1138bus"), True)
    p = _equal_to_cg(op, rhs_of("1138bus"), matvec_max=50)
    assert p.nMatvec == 50 and not p.converged
    op.free()


def test_equal_to_cg_on_a_march_matrix_where_cg_runs_fused_passes():
    op = device_op(matrix("march_const"), True)
    set_format(op, 9)
    p = _equal_to_cg(op, rhs_of("march_const"), matvec_max=12)
    assert fmt_of(op) == 9 and p.nMatvec == 12
    check_bits(p, reference("march_const", op, reltol=1e-10, matvec_max=12), "format 9")
    op.free()


@pytest.mark.parametrize("route", ["none", "diag"])
def test_grid_stride_and_odd_tail(route):
    """n beyond 512 workgroups x 512 entries: every lane takes a second pair, and the odd tail."""
    name = "poisson2d_513"
    A = matrix(name)
    assert A.shape[0] > 512 * 512 and A.shape[0] % 2 == 1
    M = jacobi(A) if route == "diag" else None
    op = device_op(A, True)
    for flexible in (False, True):
        kw = dict(reltol=1e-14, matvec_max=6, flexible=flexible)
        got = solve(op, rhs_of(name), precon=M, **kw)
        check_bits(got, reference(name, op, M, **kw), (name, route, flexible))
        assert got.nMatvec == 6
    op.free()


def _precon(kind, op, A):
    import pykrylov_amd
    from pykrylov_amd import tools
    n = A.shape[0]
    if kind == "diag":
        return jacobi(A), "diag"
    if kind == "ic0":
        return tools.ic0(op), "ilu"
    if kind == "cheb":
        return tools.chebyshev(op, degree=3), "cheb"
    if kind == "fsai":
        return tools.fsai(op), "fsai"
    if kind == "amg":
        return tools.amg(op, coarse_max=32), "amg"
    if kind == "block_jacobi":
        return tools.block_jacobi(op, 4), "device"
    assert kind == "lbfgs"
    H = pykrylov_amd.InverseLBFGSOperator(n, 5, scaling=True)
    rng = np.random.default_rng(8)
    for _ in range(2):
        v = rng.standard_normal(n)
        assert H.store(v, v * (1.0 + rng.random(n)))
    return H, "lbfgs"


@pytest.mark.parametrize("kind,flexible", [(k, False) for k in ("diag", "block_jacobi", "ic0", "cheb", "fsai", "lbfgs", "amg")]
                         + [("amg", True), ("ic0", True)])
def test_preconditioner_routes(kind, flexible):
    """The device route against the same object called back on the host: counts, history and x byte-identical, one call
    per pass."""
    name = "poisson2d_24" if kind == "amg" else "poisson2d_12"
    A = matrix(name)
    b = rhs_of(name)
    op = device_op(A, True)
    M, route = _precon(kind, op, A)
    kw = dict(reltol=1e-10, matvec_max=40, flexible=flexible)
    got = solve(op, b, precon=M, **kw)
    assert got.precon_route == route and got.nIter >= 2 and got.breakdown == 0 and got.flexible == flexible
    twin, calls = _host_twin(M)
    t = solve(op, b, precon=twin, **kw)
    assert t.precon_route == "host"
    assert (t.nMatvec, t.nIter, t.converged) == (got.nMatvec, got.nIter, got.converged), (kind, t.nMatvec, got.nMatvec)
    assert same(t.residHistory, got.residHistory) and same(t.x, got.x), kind
    assert calls[0] == got.nIter
    if kind == "amg":
        assert got.converged and got.nIter < 20                  # (3 levels; 81 passes without it, 11 with it in np.dot order)
    if kind == "diag":
        want = reference(name, op, M, **kw)
        check_bits(got, want, kind)
        assert want.precon_calls == calls[0]
    else:
        M.free()
    op.free()


def test_amg_does_its_job():
    from pykrylov_amd import tools
    name = "poisson2d_100"
    A = matrix(name)
    b = A.matvec(np.ones(A.shape[0]))
    op = device_op(A, True)
    M = tools.amg(op)
    with_amg = solve(op, b, precon=M, reltol=1e-10, abstol=0.0)
    plain = solve(op, b, reltol=1e-10, abstol=0.0)
    print("poisson2d(100): PCG %d passes, with tools.amg %d" % (plain.nIter, with_amg.nIter))
    assert with_amg.converged and plain.converged and with_amg.precon_route == "amg"
    assert abs(with_amg.nIter - 16) <= 1
    assert plain.nIter > 5 * with_amg.nIter
    assert np.linalg.norm(b - A.matvec(with_amg.x)) <= 1.01e-10 * np.linalg.norm(b)
    M.free()
    op.free()


def test_a_changing_preconditioner_through_the_host_callback():
    name = "poisson2d_30"
    A = matrix(name)
    n = A.shape[0]
    b = rhs_of(name)
    op = device_op(A, True)
    dots = gpu_order.GpuDots(n, ["pcg.pq"], gpu_order.launch_geometry(op))
    want = ref.pcg(A, b, reltol=1e-10, precon=Changing(n), flexible=True, dots=dots)
    assert want.converged
    M = Changing(n)
    got = solve(op, b, precon=M, reltol=1e-10, flexible=True)
    check_bits(got, want, "flexible")
    assert got.converged and got.precon_route == "host" and M.k == got.nIter
    std = solve(op, b, precon=Changing(n), reltol=1e-10, matvec_max=2 * got.nMatvec)
    assert not std.converged and std.nMatvec == 2 * got.nMatvec
    op.free()


def test_halt_cases():
    name = "poisson2d_12"
    A = matrix(name)
    n = A.shape[0]
    op = device_op(A, True)
    M = jacobi(A)
    for precon in (None, M):
        for mm in (1, 2, 3, 7):
            want = reference(name, op, precon, reltol=1e-14, matvec_max=mm)
            assert want.nMatvec == mm and not want.converged and len(want.history) == mm + 1
            check_bits(solve(op, rhs_of(name), precon=precon, reltol=1e-14, matvec_max=mm), want, ("matvec_max", mm))
        z = solve(op, np.zeros(n), precon=precon)
        check_bits(z, reference(name, op, precon, rhs=np.zeros(n)), "rhs = 0")
        assert z.converged and z.nMatvec == 0 and z.nIter == 0 and not z.x.any() and z.residHistory == [0.0]
        # converged in the middle of a batch of passes (the first batch is 16 passes, the second 32)
        want = reference(name, op, precon, reltol=1e-10)
        assert want.converged and 16 < want.nIter < 48 and want.nIter != 32
        got = solve(op, rhs_of(name), precon=precon, reltol=1e-10)
        check_bits(got, want, "converged inside a batch")
        # a second solve on the same object: a fresh object's result, this call's history
        b2 = A.matvec(np.cos(np.arange(n)))
        got.solve(b2, matvec_max=9)
        check_bits(got, reference(name, op, precon, reltol=1e-10, matvec_max=9, rhs=b2), "second solve")
    op.free()
    op = device_op(matrix("2.5I_5"), True)
    b = np.arange(1.0, 6.0)
    g = solve(op, b, guess=b / 2.5)
    check_bits(g, reference("2.5I_5", op, rhs=b, guess=b / 2.5), "the guess is the solution")
    assert g.converged and g.nMatvec == 1 and g.nIter == 0 and same(g.x, b / 2.5)
    op.free()


def test_finish_twice_and_iterate_after_the_halt_leave_x_alone():
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    name = "1138bus"
    A = matrix(name)
    op = device_op(A, True)
    M = jacobi(A)
    want = reference(name, op, M, reltol=1e-10, matvec_max=40)
    with DeviceRun(op, _lib.MK_PCG, rhs_of(name), precon_diag=np.asarray(M.diag), abstol=1e-8, reltol=1e-10, matvec_max=40,
                   check_curvature=1, pcg=(False,)) as run:
        res = run.run()
        assert res.halted and res.nMatvec == 40
        x = run.x()
        assert same(x, want.x)
        run.finish()
        run.finish()
        assert same(run.x(), x)
        assert run.iterate(3) == 0
        run.finish()
        assert same(run.x(), x) and same(run.history(), want.history)
    op.free()


def test_breakdowns():
    import pykrylov_amd
    name = "poisson2d_12"
    A = matrix(name)
    n = A.shape[0]
    b = rhs_of(name)
    op = device_op(A, True)
    guess = 1.0 + np.arange(n) / n
    neg = pykrylov_amd.DiagonalOperator(np.full(n, -0.25))
    for g in (None, guess):
        got = solve(op, b, precon=neg, guess=g)
        check_bits(got, reference(name, op, neg, guess=g), "a negative definite preconditioner")
        assert got.breakdown == 2 and not got.converged and got.definite and got.nIter == 0
        assert same(got.x, np.zeros(n) if g is None else g)
    # the same through a general route: the host callback
    twin, calls = _host_twin(neg)
    got = solve(op, b, precon=twin)
    assert got.breakdown == 2 and got.nIter == 0 and calls[0] == 1 and not got.x.any()
    op.free()
    # -A: the curvature test
    name = "neg_poisson2d_12"
    op = device_op(matrix(name), True)
    for precon in (None, pykrylov_amd.DiagonalOperator(np.full(n, 0.25))):
        want = reference(name, op, precon, rhs=b, guess=guess)
        got = solve(op, b, precon=precon, guess=guess)
        check_bits(got, want, "-A")
        assert not got.definite and got.breakdown == 1 and got.nMatvec == 2 and got.nIter == 0 and same(got.x, guess)
        assert same(got.infiniteDescent, want.p)
        on = solve(op, b, precon=precon, guess=guess, check_curvature=False, matvec_max=20)
        check_bits(on, reference(name, op, precon, rhs=b, guess=guess, check_curvature=False, matvec_max=20), "no curvature test")
        assert on.definite and on.nIter > 1 and on.infiniteDescent is None
    op.free()
    # a matrix holding an inf: the run halts, not converged, and the library goes on working
    data = A.data.copy()
    data[10] = np.inf
    Iref = csr_ref.RefCsr(A.indptr, A.indices, data, A.shape)
    I = device_op(Iref, True)
    s = solve(I, b)
    want = ref.pcg(Iref, b)                                      # (<p, A p> is +-inf: the pass ends in breakdown 2 or 1)
    assert not s.converged and s.nMatvec == 1 and s.breakdown in (1, 2)
    assert (s.nIter, s.breakdown, s.definite) == (want.nIter, want.breakdown, want.definite)
    assert s.nIter == 0 or not np.isfinite(s.residNorm)
    I.free()
    op = device_op(A, True)
    check_bits(solve(op, b, reltol=1e-10), reference("poisson2d_12", op, reltol=1e-10), "after the inf")
    op.free()


def test_matrix_free_operator():
    from pykrylov_amd import LinearOperator
    name = "1138bus"
    A = matrix(name)
    n = A.shape[0]
    calls = [0]

    def mv(v):
        calls[0] += 1
        return A.matvec(v)
    M = jacobi(A)
    got = solve(LinearOperator(n, n, matvec=mv, symmetric=True), rhs_of(name), precon=M, reltol=1e-10, matvec_max=60)
    assert calls[0] == got.nMatvec == 60 and got.precon_route == "diag"
    op = device_op(A, True)
    set_format(op, 0)
    twin = solve(op, rhs_of(name), precon=M, reltol=1e-10, matvec_max=60)
    assert same(twin.x, got.x) and same(twin.residHistory, got.residHistory)
    op.free()


def test_errors_through_the_c_abi():
    from pykrylov_amd import _lib
    name = "poisson2d_12"
    A = matrix(name)
    op = device_op(A, True)
    lib = _lib.init()
    p = _lib.MkParams(struct_size=ctypes.sizeof(_lib.MkParams), kind=_lib.MK_PCG, abstol=1e-8, reltol=1e-6, matvec_max=10,
                      check_curvature=1)
    h = ctypes.c_void_p()
    _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(h)))
    for bad in (2, -1):
        assert lib.mk_solver_set_pcg(h, bad) == -2                                           # MK_ERR_ARG
    assert lib.mk_solver_set_pcg(h, 1) == 0 and lib.mk_solver_set_pcg(h, 0) == 0
    _lib.check(lib.mk_solver_destroy(h))
    p.kind = _lib.MK_CG
    _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(h)))
    assert lib.mk_solver_set_pcg(h, 0) == -5                                                 # MK_ERR_UNSUPPORTED
    _lib.check(lib.mk_solver_destroy(h))
    p.kind = _lib.MK_PCG
    _lib.check(lib.mk_csr_set_row_block(op.handle, 1))
    assert lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(h)) == -5
    _lib.check(lib.mk_csr_set_row_block(op.handle, 0))
    R = csr_ref.from_coo(np.arange(5), np.arange(5), np.ones(5), (6, 5))
    rect = device_op(R, False)
    assert lib.mk_solver_create(rect.handle, ctypes.byref(p), ctypes.byref(h)) == -2         # MK_ERR_ARG
    rect.free()
    # without the setter: the standard beta
    b = rhs_of(name)
    d_b = _lib.DeviceArray.from_numpy(b)
    _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(h)))
    res = _lib.MkResult()
    _lib.check(lib.mk_solver_solve(h, d_b.ptr, None, ctypes.byref(res)))
    want = reference(name, op, matvec_max=10)
    assert res.nMatvec == 10 and res.itn == 10 and res.aux[0] == 0 and res.aux[1] == 0 and res.definite == 1
    assert same(res.residNorm, want.residNorm)
    assert lib.mk_solver_set_pcg(h, 1) == -3                                                 # MK_ERR_STATE: after the set-up
    _lib.check(lib.mk_solver_destroy(h))
    d_b.free()
    op.free()
