"""Device IDR(s) (pykrylov_amd.IDR, csrc/mk_idr.hip) bit for bit against the NumPy restatement (tests/_idr_ref.py) in the
device's summation order: s with no other column, a partial group, a full group of 8, a group of one after a full one and
three groups; format 0 and the builder's format; the grid-stride loop; every way the run can halt; a guess; the small cases;
a zero pivot; another seed; every preconditioner route against the same object called back on the host; a matrix-free
operator; a march format; errors through the C ABI.  Floats are compared as bit patterns throughout."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref, gpu_order
from tests import _idr_ref as ref
from test_gpu_ilu import device_op, ref_matrix, same
from test_gpu_lanczos import _host_twin, fmt_of, set_format
from test_idr_cpu import unit_rhs_with_an_exact_step

pytestmark = pytest.mark.gpu

G = 8                                                        # columns per launch (GM_GROUP, csrc/mk_multicol.h)
BUDGETS = (1, 3, 4, 5, 6, 9, 10, 11)                         # s = 4: inside a cycle, its last inner step, the reduction product, after it
_MAT, _RHS, _REF = {}, {}, {}


def matrix(name):
    if name not in _MAT:
        if name == "poisson2d_12":
            _MAT[name] = csr_ref.poisson2d(12)
        elif name == "poisson1d_3":
            _MAT[name] = csr_ref.poisson1d(3)
        elif name == "2.5I_5":
            _MAT[name] = csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, 2.5), (5, 5))
        elif name == "I_4":
            _MAT[name] = csr_ref.from_coo(np.arange(4), np.arange(4), np.ones(4), (4, 4))
        elif name == "one_row":
            _MAT[name] = csr_ref.from_coo(np.arange(1), np.arange(1), np.full(1, 2.0), (1, 1))
        elif name == "random_diagdom_300001":
            _MAT[name] = csr_ref.random_diagdom(300001)
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


def reference(name, **kw):
    """The restatement in the device's summation order, once per (matrix, arguments)."""
    key = (name,) + tuple(sorted((k, v if np.isscalar(v) or v is None else np.asarray(v).tobytes()) for k, v in kw.items()))
    if key not in _REF:
        b = kw.pop("rhs", None)
        _REF[key] = ref.idr(matrix(name), rhs_of(name) if b is None else b, dots=gpu_order.stream_dot, **kw)
    return _REF[key]


def solve(op, b, precon=None, reltol=1e-6, abstol=1e-8, **kw):
    from pykrylov_amd import IDR
    s = IDR(op, reltol=reltol, abstol=abstol, precon=precon)
    s.solve(b, **kw)
    return s


def check_bits(s, want, what):
    got = (s.nMatvec, s.nIter, s.cycles, s.converged, s.breakdown, s.s)
    assert got == (want.nMatvec, want.nIter, want.cycles, want.converged, want.breakdown, want.s), (what, got, want[2:7], want.s)
    assert same(s.residHistory, want.history), what
    assert same(s.x, want.x), what
    assert same(s.residNorm, want.residNorm) and same(s.residNorm0, want.residNorm0), what


@pytest.mark.parametrize("s", [1, 2, G, G + 1, 2 * G + 1])
@pytest.mark.parametrize("name", ["poisson2d_12", "jpwh_991", "random_diagdom_1e4"])
def test_bits(name, s):
    """Less than one workgroup, an odd n (the tail lane), 20 workgroups; on the plain CSR kernel and in the builder's format."""
    A = matrix(name)
    n = A.shape[0]
    want = reference(name, reltol=1e-10, s=s, matvec_max=150)
    for fmt in (0, -1):
        op = device_op(A, False)
        if fmt >= 0:
            set_format(op, fmt)
        got = solve(op, rhs_of(name), reltol=1e-10, s=s, matvec_max=150)
        check_bits(got, want, (name, s, fmt))
        assert got.precon_route == "none" and got.workspace_bytes >= 8 * 3 * s * n
        if fmt == 0:
            assert fmt_of(op) == 0
        op.free()


def test_grid_stride_and_odd_tail():
    """n beyond 512 workgroups x 512 entries: every lane takes a second pair, and the odd tail."""
    name = "random_diagdom_300001"
    A = matrix(name)
    assert A.shape[0] > 512 * 512 and A.shape[0] % 2 == 1
    want = reference(name, reltol=1e-12, s=4, matvec_max=12)
    op = device_op(A, False)
    got = solve(op, rhs_of(name), reltol=1e-12, s=4, matvec_max=12)
    check_bits(got, want, name)
    assert got.nMatvec == 12 and got.cycles == 2
    op.free()


def test_halt_cases():
    name = "random_diagdom_1e4"
    op = device_op(matrix(name), False)
    # converged inside a cycle, at a product that is neither its first nor its last
    want = reference(name, reltol=1e-10, s=8)
    assert want.converged and 1 < want.nMatvec - 9 * want.cycles < 9
    check_bits(solve(op, rhs_of(name), reltol=1e-10, s=8), want, "converged inside a cycle")
    for mm in BUDGETS:
        want = reference(name, reltol=1e-14, s=4, matvec_max=mm)
        assert want.nMatvec == mm and not want.converged and len(want.history) == mm + 1
        check_bits(solve(op, rhs_of(name), reltol=1e-14, s=4, matvec_max=mm), want, ("matvec_max", mm))
    # converged at once: a zero right-hand side, and a guess that is the solution
    z = solve(op, np.zeros(op.shape[0]), s=4)
    check_bits(z, reference(name, rhs=np.zeros(op.shape[0]), s=4), "rhs = 0")
    assert z.converged and z.nMatvec == 0 and z.nIter == 0 and not z.x.any() and z.residHistory == [0.0]
    op.free()
    op = device_op(matrix("2.5I_5"), True)
    b = np.arange(1.0, 6.0)
    g = solve(op, b, guess=b / 2.5, s=4)
    check_bits(g, reference("2.5I_5", rhs=b, guess=b / 2.5, s=4), "the guess is the solution")
    assert g.converged and g.nMatvec == 1 and g.nIter == 0 and same(g.x, b / 2.5)
    op.free()


def test_finish_twice_and_iterate_after_the_halt_leave_x_alone():
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    name = "jpwh_991"
    op = device_op(matrix(name), False)
    want = reference(name, reltol=1e-10, s=G + 1, matvec_max=40)
    with DeviceRun(op, _lib.MK_IDR, rhs_of(name), abstol=1e-8, reltol=1e-10, matvec_max=40, idr=(G + 1, 1, None)) as run:
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


def test_guess_and_a_second_solve():
    name = "jpwh_991"
    A = matrix(name)
    n = A.shape[0]
    op = device_op(A, False)
    guess = 1.0 + np.arange(n) / n
    want = reference(name, reltol=1e-10, s=4, guess=guess, matvec_max=60)
    got = solve(op, rhs_of(name), reltol=1e-10, s=4, guess=guess, matvec_max=60)
    check_bits(got, want, "guess")
    assert got.nMatvec == got.nIter + 1                          # the guess's residual product is counted
    # the same object, another right-hand side and another s: a fresh object's result
    b2 = A.matvec(np.cos(np.arange(n)))
    got.solve(b2, s=2, matvec_max=30)
    check_bits(got, reference(name, reltol=1e-10, s=2, matvec_max=30, rhs=b2), "second solve")
    op.free()


@pytest.mark.parametrize("s", [1, 4, 8])
def test_small_cases(s):
    e = unit_rhs_with_an_exact_step(5, 2.5)
    for name, b, products in (("one_row", np.array([3.0]), 1), ("2.5I_5", e, 1), ("2.5I_5", np.arange(1.0, 6.0), 1)):
        op = device_op(matrix(name), True)
        want = reference(name, rhs=b, s=s)
        got = solve(op, b, s=s)
        check_bits(got, want, (name, s))
        assert got.converged and got.nMatvec == products and got.s == min(s, op.shape[0])
        if b is e:
            assert got.residNorm == 0.0 and same(got.x, e / 2.5)
        op.free()


def test_s_is_clamped_to_n():
    op = device_op(matrix("poisson1d_3"), True)
    b = np.array([1.0, 2.0, 3.0])
    got = solve(op, b, s=4)
    check_bits(got, reference("poisson1d_3", rhs=b, s=4), "poisson1d(3)")
    assert got.s == 3 and got.nMatvec == 3 and got.converged
    op.free()


def test_a_zero_pivot_through_shadow():
    op = device_op(matrix("I_4"), True)
    e = np.eye(4)
    guess = np.array([0.0, 0.5, -1.0, 2.0])
    for g in (None, guess):
        b = e[0] if g is None else e[0] + g
        want = reference("I_4", rhs=b, s=1, shadow=e[1:2], guess=g)
        got = solve(op, b, s=1, shadow=e[1:2], guess=g)
        check_bits(got, want, "breakdown")
        assert got.breakdown == 1 and not got.converged and got.nIter == 1
        assert same(got.x, np.zeros(4) if g is None else g)
    op.free()


def test_shadow_rows_and_another_seed():
    name = "jpwh_991"
    A = matrix(name)
    op = device_op(A, False)
    base = reference(name, reltol=1e-10, s=4, matvec_max=30)
    want = reference(name, reltol=1e-10, s=4, matvec_max=30, seed=12345)
    got = solve(op, rhs_of(name), reltol=1e-10, s=4, matvec_max=30, seed=12345)
    check_bits(got, want, "seed")
    assert not same(got.x, base.x)
    # the caller's rows: the hashed ones handed in give the default run's bits; n is odd, so the rows are re-pitched
    P = ref.shadow_rows(4, A.shape[0], 1)
    check_bits(solve(op, rhs_of(name), reltol=1e-10, s=4, matvec_max=30, shadow=P), base, "shadow")
    op.free()


def _precon(kind, op, A):
    import pykrylov_amd
    from pykrylov_amd import tools
    n = A.shape[0]
    if kind == "diag":
        rows = np.repeat(np.arange(n), np.diff(A.indptr))
        d = np.zeros(n)
        d[rows[rows == A.indices]] = A.data[rows == A.indices]
        return pykrylov_amd.DiagonalOperator(1.0 / d), "diag"
    if kind == "ilu0":
        return tools.ilu0(op), "ilu"
    if kind == "ic0":
        return tools.ic0(op), "ilu"
    if kind == "cheb":
        return tools.chebyshev(op, degree=3), "cheb"
    if kind == "fsai":
        return tools.fsai(op), "fsai"
    if kind == "block_jacobi":
        return tools.block_jacobi(op, 4), "device"
    assert kind == "lbfgs"
    H = pykrylov_amd.InverseLBFGSOperator(n, 5, scaling=True)
    rng = np.random.default_rng(8)
    for _ in range(2):
        v = rng.standard_normal(n)
        assert H.store(v, v * (1.0 + rng.random(n)))
    return H, "lbfgs"


@pytest.mark.parametrize("name,kind", [("jpwh_991", "diag"), ("jpwh_991", "ilu0")]
                         + [("poisson2d_12", k) for k in ("ic0", "cheb", "fsai", "block_jacobi", "lbfgs")])
def test_preconditioner_routes(name, kind):
    """The device route against the same object called back on the host: products, history and x byte-identical, one call
    per product.  s = 9: two groups, so v passes through memory between them."""
    A = matrix(name)
    b = rhs_of(name)
    op = device_op(A, name == "poisson2d_12")
    M, route = _precon(kind, op, A)
    kw = dict(reltol=1e-10, s=G + 1, matvec_max=40)
    got = solve(op, b, precon=M, **kw)
    assert got.precon_route == route and got.nMatvec >= 2
    twin, calls = _host_twin(M)
    t = solve(op, b, precon=twin, **kw)
    assert t.precon_route == "host"
    assert t.nMatvec == got.nMatvec and same(t.residHistory, got.residHistory) and same(t.x, got.x), (name, kind)
    assert calls[0] == got.nMatvec
    if kind == "diag":
        want = ref.idr(A, b, precon=M, dots=gpu_order.stream_dot, **kw)
        check_bits(got, want, (name, kind))
        assert want.precon_calls == calls[0]
    else:
        M.free()
    op.free()


def test_matrix_free_operator():
    from pykrylov_amd import LinearOperator
    name = "jpwh_991"
    A = matrix(name)
    n = A.shape[0]
    calls = [0]

    def mv(v):
        calls[0] += 1
        return A.matvec(v)
    got = solve(LinearOperator(n, n, matvec=mv), rhs_of(name), reltol=1e-10, s=G + 1, matvec_max=150)
    check_bits(got, reference(name, reltol=1e-10, s=G + 1, matvec_max=150), "matrix free")
    assert calls[0] == got.nMatvec
    op = device_op(A, False)
    twin = solve(op, rhs_of(name), reltol=1e-10, s=G + 1, matvec_max=150)
    assert same(twin.x, got.x) and same(twin.residHistory, got.residHistory)
    op.free()


def test_march_format():
    name = "march_const"
    op = device_op(matrix(name), True)
    set_format(op, 9)
    want = reference(name, reltol=1e-12, s=4, matvec_max=12)
    got = solve(op, rhs_of(name), reltol=1e-12, s=4, matvec_max=12)
    assert fmt_of(op) == 9
    check_bits(got, want, "format 9")
    assert got.nMatvec == 12 and got.cycles == 2
    op.free()


def test_errors_through_the_c_abi():
    from pykrylov_amd import _lib
    A = matrix("poisson2d_12")
    op = device_op(A, True)
    lib = _lib.init()
    p = _lib.MkParams(struct_size=ctypes.sizeof(_lib.MkParams), kind=_lib.MK_IDR, abstol=1e-8, reltol=1e-6, matvec_max=10)
    h = ctypes.c_void_p()
    _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(h)))
    for bad in (0, 33, -1):
        assert lib.mk_solver_set_idr(h, bad, 1, None) == -2                                  # MK_ERR_ARG
    assert lib.mk_solver_set_idr(h, 32, 7, None) == 0
    _lib.check(lib.mk_solver_destroy(h))
    p.kind = _lib.MK_CG
    _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(h)))
    assert lib.mk_solver_set_idr(h, 4, 1, None) == -5                                        # MK_ERR_UNSUPPORTED
    _lib.check(lib.mk_solver_destroy(h))
    p.kind = _lib.MK_IDR
    _lib.check(lib.mk_csr_set_row_block(op.handle, 1))
    assert lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(h)) == -5
    _lib.check(lib.mk_csr_set_row_block(op.handle, 0))
    # without the setter: s = 4 and seed = 1
    b = rhs_of("poisson2d_12")
    d_b = _lib.DeviceArray.from_numpy(b)
    _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(h)))
    res = _lib.MkResult()
    _lib.check(lib.mk_solver_solve(h, d_b.ptr, None, ctypes.byref(res)))
    want = reference("poisson2d_12", s=4, matvec_max=10)
    assert res.nMatvec == 10 and res.aux[0] == 4 and res.aux[1] == 2 and res.aux[3] == 0
    assert same(res.residNorm, want.residNorm)
    assert lib.mk_solver_set_idr(h, 8, 1, None) == -3                                        # MK_ERR_STATE: after the set-up
    _lib.check(lib.mk_solver_destroy(h))
    d_b.free()
    op.free()
