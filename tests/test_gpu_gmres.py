"""Device GMRES(m) (pykrylov_amd.GMRES, csrc/mk_gmres.hip) bit for bit against the NumPy restatement (tests/_gmres_ref.py) in
the device's summation order: restarts that meet a full group of basis columns, a group of one and three groups; both
orthogonalisation counts; format 0 and the builder's format; the grid-stride loop; every way the run can halt; a guess; the
edge cases; every preconditioner route against the same object called back on the host; a matrix-free operator; a march
format; errors.  Floats are compared as bit patterns throughout."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref, gpu_order
from tests import _gmres_ref as ref
from test_gpu_ilu import device_op, ref_matrix, same
from test_gpu_lanczos import _host_twin, fmt_of, set_format

pytestmark = pytest.mark.gpu

G = 8                                                        # basis columns per launch (GM_GROUP, csrc/mk_gmres.hip)
_MAT, _RHS, _REF = {}, {}, {}


def matrix(name):
    if name not in _MAT:
        if name == "poisson2d_12":
            _MAT[name] = csr_ref.poisson2d(12)
        elif name == "poisson1d_3":
            _MAT[name] = csr_ref.poisson1d(3)
        elif name == "2.5I_5":
            _MAT[name] = csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, 2.5), (5, 5))
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
        _REF[key] = ref.gmres(matrix(name), rhs_of(name) if b is None else b, dots=gpu_order.stream_dot, **kw)
    return _REF[key]


def solve(op, b, precon=None, reltol=1e-6, abstol=1e-8, **kw):
    from pykrylov_amd import GMRES
    s = GMRES(op, reltol=reltol, abstol=abstol, precon=precon)
    s.solve(b, **kw)
    return s


def check_bits(s, want, what):
    assert (s.nMatvec, s.nIter, s.restarts, s.converged) == (want.nMatvec, want.nIter, want.restarts, want.converged), \
        (what, (s.nMatvec, s.nIter, s.restarts, s.converged), want[2:6])
    assert same(s.residHistory, want.history), what
    assert same(s.x, want.x), what
    assert same(s.residNorm, want.residNorm) and same(s.residNorm0, want.residNorm0), what
    assert s.last_cycle_steps == want.last_steps, what


@pytest.mark.parametrize("reorth", [True, False], ids=["cgs2", "cgs1"])
@pytest.mark.parametrize("restart", [1, G, G + 1, 2 * G + 1, 30])
@pytest.mark.parametrize("name", ["poisson2d_12", "jpwh_991", "random_diagdom_1e4"])
def test_bits(name, restart, reorth):
    """Less than one workgroup, an odd n (the tail lane), 20 workgroups; on the plain CSR kernel and in the builder's format."""
    A = matrix(name)
    want = reference(name, reltol=1e-10, restart=restart, reorth=reorth, matvec_max=150)
    for fmt in (0, -1):
        op = device_op(A, False)
        if fmt >= 0:
            set_format(op, fmt)
        s = solve(op, rhs_of(name), reltol=1e-10, restart=restart, reorth=reorth, matvec_max=150)
        check_bits(s, want, (name, restart, reorth, fmt))
        assert s.precon_route == "none" and s.basis_bytes >= 8 * (min(restart, A.shape[0]) + 1) * A.shape[0]
        if fmt == 0:
            assert fmt_of(op) == 0
        op.free()


def test_grid_stride_and_odd_tail():
    """n beyond 512 workgroups x 512 entries: every lane takes a second pair, and the odd tail."""
    name = "random_diagdom_300001"
    A = matrix(name)
    assert A.shape[0] > 512 * 512 and A.shape[0] % 2 == 1
    want = reference(name, reltol=1e-12, restart=10, matvec_max=14)
    op = device_op(A, False)
    s = solve(op, rhs_of(name), reltol=1e-12, restart=10, matvec_max=14)
    check_bits(s, want, name)
    assert s.nMatvec == 14 and s.restarts == 1
    op.free()


def test_halt_cases():
    name = "random_diagdom_1e4"
    A = matrix(name)
    op = device_op(A, False)
    # converged inside the second cycle, at a step that is neither its first nor its last
    want = reference(name, reltol=1e-10, restart=30)
    assert want.converged and want.restarts == 1 and 1 < want.last_steps < 30
    check_bits(solve(op, rhs_of(name), reltol=1e-10, restart=30), want, "converged inside a cycle")
    # out of products inside a cycle (8), exactly at a cycle end (5, 11), with the restart's product (6), at once (1)
    for mm in (8, 5, 11, 6, 1):
        want = reference(name, reltol=1e-14, restart=5, matvec_max=mm)
        assert want.nMatvec == mm and not want.converged
        s = solve(op, rhs_of(name), reltol=1e-14, restart=5, matvec_max=mm)
        check_bits(s, want, ("matvec_max", mm))
    op.free()


def test_finish_twice_and_iterate_after_the_halt_leave_x_alone():
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    name = "jpwh_991"
    op = device_op(matrix(name), False)
    want = reference(name, reltol=1e-10, restart=9, matvec_max=40)
    with DeviceRun(op, _lib.MK_GMRES, rhs_of(name), abstol=1e-8, reltol=1e-10, matvec_max=40, restart=9, reorth=1) as run:
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
    want = reference(name, reltol=1e-10, restart=17, guess=guess, matvec_max=60)
    s = solve(op, rhs_of(name), reltol=1e-10, restart=17, guess=guess, matvec_max=60)
    check_bits(s, want, "guess")
    assert s.nMatvec == s.nIter + s.restarts + 1                 # the guess's residual product is counted
    # rhs and guess resident in HBM
    from pykrylov_amd import _lib
    d_b, d_g = _lib.DeviceArray.from_numpy(rhs_of(name)), _lib.DeviceArray.from_numpy(guess)
    s2 = solve(op, d_b, reltol=1e-10, restart=17, guess=d_g, matvec_max=60)
    check_bits(s2, want, "device arrays")
    assert same(d_b.to_numpy(), rhs_of(name)) and same(d_g.to_numpy(), guess)
    # the same object, another right-hand side: a fresh object's result
    b2 = A.matvec(np.cos(np.arange(n)))
    s.solve(b2, restart=6, matvec_max=30)
    fresh = solve(op, b2, reltol=1e-10, restart=6, matvec_max=30)
    assert same(s.x, fresh.x) and same(s.residHistory, fresh.residHistory) and s.nMatvec == fresh.nMatvec
    check_bits(s, reference(name, reltol=1e-10, restart=6, matvec_max=30, rhs=b2), "second solve")
    d_b.free()
    d_g.free()
    op.free()


def test_edge_cases():
    for name, b, restart, steps in (("poisson1d_3", np.array([1.0, 2.0, 3.0]), 10, 3), ("2.5I_5", np.arange(1.0, 6.0), 10, 1),
                                    ("one_row", np.array([3.0]), 4, 1), ("poisson1d_3", np.zeros(3), 10, 0)):
        op = device_op(matrix(name), True)
        want = reference(name, rhs=b, restart=restart)
        s = solve(op, b, restart=restart)
        check_bits(s, want, (name, restart))
        assert s.converged and s.nIter == steps and s.nMatvec == steps and s.restarts == 0
        op.free()


def _precon(kind, op, A):
    import pykrylov_amd
    from pykrylov_amd import tools
    n = A.shape[0]
    if kind == "diag":
        rows = np.repeat(np.arange(n), np.diff(A.indptr))
        d = np.zeros(n)
        d[rows[rows == A.indices]] = A.data[rows == A.indices]
        return pykrylov_amd.DiagonalOperator(1.0 / d)
    if kind == "ilu":
        return tools.ilu0(op)
    if kind == "device":
        return tools.block_jacobi(op, 4)
    if kind == "cheb":
        return tools.chebyshev(op, degree=3)
    assert kind == "lbfgs"
    H = pykrylov_amd.InverseLBFGSOperator(n, 5, scaling=True)
    rng = np.random.default_rng(8)
    for _ in range(2):
        v = rng.standard_normal(n)
        assert H.store(v, v * (1.0 + rng.random(n)))
    return H


@pytest.mark.parametrize("name,kind", [(nm, k) for nm in ("jpwh_991", "random_diagdom_1e4") for k in ("diag", "ilu", "device", "lbfgs")]
                         + [("poisson2d_100", "cheb")])
def test_preconditioner_routes(name, kind):
    """The device route against the same object called back on the host (products, history and x byte-identical, as many calls
    as the restatement makes), and both against the restatement preconditioned by that object."""
    A = matrix(name)
    b = rhs_of(name)
    op = device_op(A, kind == "cheb")
    M = _precon(kind, op, A)
    kw = dict(reltol=1e-10, restart=G + 1, matvec_max=60)
    want = ref.gmres(A, b, precon=M, dots=gpu_order.stream_dot, **kw)
    s = solve(op, b, precon=M, **kw)
    assert s.precon_route == kind
    check_bits(s, want, (name, kind))
    twin, calls = _host_twin(M)
    t = solve(op, b, precon=twin, **kw)
    assert t.precon_route == "host"
    assert t.nMatvec == s.nMatvec and same(t.residHistory, s.residHistory) and same(t.x, s.x), (name, kind)
    assert calls[0] == want.precon_calls and want.precon_calls >= want.nIter + want.restarts
    if kind != "diag":
        M.free()
    op.free()


def test_matrix_free_operator():
    from pykrylov_amd import LinearOperator
    name = "jpwh_991"
    A = matrix(name)
    n = A.shape[0]
    want = reference(name, reltol=1e-10, restart=G + 1, reorth=True, matvec_max=150)
    calls = [0]

    def mv(v):
        calls[0] += 1
        return A.matvec(v)
    s = solve(LinearOperator(n, n, matvec=mv), rhs_of(name), reltol=1e-10, restart=G + 1, matvec_max=150)
    check_bits(s, want, "matrix free")
    assert calls[0] == s.nMatvec


def test_march_format():
    name = "march_const"
    A = matrix(name)
    op = device_op(A, True)
    set_format(op, 9)
    want = reference(name, reltol=1e-12, restart=5, matvec_max=12)
    s = solve(op, rhs_of(name), reltol=1e-12, restart=5, matvec_max=12)
    assert fmt_of(op) == 9
    check_bits(s, want, "format 9")
    assert s.nMatvec == 12 and s.restarts == 2
    op.free()


def test_errors():
    import pykrylov_amd
    from pykrylov_amd import _lib, GMRES
    A = matrix("poisson2d_12")
    n = A.shape[0]
    op = device_op(A, True)
    b = np.ones(n)
    for bad in (0, 129):
        with pytest.raises(ValueError, match="restart"):
            GMRES(op).solve(b, restart=bad)
    lib = _lib.init()
    p = _lib.MkParams(struct_size=ctypes.sizeof(_lib.MkParams), kind=_lib.MK_GMRES, abstol=1e-8, reltol=1e-6, matvec_max=10,
                      reorth=1)
    h = ctypes.c_void_p()
    for bad in (0, 129, -1):
        p.restart = bad
        assert lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(h)) == -2       # MK_ERR_ARG
    # a rectangular operator: Python and the C call
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    keep = rows < n - 3
    Rm = csr_ref.from_coo(rows[keep], A.indices[keep], A.data[keep], (n - 3, n))
    rect = pykrylov_amd.CsrOperator(Rm.indptr, Rm.indices, Rm.data, Rm.shape)
    with pytest.raises(ValueError, match="square"):
        GMRES(rect).solve(np.ones(n - 3))
    p.restart = 5
    assert lib.mk_solver_create(rect.handle, ctypes.byref(p), ctypes.byref(h)) == -2
    # a preconditioner of the wrong size
    with pytest.raises(ValueError, match="shape"):
        GMRES(op, precon=pykrylov_amd.DiagonalOperator(np.ones(n - 1))).solve(b)
    with pytest.raises(ValueError, match="shape"):
        GMRES(op, precon=pykrylov_amd.InverseLBFGSOperator(n - 1)).solve(b)
    # a partitioned handle: the C call refuses, the class raises before it creates anything
    _lib.check(lib.mk_csr_set_row_block(op.handle, 1))
    assert lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(h)) == -5           # MK_ERR_UNSUPPORTED
    _lib.check(lib.mk_csr_set_row_block(op.handle, 0))
    op.local_size = n // 2
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        GMRES(op).solve(b)
    del op.local_size
    # a matrix holding an inf: the run halts, not converged, and the library goes on working
    data = A.data.copy()
    data[10] = np.inf
    I = device_op(csr_ref.RefCsr(A.indptr, A.indices, data, A.shape), True)
    s = GMRES(I)
    s.solve(b, restart=5)
    assert not s.converged and s.nMatvec == 1 and s.nIter == 1 and not np.isfinite(s.residNorm)
    good = solve(op, rhs_of("poisson2d_12"), reltol=1e-10, restart=30, matvec_max=150)
    check_bits(good, reference("poisson2d_12", reltol=1e-10, restart=30, reorth=True, matvec_max=150), "after the inf")
    for o in (op, rect, I):
        o.free()
