"""Preconditioners that are device operators (mk_solver_set_precon_csr): ``precon * r`` evaluated as a product on the
device at the reference's preconditioner sites (generic/generic.py:76; cg.py:91-92,137-138; bicgstab.py:96-99,120-123;
cgs.py:79-80,88-94; tfqmr.py:109-110,142-143; minres.py:249-251; symmlq.py:188-190,308-310).  The product of a device
matrix has the bits of the scalar CSR loop, so a solve with the preconditioner ON the device must agree bit for bit
with the same solve whose preconditioner is the same matrix applied on the HOST through the callback path."""
import numpy as np
import pytest

from oracle import csr_ref

pytestmark = pytest.mark.gpu


class HostMatrixPrecon(object):
    """The same preconditioner as a host object: ``precon * r`` = the oracle's CSR product.  Counts its calls."""

    def __init__(self, M):
        self.M, self.calls = M, 0

    def __mul__(self, r):
        self.calls += 1
        return self.M.matvec(r)


def problem(n_side=20, nonsym=False, seed=3):
    from pykrylov_amd import CsrOperator, tools
    rng = np.random.default_rng(seed)
    A = csr_ref.poisson3d_varcoef(n_side, n_side, 5, seed=seed)
    if nonsym:
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        skew = np.where(A.indices > rows, 1.25, 1.0)                         # upper triangle scaled: nonsymmetric
        A = csr_ref.RefCsr(A.indptr, A.indices, A.data * skew, A.shape)
    op = CsrOperator(A.indptr, A.indices, A.data, A.shape, symmetric=not nonsym)
    Mop = tools.block_jacobi(op, 4)
    Mref = csr_ref.RefCsr(*Mop.to_csr_arrays(), shape=Mop.shape)
    rhs = A.matvec(1.0 + rng.random(A.shape[0]))
    return A, op, Mop, Mref, rhs


def test_block_jacobi_is_the_inverse_of_the_diagonal_blocks():
    A, op, Mop, Mref, _ = problem(8)
    D, Mi = A.to_dense(), Mref.to_dense()
    n = A.shape[0]
    for b0 in range(0, n, 4):
        blk = D[b0:b0 + 4, b0:b0 + 4]
        assert np.allclose(Mi[b0:b0 + 4, b0:b0 + 4] @ blk, np.eye(len(blk)), atol=1e-12)
    assert Mref.nnz <= 4 * n and np.array_equal(Mi, Mi * (np.abs(np.subtract.outer(np.arange(n) // 4, np.arange(n) // 4)) == 0))
    op.free()
    Mop.free()


@pytest.mark.parametrize("solver", ["cg", "bicgstab", "cgs", "tfqmr", "minres", "symmlq"])
def test_device_preconditioner_matches_the_host_callback_path_bit_for_bit(solver):
    import pykrylov_amd
    from pykrylov_amd.generic import DevicePrecon
    nonsym = solver in ("bicgstab", "cgs", "tfqmr")
    A, op, Mop, Mref, rhs = problem(nonsym=nonsym)
    cls = dict(cg=pykrylov_amd.CG, bicgstab=pykrylov_amd.BiCGSTAB, cgs=pykrylov_amd.CGS, tfqmr=pykrylov_amd.TFQMR,
               minres=pykrylov_amd.Minres, symmlq=pykrylov_amd.Symmlq)[solver]
    host = HostMatrixPrecon(Mref)
    runs = []
    for precon in (Mop, host):
        if solver == "minres":
            s = cls(op)
            assert isinstance(s._device_precon(precon), DevicePrecon) == (precon is Mop)
            s.solve(rhs, precon=precon, show=False, check=False, etol=0.0, rtol=1e-10)
            runs.append((s.itn, s.istop, np.array(s.residHistory), s.x))
        elif solver == "symmlq":
            s = cls(op, precon=precon)
            s.solve(rhs, rtol=1e-10)
            runs.append((s.nMatvec, 0, np.array([s.residNorm]), s.x))
        else:
            s = cls(op, precon=precon, reltol=1e-10)
            assert isinstance(s._device_precon(precon), DevicePrecon) == (precon is Mop)
            s.solve(rhs, matvec_max=400)
            runs.append((s.nMatvec, int(s.converged), np.array(getattr(s, "residHistory", [s.residNorm])), s.x))
    (k0, c0, h0, x0), (k1, c1, h1, x1) = runs
    assert host.calls > 3                                                    # the host path really went through callbacks
    assert k0 == k1 and c0 == c1 and np.array_equal(h0, h1) and np.array_equal(x0, x1), solver
    if solver != "cg":                                                       # (the reference's preconditioned CG stalls,
        assert np.linalg.norm(A.matvec(x0) - rhs) <= 0.1 * np.linalg.norm(rhs)    # DESIGN.md section 7)
    op.free()
    Mop.free()


def test_block_preconditioner_of_device_matrices_and_wrong_shapes():
    """A BlockDiagonalLinearOperator of device matrices as preconditioner (device view), and shape errors."""
    import pykrylov_amd
    from pykrylov_amd import CsrOperator, tools
    from pykrylov_amd.blkop import BlockDiagonalLinearOperator
    from pykrylov_amd.generic import DevicePrecon
    A, op, Mop, Mref, rhs = problem(nonsym=True)
    n = A.shape[0]
    half = n // 2
    # two independent block-Jacobi preconditioners of the two halves of the diagonal, glued by a block operator
    ip, ix, dv = Mop.to_csr_arrays()
    r = np.repeat(np.arange(n), np.diff(ip))
    top, bot = r < half, r >= half
    M1 = CsrOperator.from_coo(r[top], ix[top], dv[top], (half, half))
    M2 = CsrOperator.from_coo(r[bot] - half, ix[bot] - half, dv[bot], (n - half, n - half))
    K = BlockDiagonalLinearOperator([M1, M2])
    s = pykrylov_amd.BiCGSTAB(op, precon=K, reltol=1e-10)
    assert isinstance(s._device_precon(K), DevicePrecon)
    s.solve(rhs)
    s2 = pykrylov_amd.BiCGSTAB(op, precon=Mop, reltol=1e-10)
    s2.solve(rhs)
    assert s.converged and s.nMatvec == s2.nMatvec and np.array_equal(s.x, s2.x)   # same matrix, same bits
    with pytest.raises(ValueError):
        pykrylov_amd.BiCGSTAB(op, precon=M1).solve(rhs)
    for o in (op, Mop, M1, M2):
        o.free()


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_every_setter_replaces_whatever_preconditioner_was_attached(solver):
    """One solver walks through the attachments of the C ABI -- device matrix, incomplete factor, L-BFGS operator, host
    callback, diagonal, NULL -- and solves after each step: history and iterate must have the bits of a fresh solver that
    was only ever given that one preconditioner (so nothing of the previous attachment acts on), and consecutive steps
    must differ (so the comparison can see a preconditioner that stayed).  Then a factor and an L-BFGS operator are
    destroyed while the solver holds them and replaced on it."""
    import ctypes
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    A, op, Mop, Mref, rhs = problem(12)                                      # SPD, n = 720
    n = A.shape[0]
    lib = _lib.init()
    rng = np.random.default_rng(11)
    kind = dict(cg=_lib.MK_CG, bicgstab=_lib.MK_BICGSTAB)[solver]

    def factor():
        h = ctypes.c_void_p()
        _lib.check((lib.mk_ic0_create if solver == "cg" else lib.mk_ilu0_create)(op.handle, ctypes.byref(h)))
        return h

    def lbfgs():                                                             # three pairs (s, A s): an SPD inverse
        h = ctypes.c_void_p()
        _lib.check(lib.mk_lbfgs_create(n, 3, 1, ctypes.byref(h)))
        for _ in range(3):
            s = rng.standard_normal(n)
            ds, dy = _lib.DeviceArray.from_numpy(s), _lib.DeviceArray.from_numpy(A.matvec(s))
            ok = ctypes.c_int32(0)
            _lib.check(lib.mk_lbfgs_store(h, ds.ptr, dy.ptr, 1e-20, ctypes.byref(ok)))
            assert ok.value == 1
            ds.free()
            dy.free()
        return h

    F, H = factor(), lbfgs()
    dinv = 1.0 / A.to_dense().diagonal()
    d_dinv = _lib.DeviceArray.from_numpy(dinv)
    calls = [0]

    def call(user, rp, yp):                                                  # a scaled Jacobi on the host
        r = np.ctypeslib.as_array(ctypes.cast(rp, ctypes.POINTER(ctypes.c_double)), shape=(n,))
        np.ctypeslib.as_array(ctypes.cast(yp, ctypes.POINTER(ctypes.c_double)), shape=(n,))[:] = 0.75 * dinv * r
        calls[0] += 1
        return 0
    cb = _lib.PRECON_FN(call)
    steps = [("device matrix", lambda h: lib.mk_solver_set_precon_csr(h, Mop.handle)),
             ("factor", lambda h: lib.mk_solver_set_precon_ilu(h, F)),
             ("lbfgs", lambda h: lib.mk_solver_set_precon_lbfgs(h, H)),
             ("callback", lambda h: lib.mk_solver_set_precon_callback(h, cb, None)),
             ("diagonal", lambda h: lib.mk_solver_set_precon_diag(h, d_dinv.ptr)),
             ("null", lambda h: lib.mk_solver_set_precon_csr(h, None))]

    def new_run():
        return DeviceRun(op, kind, rhs, abstol=0.0, reltol=1e-10, matvec_max=60)

    def solve(run):
        res = run.run()
        return int(res.nMatvec), run.history(), run.x()

    def same(a, b):
        return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])

    walker, prev, alone = new_run(), None, {}
    for name, attach in steps:
        _lib.check(attach(walker.handle))
        got = solve(walker)
        fresh = new_run()
        _lib.check(attach(fresh.handle))
        want = solve(fresh)
        fresh.close()
        assert got[0] > 3 and np.all(np.isfinite(got[2])), (solver, name)       # (BiCGSTAB keeps no history)
        assert same(got, want), (solver, name)
        assert prev is None or not same(got, prev), (solver, name)
        prev = alone[name] = got
    assert calls[0] > 3
    plain = prev

    # ... and every ordered pair a -> b of the six, the walk's order or not (device matrix -> diagonal among them), with the
    # NULL of every setter in turn
    nulls = [lambda h: lib.mk_solver_set_precon_diag(h, None),
             lambda h: lib.mk_solver_set_precon_callback(h, _lib.PRECON_FN(), None),        # (a NULL function pointer)
             lambda h: lib.mk_solver_set_precon_csr(h, None), lambda h: lib.mk_solver_set_precon_ilu(h, None),
             lambda h: lib.mk_solver_set_precon_lbfgs(h, None)]
    for k, (a, attach_a) in enumerate(steps[:5]):
        for b, attach_b in steps[:5] + [("null", nulls[k])]:
            if a != b:
                run = new_run()
                _lib.check(attach_a(run.handle))
                assert same(solve(run), alone[a]), (solver, a)
                _lib.check(attach_b(run.handle))
                assert same(solve(run), alone[b]), (solver, a, b)
                run.close()

    # destroyed while held: the solver keeps applying the object until it is replaced, which frees it
    _lib.check(lib.mk_solver_set_precon_ilu(walker.handle, F))
    _lib.check(lib.mk_solver_set_precon_ilu(walker.handle, F))               # (re-setting the attached object keeps it)
    with_f = solve(walker)
    small = ctypes.c_void_p()
    _lib.check(lib.mk_lbfgs_create(n - 1, 3, 1, ctypes.byref(small)))
    assert lib.mk_solver_set_precon_lbfgs(walker.handle, small) == -2       # MK_ERR_ARG: a setter that fails changes nothing
    _lib.check(lib.mk_lbfgs_destroy(small))
    assert same(solve(walker), with_f)
    _lib.check(lib.mk_ilu_destroy(F))
    assert same(solve(walker), with_f)
    _lib.check(lib.mk_solver_set_precon_lbfgs(walker.handle, H))             # F goes here
    with_h = solve(walker)
    _lib.check(lib.mk_lbfgs_destroy(H))
    assert same(solve(walker), with_h) and not same(with_h, with_f)
    _lib.check(lib.mk_solver_set_precon_diag(walker.handle, None))           # H goes here
    assert same(solve(walker), plain)
    F2, H2 = factor(), lbfgs()                                               # later creations work
    _lib.check(lib.mk_solver_set_precon_ilu(walker.handle, F2))
    assert same(solve(walker), with_f)
    _lib.check(lib.mk_solver_set_precon_lbfgs(walker.handle, H2))
    assert np.all(np.isfinite(solve(walker)[2]))
    walker.close()
    _lib.check(lib.mk_ilu_destroy(F2))
    _lib.check(lib.mk_lbfgs_destroy(H2))
    d_dinv.free()
    op.free()
    Mop.free()


# ------------------------------------------------------------------ the device preconditioner OBJECTS, one body for all kinds
# (kind, how `tools` makes it, the solver that takes it, the launch counters of `info` and their values per matrix:
#  launches per apply, read from the commit before the objects got their common base -- neither the kernels nor their
#  order may change)
OBJECTS = {
    "ilu0": (lambda tools, op: tools.ilu0(op), "bicgstab", ("launches_forward", "launches_backward"), {64: (1, 1), 1: (1, 1)}),
    "ic0": (lambda tools, op: tools.ic0(op), "pcg", ("launches_forward", "launches_backward"), {64: (1, 1), 1: (1, 1)}),
    "chebyshev": (lambda tools, op: tools.chebyshev(op, degree=3), "pcg", ("launches",), {64: (4,), 1: (4,)}),
    "fsai": (lambda tools, op: tools.fsai(op), "pcg", ("launches",), {64: (2,), 1: (2,)}),
    "amg": (lambda tools, op: tools.amg(op, coarse_max=8), "pcg", ("launches",), {64: (19,), 1: (1,)}),
}
# counters of `info` that count applies and so may differ before and after a solve: none of these five kinds has one
# (`applies` and `launches_last_apply` of an L-BFGS operator would be named here)
APPLY_COUNTERS = ()


@pytest.mark.parametrize("n", [64, 1])
@pytest.mark.parametrize("kind", sorted(OBJECTS))
def test_device_objects_share_one_apply_path_and_one_lifetime(kind, n):
    """poisson2d(8) and the 1 x 1 matrix [[2.0]] (`tools.amg` takes it too: one level, its dense inverse).  (1) ``M * v``,
    `apply_device` out of place and in place agree bit for bit; (2) after a solve that ran to convergence -- its loop has
    halted -- ``M * v`` has the bits it had before: the standalone apply reads the object's own never-raised words, not the
    solver's; (3) `info` without its times is what it was; (4) freed twice while a solver holds it, the solve gives the bits
    of the solve with the live object, and afterwards ``M * v`` raises."""
    from pykrylov_amd import CsrOperator, _lib, tools
    from pykrylov_amd.generic import DeviceRun
    make, solver, counters, launches = OBJECTS[kind]
    if n == 1:
        indptr, indices, data, shape = np.array([0, 1]), np.array([0]), np.array([2.0]), (1, 1)
        rhs = np.array([2.0])
    else:
        A = csr_ref.poisson2d(8)
        indptr, indices, data, shape = A.indptr, A.indices, A.data, A.shape
        rhs = A.matvec(np.ones(n))
    op = CsrOperator(indptr, indices, data, shape, symmetric=True)
    M = make(tools, op)
    v = np.random.default_rng(5).standard_normal(n)

    def counts():
        return {k: c for k, c in M.info.items() if not k.endswith("_us") and k not in APPLY_COUNTERS}

    def new_run():
        extra = dict(check_curvature=1, pcg=(False,)) if solver == "pcg" else {}
        return DeviceRun(op, _lib.MK_PCG if solver == "pcg" else _lib.MK_BICGSTAB, rhs, None, precon_diag=M, abstol=0.0,
                         reltol=1e-10, matvec_max=200, **extra)

    def solve(run):
        res = run.run()
        x = run.x()
        assert res.halted and res.converged and res.nMatvec >= 1 and np.all(np.isfinite(x)), (kind, n)
        run.close()
        return x

    # (1)
    y = M * v
    assert y.shape == (n,) and np.all(np.isfinite(y)) and np.any(y != v)
    d_in, d_out = _lib.DeviceArray.from_numpy(v), _lib.DeviceArray(n)
    M.apply_device(d_in, d_out)
    assert np.array_equal(d_out.to_numpy(), y) and np.array_equal(d_in.to_numpy(), v)
    M.apply_device(d_in, d_in)
    assert np.array_equal(d_in.to_numpy(), y)
    d_in.free()
    d_out.free()
    before = counts()
    print("%s n = %d: %s" % (kind, n, before))
    assert tuple(before[c] for c in counters) == launches[n]
    # (2), (3)
    run = new_run()
    assert run.precon_kind == M.route
    x_live = solve(run)
    assert np.array_equal(M * v, y)
    assert counts() == before
    # (4)
    run = new_run()
    M.free()
    M.free()
    assert np.array_equal(solve(run), x_live)
    with pytest.raises(ValueError, match="freed"):
        M * v
    op.free()
