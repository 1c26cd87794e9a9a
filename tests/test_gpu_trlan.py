"""Device thick-restart Lanczos (pykrylov_amd.ThickRestartLanczos, csrc/mk_trlan.hip) bit for bit against the NumPy
restatement (tests/_trlan_ref.py) in the device's summation order: less than one workgroup, the odd tail, irregular rows;
basis sizes that meet a full group of columns, a group of one, three groups and five; one rotation launch and two (the
out-of-place route); both ends of the spectrum; format 0, the builder's format and a march format; the grid-stride loop;
every way the run can halt; start vectors; a matrix-free operator; the argument errors of the long parameter block.  Floats
are compared as bit patterns throughout."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref, gpu_order
from tests import _trlan_ref as ref
from test_gpu_gmres import matrix as _gmres_matrix
from test_gpu_ilu import device_op, same
from test_gpu_lanczos import fmt_of, set_format

pytestmark = pytest.mark.gpu

G = 8                                                        # basis columns per launch (GM_GROUP, csrc/mk_multicol.h)
KT = ref.KT                                                  # output columns per rotation launch
_MAT, _REF = {}, {}


def matrix(name):
    if name not in _MAT:
        if name == "varcoef_7_5_3":
            _MAT[name] = csr_ref.poisson3d_varcoef(7, 5, 3)
        elif name == "poisson2d_31":
            _MAT[name] = csr_ref.poisson2d(31)
        elif name == "poisson1d_300001":
            _MAT[name] = csr_ref.poisson1d(300001)
        else:
            _MAT[name] = _gmres_matrix(name)                 # 1138bus, 2.5I_5, march_const
    return _MAT[name]


def reference(name, nev, geometry=None, **kw):
    """The restatement with the device's dots in the operator's launch geometry, once per (matrix, geometry, arguments)."""
    key = (name, nev, repr(geometry)) + tuple(sorted((k, v if np.isscalar(v) or v is None else np.asarray(v).tobytes())
                                                for k, v in kw.items()))
    if key not in _REF:
        A = matrix(name)
        dots = gpu_order.GpuDots(A.shape[0], (), geometry=geometry)          # (no dot of this loop is fused into a product)
        _REF[key] = ref.trlan(A, nev, dots=lambda a, b: dots(a, b, "trlan"), **kw)
    return _REF[key]


def solve(op, nev, reltol=1e-10, abstol=0.0, **kw):
    from pykrylov_amd import ThickRestartLanczos
    s = ThickRestartLanczos(op, reltol=reltol, abstol=abstol)
    s.solve(nev, **kw)
    return s


def counts(r):
    return (r.nMatvec, r.nIter, r.cycles, r.nconv, bool(r.converged), bool(r.breakdown), r.ncv, r.keep, r.sweeps)


def check_bits(s, want, what):
    assert counts(s) == counts(want), (what, counts(s), counts(want))
    assert same(s.residHistory, want.history), what
    assert same(s.w, want.w) and same(s.residNorms, want.residNorms), what
    assert np.array_equal(s.pairIters, want.pairIters), what
    assert same(s.X, want.X), what
    assert same(s.anorm, want.anorm) and same(s.threshold, want.threshold), what
    assert same(s.residNorm, want.residNorm) and same(s.residNorm0, want.residNorm0), what


def workspace(n, ncv, keep):
    "The documented layout: ncv + 1 columns and 16 (ceil(keep / 16) - 1) spare ones of n rounded up to even, plus 2, doubles."
    return 8 * (ncv + 1 + KT * ((keep + KT - 1) // KT - 1)) * (n + (n & 1) + 2)


SHAPES = [(1, G), (2, G + 1), (4, 2 * G + 1), (16, 40)]       # (nev, ncv): a full group, a group of one, three groups, five


@pytest.mark.parametrize("which", ["SA", "LA"])
@pytest.mark.parametrize("nev,ncv", SHAPES)
@pytest.mark.parametrize("name", ["varcoef_7_5_3", "poisson2d_31"])
def test_bits(name, nev, ncv, which):
    """Less than one workgroup and an odd n (the tail lane); on the plain CSR kernel and in the builder's format.  (16, 40)
    keeps 28 vectors: two rotation launches, the first into the spare columns."""
    A = matrix(name)
    n = A.shape[0]
    kw = dict(which=which, ncv=ncv, matvec_max=160)
    for fmt in (0, -1):
        op = device_op(A, True)
        if fmt >= 0:
            set_format(op, fmt)
        s = solve(op, nev, **kw)
        want = reference(name, nev, geometry=gpu_order.launch_geometry(op), **kw)
        check_bits(s, want, (name, nev, ncv, which, fmt))
        assert s.cycles >= 2 and s.workspace_bytes == workspace(n, ncv, s.keep)
        assert (s.keep > KT) == (nev == 16)
        if fmt == 0:
            assert fmt_of(op) == 0
        op.free()


@pytest.mark.parametrize("nev,ncv,keep", [(4, 16, None), (16, 40, None), (4, 40, 33)])
def test_irregular_rows_largest(nev, ncv, keep):
    """1138bus from the top; keep = 33 takes three rotation launches."""
    name = "1138bus"
    op = device_op(matrix(name), True)
    kw = dict(which="LA", ncv=ncv, keep=keep, matvec_max=400)
    want = reference(name, nev, **kw)
    s = solve(op, nev, **kw)
    check_bits(s, want, (name, nev, ncv, keep))
    assert s.converged and s.workspace_bytes == workspace(1138, ncv, s.keep)
    lam = np.linalg.eigvalsh(matrix(name).to_dense())[-nev:]
    assert np.max(np.abs(s.w - lam)) <= 1e-12 * lam[-1]
    op.free()


def test_grid_stride_and_odd_tail():
    """n beyond 512 workgroups x 512 entries: every lane takes a second pair, and the odd tail; out of products."""
    name = "poisson1d_300001"
    A = matrix(name)
    assert A.shape[0] > 512 * 512 and A.shape[0] % 2 == 1
    op = device_op(A, True)
    kw = dict(which="LA", ncv=9, matvec_max=18)
    want = reference(name, 2, geometry=gpu_order.launch_geometry(op), **kw)
    s = solve(op, 2, **kw)
    check_bits(s, want, name)
    assert not s.converged and s.cycles >= 2 and s.nMatvec <= 18 and s.nMatvec + (9 - s.keep) > 18
    op.free()


def test_march_format():
    name = "march_const"
    A = matrix(name)
    op = device_op(A, True)
    set_format(op, 9)
    kw = dict(which="SA", ncv=9, matvec_max=13)
    s = solve(op, 2, **kw)
    assert fmt_of(op) == 9
    check_bits(s, reference(name, 2, geometry=gpu_order.launch_geometry(op), **kw), "format 9")
    assert s.cycles == 2 and s.nMatvec == 13 and not s.converged
    op.free()


def test_halt_cases():
    # converged: test_bits.  Out of products, with room for several cycles and for none but the first
    name = "1138bus"
    op = device_op(matrix(name), True)
    for mm in (60, 16):
        kw = dict(which="SA", ncv=16, matvec_max=mm)
        want = reference(name, 4, **kw)
        assert not want.converged and want.nMatvec <= mm and want.residNorm > want.threshold
        s = solve(op, 4, **kw)
        check_bits(s, want, ("matvec_max", mm))
        assert (s.cycles == 1) == (mm == 16) and np.all(s.pairIters[s.residNorms > s.threshold] == -1)
    op.free()
    # a breakdown that leaves enough vectors, and one that does not
    name = "2.5I_5"
    op = device_op(matrix(name), True)
    one = solve(op, 1, ncv=3)
    check_bits(one, reference(name, 1, ncv=3), "breakdown, nev = 1")
    assert one.breakdown and one.converged and one.nIter == 1 and one.X.shape == (1, 5) and list(one.residNorms) == [0.0]
    two = solve(op, 2, which="LA", ncv=3)
    check_bits(two, reference(name, 2, which="LA", ncv=3), "breakdown, nev = 2")
    assert two.breakdown and not two.converged and two.nconv == 1 and two.w.shape == (1,) and two.X.shape == (1, 5)
    op.free()
    # a basis as large as the matrix: the last step breaks down, every pair is exact
    name = "varcoef_7_5_3"
    op = device_op(matrix(name), True)
    s = solve(op, 4, ncv=105)
    check_bits(s, reference(name, 4, ncv=105), "ncv = n")
    assert s.breakdown and s.converged and s.nIter == 105 and s.cycles == 1 and not s.residNorms.any()
    op.free()


def test_start_vectors_and_a_second_solve():
    from pykrylov_amd import _lib
    name = "poisson2d_31"
    A = matrix(name)
    n = A.shape[0]
    op = device_op(A, True)
    v0 = np.cos(np.arange(n)) + 2.0
    kw = dict(which="LA", ncv=17, matvec_max=120)
    want = reference(name, 3, start=v0, **kw)
    s = solve(op, 3, start=v0, **kw)
    check_bits(s, want, "host start")
    d_v = _lib.DeviceArray.from_numpy(v0)
    check_bits(solve(op, 3, start=d_v, **kw), want, "device start")
    assert same(d_v.to_numpy(), v0)
    d_v.free()
    # another seed is another run; the same object solves again with a fresh object's bits
    other = reference(name, 3, seed=5, **kw)
    assert not same(other.history, reference(name, 3, **kw).history)
    s.solve(3, seed=5, **kw)
    check_bits(s, other, "second solve")
    s.solve(3, start=v0, **kw)
    check_bits(s, want, "third solve")
    op.free()


def test_finish_twice_and_iterate_after_the_halt_change_nothing():
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    name = "varcoef_7_5_3"
    op = device_op(matrix(name), True)
    want = reference(name, 2, which="LA", ncv=9, matvec_max=160)
    with DeviceRun(op, _lib.MK_TRLAN, None, abstol=0.0, reltol=1e-10, matvec_max=160, eig=(2, 9, 1, 0, 1)) as run:
        run.setup()
        assert run.iterate(1) == 9                           # one pass is one cycle
        res = run.finish()
        assert not res.halted and res.itn == 9 and res.aux[0] == 1 and res.aux[2] == want.keep
        while not res.halted:
            run.iterate(1 << 20)
            res = run.finish()
        assert res.converged and res.nMatvec == want.nMatvec
        X = np.stack([run.vector(i) for i in range(2)])
        assert same(X, want.X) and same(run.x(), want.X[0])
        run.finish()
        assert run.iterate(3) == 0
        res = run.finish()
        assert same(np.stack([run.vector(i) for i in range(2)]), X) and same(run.history(), want.history)
        assert same(run.vector(2).reshape(2, 3)[:, 0], want.w)
        p, ln = ctypes.c_void_p(), ctypes.c_int64()
        assert run.lib.mk_solver_vector(run.handle, 3, ctypes.byref(p), ctypes.byref(ln)) == -2
    op.free()


def test_the_composed_rotation_has_the_kernels_bits():
    """mk_params.window != 0 composes the rotation of GmOpCombine launches (what tools/trlan_bench.py times the kernel
    against): other launches, keep spare columns, the same bits."""
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    name = "poisson2d_31"
    A = matrix(name)
    n = A.shape[0]
    op = device_op(A, True)
    for nev, ncv in ((2, G + 1), (16, 40)):
        want = reference(name, nev, which="LA", ncv=ncv, matvec_max=160)
        with DeviceRun(op, _lib.MK_TRLAN, None, abstol=0.0, reltol=1e-10, matvec_max=160, window=1, eig=(nev, ncv, 1, 0, 1)) as run:
            res = run.run()
            assert (res.nMatvec, res.itn, int(res.aux[0]), bool(res.converged)) == \
                (want.nMatvec, want.nIter, want.cycles, want.converged)
            assert same(np.stack([run.vector(i) for i in range(nev)]), want.X) and same(run.history(), want.history)
            assert same(run.vector(nev).reshape(nev, 3)[:, 0], want.w)
            assert res.aux[3] == 8 * (ncv + 1 + want.keep) * (n + (n & 1) + 2)
            ms = run.history2()
            assert len(ms) == want.cycles and np.all(ms >= 0.0)
    op.free()


def test_matrix_free_operator():
    from pykrylov_amd import LinearOperator
    name = "varcoef_7_5_3"
    A = matrix(name)
    n = A.shape[0]
    kw = dict(which="SA", ncv=G + 1, matvec_max=160)
    want = reference(name, 2, **kw)
    calls = [0]

    def mv(v):
        calls[0] += 1
        return A.matvec(v)
    s = solve(LinearOperator(n, n, matvec=mv, symmetric=True), 2, **kw)
    check_bits(s, want, "matrix free")
    assert calls[0] == s.nMatvec


def test_eigsh_wrapper():
    import pykrylov_amd
    name = "varcoef_7_5_3"
    op = device_op(matrix(name), True)
    w, X = pykrylov_amd.eigsh(op, k=3, which="SA", tol=1e-10)
    want = reference(name, 3, which="SA", reltol=1e-10)
    assert same(w, want.w) and same(X, want.X.T)
    slow = device_op(matrix("1138bus"), True)
    with pytest.raises(RuntimeError, match="converged"):
        pykrylov_amd.eigsh(slow, k=4, which="SA", ncv=16, maxiter=40)
    slow.free()
    op.free()


def test_errors():
    from pykrylov_amd import _lib, ThickRestartLanczos
    A = matrix("varcoef_7_5_3")
    n = A.shape[0]
    op = device_op(A, True)
    lib = _lib.init()
    h = ctypes.c_void_p()

    def block(nev, ncv, which=0, keep=0, size=None, kind=_lib.MK_TRLAN):
        b = _lib.MkParamsEig()
        b.base.struct_size = ctypes.sizeof(_lib.MkParamsEig) if size is None else size
        b.base.kind, b.base.abstol, b.base.reltol, b.base.matvec_max = kind, 0.0, 1e-10, 200
        b.nev, b.ncv, b.which, b.keep, b.seed = nev, ncv, which, keep, 1
        return b

    def create(b, operator=op):
        return lib.mk_solver_create(operator.handle, ctypes.byref(b.base), ctypes.byref(h))
    # a wrong struct_size, nev >= ncv, ncv > n, ncv > 128 (on a matrix that has the rows), keep out of range, which
    big = device_op(matrix("poisson2d_31"), True)
    for b, o in ((block(2, 9, size=ctypes.sizeof(_lib.MkParamsEig) + 8), op), (block(0, 9), op), (block(9, 9), op), (block(10, 9), op),
                 (block(2, n + 1), op), (block(2, 129), big), (block(4, 16, keep=3), op), (block(4, 16, keep=16), op),
                 (block(4, 16, keep=-1), op), (block(2, 9, which=2), op)):
        assert create(b, o) == -2                                                            # MK_ERR_ARG
    # the short block and the shifts block
    short = _lib.MkParams(struct_size=ctypes.sizeof(_lib.MkParams), kind=_lib.MK_TRLAN, abstol=0.0, reltol=1e-10, matvec_max=200)
    assert lib.mk_solver_create(op.handle, ctypes.byref(short), ctypes.byref(h)) == -2
    sh = _lib.MkParamsShifts()
    sh.base.struct_size, sh.base.kind, sh.base.matvec_max, sh.nsigma = ctypes.sizeof(_lib.MkParamsShifts), _lib.MK_TRLAN, 200, 1
    assert lib.mk_solver_create(op.handle, ctypes.byref(sh.base), ctypes.byref(h)) == -2
    # another kind takes the eig block and ignores its tail
    cg = block(0, 0, kind=_lib.MK_CG)
    assert create(cg) == 0
    _lib.check(lib.mk_solver_destroy(h))
    # a good block: a guess and matvec_max < ncv at set-up, every preconditioner setter
    good = block(2, 9)
    assert create(good) == 0
    d = _lib.DeviceArray.from_numpy(np.ones(n))
    assert lib.mk_solver_setup(h, d.ptr, d.ptr) == -2
    assert lib.mk_solver_set_precon_diag(h, d.ptr) == -5                                     # MK_ERR_UNSUPPORTED
    assert lib.mk_solver_set_precon_csr(h, op.handle) == -5
    zero = _lib.DeviceArray.from_numpy(np.zeros(n))
    assert lib.mk_solver_setup(h, zero.ptr, None) == -2                                      # a start vector without a norm
    assert lib.mk_solver_setup(h, None, None) == 0                                           # the hashed start vector
    _lib.check(lib.mk_solver_destroy(h))
    few = block(2, 9)
    few.base.matvec_max = 8
    assert create(few) == 0
    assert lib.mk_solver_setup(h, None, None) == -2
    _lib.check(lib.mk_solver_destroy(h))
    # a partitioned handle: the C call refuses, the class raises before it creates anything
    _lib.check(lib.mk_csr_set_row_block(op.handle, 1))
    assert create(block(2, 9)) == -5
    _lib.check(lib.mk_csr_set_row_block(op.handle, 0))
    op.local_size = n // 2
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        ThickRestartLanczos(op).solve(2)
    del op.local_size
    # a matrix holding an inf is an error, and the library goes on working
    data = A.data.copy()
    data[10] = np.inf
    I = device_op(csr_ref.RefCsr(A.indptr, A.indices, data, A.shape), True)
    with pytest.raises(_lib.MkError, match="not finite"):
        ThickRestartLanczos(I).solve(2, ncv=9)
    kw = dict(which="LA", ncv=9, matvec_max=160)
    check_bits(solve(op, 2, **kw), reference("varcoef_7_5_3", 2, **kw), "after the inf")
    for o in (op, big, I):
        o.free()
    d.free()
    zero.free()
