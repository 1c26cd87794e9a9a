"""Device thick-restart SVD (pykrylov_amd.ThickRestartSVD, csrc/mk_trsvd.hip) bit for bit against the NumPy restatement
(tests/_trsvd_ref.py) in the device's summation order: a tall matrix and a wide one (the swap), less than one workgroup and
several, odd lengths; basis sizes of one, two, four and five column groups, rotation tiles of 4, 8 and 16 and the spare
columns; both ends of the spectrum and both reorthogonalisation modes -- the one-sided mode's <u, u> is summed in the row
order of A's product kernel --; plain CSR and the builder's format for A and A'; the grid-stride loop; every way the run can
halt; start vectors; a matrix-free operator; the wrapper; the argument errors of Python and of the C ABI.  Floats are compared
as bit patterns throughout."""
import ctypes
import os

import numpy as np
import pytest

from oracle import csr_ref, gpu_order
from tests import _trsvd_ref as ref
from test_gpu_gmres import matrix as _gmres_matrix                       # noqa: F401  (what test_gpu_trlan.py imports)
from test_gpu_ilu import device_op, same
from test_gpu_lanczos import fmt_of, set_format

pytestmark = pytest.mark.gpu

KT = ref.KT                                                  # output columns per rotation launch
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("full", "one-sided")
_MAT, _REF = {}, {}


def rnd(R, C, per, seed):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(R), per)
    cols = rng.integers(0, C, R * per)
    vals = rng.random(R * per) - 0.5
    return csr_ref.from_coo(rows, cols, vals, (R, C))


def matrix(name):
    "The TALL matrix of a case; the cases named `..._T` hand its transpose to the class."
    if name not in _MAT:
        if name == "rank_deficient":
            S = rnd(50, 5, 3, 11)
            _MAT[name] = csr_ref.RefCsr(S.indptr, S.indices, S.data, (50, 20))
        elif name == "jpwh_991":
            _MAT[name] = csr_ref.read_matrix_market(os.path.join(GOLDEN, "jpwh_991.mtx"))
        elif name == "diag_7_5":                             # 3 I_5 on top of two zero rows: A v_1 = 3 [v_1; 0], A' u_1 = 3 v_1
            _MAT[name] = csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, 3.0), (7, 5))
        else:
            _MAT[name] = {"rnd_300_120": lambda: rnd(300, 120, 5, 3), "rnd_211_60": lambda: rnd(211, 60, 4, 5),
                          "rnd_stride": lambda: rnd(300001, 270001, 2, 13)}[name]()
    return _MAT[name]


def operators(name, wide=False):
    """(the operator handed to the class, its tall side) on the device."""
    A = matrix(name)
    op = device_op(A.transpose() if wide else A, False)
    return op, (op.T if wide else op)


def reference(name, nsv, geometry=None, **kw):
    """The restatement with the device's dots -- <u, u> of the one-sided mode in the launch geometry of the tall operator's
    product --, once per (matrix, geometry, arguments)."""
    key = (name, nsv, repr(geometry)) + tuple(sorted((k, v if np.isscalar(v) or v is None else np.asarray(v).tobytes())
                                                for k, v in kw.items()))
    if key not in _REF:
        A = matrix(name)
        dots = gpu_order.GpuDots(A.shape[0], [ref.SITE_UU], geometry=geometry)
        _REF[key] = ref.trsvd(A, nsv, dots=dots, **kw)
    return _REF[key]


def solve(op, nsv, reltol=1e-10, abstol=0.0, **kw):
    from pykrylov_amd import ThickRestartSVD
    s = ThickRestartSVD(op, reltol=reltol, abstol=abstol)
    s.solve(nsv, **kw)
    return s


def counts(r):
    return (r.nMatvec, r.nIter, r.cycles, r.nconv, bool(r.converged), int(r.breakdown), r.ncv, r.keep, r.reorth, r.sweeps)


def check_bits(s, want, what, wide=False):
    assert counts(s) == counts(want), (what, counts(s), counts(want))
    assert same(s.residHistory, want.history), what
    assert same(s.s, want.s) and same(s.residNorms, want.residNorms), what
    assert np.array_equal(s.pairIters, want.pairIters), what
    left, right = (s.V, s.U) if wide else (s.U, s.V)         # (of the tall operator)
    assert same(left, want.U) and same(right, want.V), what
    assert same(s.anorm, want.anorm) and same(s.threshold, want.threshold), what
    assert same(s.residNorm, want.residNorm) and same(s.residNorm0, want.residNorm0), what
    assert s.transposed == wide and not np.isnan(s.U).any() and not np.isnan(s.V).any()


def workspace(R, C, ncv, keep):
    "The documented layout: ncv (U) and ncv + 1 (V) columns and 16 (ceil(keep / 16) - 1) spare ones each, of the length rounded up to even, plus 2, doubles."
    spare = KT * ((keep + KT - 1) // KT - 1)
    return 8 * ((ncv + spare) * (R + (R & 1) + 2) + (ncv + 1 + spare) * (C + (C & 1) + 2))


SHAPES = [(1, 8, None), (4, 16, None), (8, 32, None), (16, 40, None), (4, 40, 33)]


@pytest.mark.parametrize("reorth", MODES)
@pytest.mark.parametrize("which", ["LM", "SM"])
@pytest.mark.parametrize("nsv,ncv,keep", SHAPES)
@pytest.mark.parametrize("name,wide", [("rnd_300_120", False), ("rnd_211_60", True)])
def test_bits(name, wide, nsv, ncv, keep, which, reorth):
    """One, two, four and five column groups; keeps of 4, 10, 20 (tiles of 4, 8 and 16 columns), 28 and 33 (two and three
    rotation launches, the first into the spare columns); the wide case is swapped by the class."""
    R, C = matrix(name).shape
    kw = dict(which=which, ncv=ncv, keep=keep, reorth=reorth, matvec_max=160)
    op, tall = operators(name, wide)
    s = solve(op, nsv, **kw)
    want = reference(name, nsv, geometry=gpu_order.launch_geometry(tall), **kw)
    check_bits(s, want, (name, nsv, ncv, keep, which, reorth), wide)
    assert s.cycles >= 2 and s.workspace_bytes == workspace(R, C, ncv, s.keep)
    assert s.U.shape == (nsv, op.shape[0]) and s.V.shape == (nsv, op.shape[1])
    op.free()


@pytest.mark.parametrize("reorth", MODES)
def test_irregular_rows_square_nonsymmetric(reorth):
    name = "jpwh_991"
    kw = dict(which="LM", ncv=16, reorth=reorth, matvec_max=400)
    op, tall = operators(name)
    s = solve(op, 4, **kw)
    check_bits(s, reference(name, 4, geometry=gpu_order.launch_geometry(tall), **kw), (name, reorth))
    assert s.converged
    sv = np.linalg.svd(matrix(name).to_dense(), compute_uv=False)
    assert np.max(np.abs(s.s - sv[:4])) <= 1e-12 * sv[0]
    op.free()


@pytest.mark.parametrize("reorth", MODES)
def test_grid_stride_and_odd_tails(reorth):
    """Both lengths beyond 512 workgroups x 512 entries and odd: every lane of the stream kernels takes a second pair, and the
    odd tail, in the long space and in the short one; out of products after two cycles."""
    name = "rnd_stride"
    R, C = matrix(name).shape
    assert C > 512 * 512 and R > C and R % 2 == 1 and C % 2 == 1
    op, tall = operators(name)
    kw = dict(which="LM", ncv=9, reorth=reorth, matvec_max=26)
    want = reference(name, 2, geometry=gpu_order.launch_geometry(tall), **kw)
    s = solve(op, 2, **kw)
    check_bits(s, want, (name, reorth))
    assert not s.converged and s.cycles == 2 and s.nMatvec == 26
    op.free()


@pytest.mark.parametrize("reorth", MODES)
def test_storage_formats(reorth):
    """Plain CSR and the builder's format, for A and A': the same bits (the one-sided <u, u> follows the launch geometry)."""
    name = "rnd_300_120"
    kw = dict(which="LM", ncv=16, reorth=reorth, matvec_max=160)
    runs = []
    for fmt in (0, -1):
        op, tall = operators(name)
        if fmt >= 0:
            set_format(op, fmt)
            set_format(op.T, fmt)
        s = solve(op, 4, **kw)
        check_bits(s, reference(name, 4, geometry=gpu_order.launch_geometry(tall), **kw), (name, reorth, fmt))
        if fmt == 0:
            assert fmt_of(op) == 0 and fmt_of(op.T) == 0
        runs.append(s)
        op.free()
    assert same(runs[0].s, runs[1].s) and same(runs[0].U, runs[1].U) and same(runs[0].V, runs[1].V)


@pytest.mark.parametrize("reorth", MODES)
def test_halt_cases(reorth):
    # converged: test_irregular_rows_square_nonsymmetric.  Out of products: test_bits.  No room for the first cycle:
    name = "rnd_300_120"
    op, tall = operators(name)
    geo = gpu_order.launch_geometry(tall)
    kw = dict(which="LM", ncv=16, reorth=reorth, matvec_max=31)
    s = solve(op, 4, **kw)
    check_bits(s, reference(name, 4, geometry=geo, **kw), "no room")
    assert s.cycles == 0 and s.nMatvec == 0 and not s.converged and s.breakdown == 0
    assert s.s.shape == (0,) and s.U.shape == (0, 300) and s.V.shape == (0, 120) and s.residHistory == []
    # a start vector without a positive, finite norm: halted before the first step, nothing NaN
    for bad in (np.zeros(120), np.full(120, np.inf)):
        kw = dict(which="LM", ncv=16, reorth=reorth, start=bad)
        z = solve(op, 4, **kw)
        assert z.breakdown == 3 and z.cycles == 0 and z.nMatvec == 0 and not z.converged
        assert z.s.shape == (0,) and z.U.shape == (0, 300) and z.V.shape == (0, 120) and z.residNorms.shape == (0,)
        assert counts(z)[:6] == counts(reference(name, 4, geometry=geo, **kw))[:6]
    # the object still solves
    kw = dict(which="LM", ncv=16, reorth=reorth, matvec_max=160)
    check_bits(solve(op, 4, **kw), reference(name, 4, geometry=geo, **kw), "after the bad start vectors")
    op.free()
    # a basis as large as the short side: the last step's beta breaks down, every triplet is exact
    name = "rnd_211_60"
    op, tall = operators(name)
    kw = dict(which="SM", ncv=60, reorth=reorth)
    s = solve(op, 4, **kw)
    check_bits(s, reference(name, 4, geometry=gpu_order.launch_geometry(tall), **kw), "ncv = ncols")
    assert s.breakdown == 1 and s.converged and s.nIter == 60 and s.cycles == 1 and not s.residNorms.any()
    op.free()
    # a beta breakdown that leaves too few triplets
    name = "diag_7_5"
    op, tall = operators(name)
    geo = gpu_order.launch_geometry(tall)
    one = solve(op, 1, ncv=3, reorth=reorth)
    check_bits(one, reference(name, 1, geometry=geo, ncv=3, reorth=reorth), "breakdown, nsv = 1")
    assert one.breakdown == 1 and one.converged and one.nIter == 1 and one.nMatvec == 2 and list(one.residNorms) == [0.0]
    two = solve(op, 2, ncv=3, reorth=reorth)
    check_bits(two, reference(name, 2, geometry=geo, ncv=3, reorth=reorth), "breakdown, nsv = 2")
    assert two.breakdown == 1 and not two.converged and two.nconv == 1 and two.s.shape == (1,) and two.U.shape == (1, 7)
    op.free()
    # an alpha breakdown: a rank-deficient matrix
    name = "rank_deficient"
    op, tall = operators(name)
    geo = gpu_order.launch_geometry(tall)
    kw = dict(which="LM", ncv=10, reorth=reorth)
    s = solve(op, 3, **kw)
    check_bits(s, reference(name, 3, geometry=geo, **kw), "alpha breakdown")
    assert s.breakdown == 2 and s.converged and s.nIter == 6 and s.nMatvec == 11
    kw = dict(which="SM", ncv=10, reorth=reorth)
    z = solve(op, 2, **kw)
    check_bits(z, reference(name, 2, geometry=geo, **kw), "alpha breakdown, the zero")
    assert z.breakdown == 2 and z.s[-1] == 0.0 and not z.U[-1].any()
    op.free()


def test_start_vectors_and_a_second_solve():
    from pykrylov_amd import _lib
    name = "rnd_300_120"
    op, tall = operators(name)
    geo = gpu_order.launch_geometry(tall)
    v0 = np.cos(np.arange(120)) + 2.0
    kw = dict(which="LM", ncv=17, reorth="one-sided", matvec_max=120)
    want = reference(name, 3, geometry=geo, start=v0, **kw)
    s = solve(op, 3, start=v0, **kw)
    check_bits(s, want, "host start")
    d_v = _lib.DeviceArray.from_numpy(v0)
    check_bits(solve(op, 3, start=d_v, **kw), want, "device start")
    assert same(d_v.to_numpy(), v0)
    # another start is another run; the same object solves again with a fresh object's bits
    other = reference(name, 3, geometry=geo, seed=5, **kw)
    assert not same(other.history, want.history)
    s.solve(3, seed=5, **kw)
    check_bits(s, other, "second solve")
    s.solve(3, start=d_v, **kw)
    check_bits(s, want, "third solve")
    d_v.free()
    op.free()


@pytest.mark.parametrize("reorth", [1, 0])
def test_finish_twice_and_iterate_after_the_halt_change_nothing(reorth):
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    name = "rnd_300_120"
    op, tall = operators(name)
    want = reference(name, 2, geometry=gpu_order.launch_geometry(tall), which="LM", ncv=9, matvec_max=400,
                     reorth=MODES[1 - reorth])
    with DeviceRun(op, _lib.MK_TRSVD, None, transpose=op.T, abstol=0.0, reltol=1e-10, matvec_max=400, reorth=reorth,
                   eig=(2, 9, 1, 0, 1)) as run:
        run.setup()
        assert run.iterate(1) == 9                           # one pass is one cycle
        res = run.finish()
        assert not res.halted and res.itn == 9 and res.nMatvec == 18 and res.aux[0] == 1 and res.aux[2] == want.keep
        assert res.aux[6] == reorth
        while not res.halted:
            run.iterate(1 << 20)
            res = run.finish()
        assert res.converged and res.nMatvec == want.nMatvec and res.istop == want.sweeps
        V = np.stack([run.vector(i) for i in range(2)])
        U = np.stack([run.vector(2 + i) for i in range(2)])
        assert same(V, want.V) and same(U, want.U) and same(run.x(), want.V[0])
        run.finish()
        assert run.iterate(3) == 0
        res = run.finish()
        assert same(np.stack([run.vector(i) for i in range(2)]), V) and same(np.stack([run.vector(2 + i) for i in range(2)]), U)
        assert same(run.history(), want.history) and same(run.vector(4).reshape(2, 3)[:, 0], want.s)
        ms = run.history2()
        assert len(ms) == want.cycles and np.all(ms >= 0.0)
        p, ln = ctypes.c_void_p(), ctypes.c_int64()
        assert run.lib.mk_solver_vector(run.handle, 5, ctypes.byref(p), ctypes.byref(ln)) == -2
    op.free()


@pytest.mark.parametrize("reorth", MODES)
def test_matrix_free_operator(reorth):
    from pykrylov_amd import LinearOperator
    name = "rnd_300_120"
    A = matrix(name)
    R, C = A.shape
    kw = dict(which="LM", ncv=16, reorth=reorth, matvec_max=160)
    op, tall = operators(name)
    csr = solve(op, 4, **kw)
    calls = [0, 0]

    def mv(v):
        calls[0] += 1
        return A.matvec(v)

    def mvt(u):
        calls[1] += 1
        return A.rmatvec(u)
    s = solve(LinearOperator(C, R, matvec=mv, matvec_transp=mvt), 4, **kw)
    check_bits(s, reference(name, 4, geometry=gpu_order.launch_geometry(tall), **kw), "matrix free")
    assert same(s.s, csr.s) and same(s.U, csr.U) and same(s.V, csr.V)
    assert calls[0] == s.nIter and calls[0] + calls[1] == s.nMatvec
    # ... and a wide one: the class swaps the two callables
    calls[:] = [0, 0]
    w = solve(LinearOperator(R, C, matvec=mvt, matvec_transp=mv), 4, **kw)
    assert w.transposed and same(w.s, csr.s) and same(w.V, csr.U) and same(w.U, csr.V)
    assert calls[0] == w.nIter and calls[0] + calls[1] == w.nMatvec
    op.free()


def test_svds_wrapper():
    import pykrylov_amd
    name = "rnd_300_120"
    A = matrix(name)
    op, tall = operators(name)
    U, s, Vt = pykrylov_amd.svds(op, k=3, tol=1e-10)
    want = reference(name, 3, geometry=gpu_order.launch_geometry(tall), reltol=1e-10)
    assert U.shape == (300, 3) and s.shape == (3,) and Vt.shape == (3, 120) and np.all(np.diff(s) <= 0)
    assert same(s, want.s) and same(U, want.U.T) and same(Vt, want.V)
    D = A.to_dense()
    assert np.max(np.abs(D @ Vt.T - U * s[None, :])) <= 2e-10 * s[0]      # U diag(s) Vt acts as A on the right vectors
    assert np.max(np.abs((U * s[None, :]) @ (Vt @ Vt.T) - U * s[None, :])) <= 1e-12 * s[0]
    with pytest.raises(RuntimeError, match="converged"):
        pykrylov_amd.svds(op, k=4, which="SM", ncv=16, maxiter=40)
    op.free()


def test_errors():
    from pykrylov_amd import _lib, ThickRestartSVD
    A = matrix("rnd_211_60")
    R, C = A.shape
    op, tall = operators("rnd_211_60")
    # through Python
    with pytest.raises(ValueError, match="preconditioner"):
        ThickRestartSVD(op, precon=np.ones(C)).solve(2)
    for kw in (dict(nsv=8, ncv=8), dict(nsv=2, ncv=C + 1), dict(nsv=2, which="LA"), dict(nsv=2, reorth="partial")):
        with pytest.raises(ValueError):
            ThickRestartSVD(op).solve(**kw)
    op.local_size = R // 2
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        ThickRestartSVD(op).solve(2)
    del op.local_size
    # through the C ABI
    lib = _lib.init()
    h = ctypes.c_void_p()

    def block(nev, ncv, which=1, keep=0, reorth=1, size=None):
        b = _lib.MkParamsEig()
        b.base.struct_size = ctypes.sizeof(_lib.MkParamsEig) if size is None else size
        b.base.kind, b.base.abstol, b.base.reltol, b.base.matvec_max, b.base.reorth = _lib.MK_TRSVD, 0.0, 1e-10, 400, reorth
        b.nev, b.ncv, b.which, b.keep, b.seed = nev, ncv, which, keep, 1
        return b

    def create(b, operator=op):
        return lib.mk_solver_create(operator.handle, ctypes.byref(b.base), ctypes.byref(h))
    for b in (block(0, 9), block(9, 9), block(2, C + 1), block(4, 16, keep=3), block(4, 16, keep=16), block(2, 9, which=2),
              block(2, 9, reorth=2), block(2, 9, reorth=-1)):
        assert create(b) == -2                                                               # MK_ERR_ARG
    assert create(block(2, 9), op.T) == -2                                                   # a wide matrix handed to the kind
    short = _lib.MkParams(struct_size=ctypes.sizeof(_lib.MkParams), kind=_lib.MK_TRSVD, abstol=0.0, reltol=1e-10, matvec_max=400,
                          reorth=1)
    assert lib.mk_solver_create(op.handle, ctypes.byref(short), ctypes.byref(h)) == -2
    sh = _lib.MkParamsShifts()
    sh.base.struct_size, sh.base.kind, sh.base.matvec_max, sh.base.reorth, sh.nsigma = \
        ctypes.sizeof(_lib.MkParamsShifts), _lib.MK_TRSVD, 400, 1, 1
    assert lib.mk_solver_create(op.handle, ctypes.byref(sh.base), ctypes.byref(h)) == -2
    # a good block: set-up without a transpose, a guess, every preconditioner setter
    assert create(block(2, 9)) == 0
    d = _lib.DeviceArray.from_numpy(np.ones(R))
    assert lib.mk_solver_setup(h, None, None) == -3                                          # MK_ERR_STATE
    _lib.check(lib.mk_solver_set_transpose(h, op.T.handle))
    assert lib.mk_solver_setup(h, d.ptr, d.ptr) == -2
    assert lib.mk_solver_set_precon_diag(h, d.ptr) == -5                                     # MK_ERR_UNSUPPORTED
    assert lib.mk_solver_set_precon_csr(h, op.handle) == -5
    assert lib.mk_solver_set_lls_precon(h, d.ptr, None) == -5
    assert lib.mk_solver_set_lls_precon_csr(h, 0, op.handle) == -5
    assert lib.mk_solver_setup(h, None, None) == 0                                           # the hashed start vector
    _lib.check(lib.mk_solver_destroy(h))
    # a partitioned handle: the C call refuses
    _lib.check(lib.mk_csr_set_row_block(op.handle, 1))
    assert create(block(2, 9)) == -5
    _lib.check(lib.mk_csr_set_row_block(op.handle, 0))
    # a matrix holding an inf is an error, and the library goes on working
    data = A.data.copy()
    data[10] = np.inf
    bad = device_op(csr_ref.RefCsr(A.indptr, A.indices, data, A.shape), False)
    with pytest.raises(_lib.MkError, match="not finite"):
        ThickRestartSVD(bad).solve(2, ncv=9)
    kw = dict(which="LM", ncv=9, reorth="one-sided", matvec_max=160)
    check_bits(solve(op, 2, **kw), reference("rnd_211_60", 2, geometry=gpu_order.launch_geometry(tall), **kw), "after the inf")
    for o in (op, bad):
        o.free()
    d.free()
