"""Device multi-shift CG (pykrylov_amd.ShiftedCG, csrc/mk_mscg.hip) bit for bit against the NumPy restatement
(tests/_mscg_ref.py) in the device's summation order: one column, a full group, a group boundary and four groups; equal to
`PCG` and `CG` at a zero shift; the grid-stride loop; frozen columns that are really left alone; every storage format; every
way the run can halt; both breakdowns; a matrix-free operator; the C ABI.  Floats are compared as bit patterns throughout."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref, gpu_order
from tests import _mscg_ref as ref
from test_gpu_ilu import device_op, same
from test_gpu_lanczos import fmt_of, set_format
from test_gpu_pcg import matrix, rhs_of
from test_gpu_pcg import solve as pcg_solve

pytestmark = pytest.mark.gpu

_REF = {}


def geometric(ns):
    """`ns` shifts from 1e-3 to 1e3: the large ones freeze early, the small ones late or never."""
    return [1.0] if ns == 1 else [float(s) for s in np.geomspace(1e-3, 1e3, ns)]


def reference(name, op, shifts, **kw):
    """The restatement in the summation order of `op`'s launches, once per (matrix, launch geometry, arguments)."""
    geo = gpu_order.launch_geometry(op)
    key = (name, geo, tuple(shifts)) \
        + tuple(sorted((k, v if np.isscalar(v) or v is None else np.asarray(v).tobytes()) for k, v in kw.items()))
    if key not in _REF:
        A = matrix(name)
        b = kw.pop("rhs", None)
        _REF[key] = ref.mscg(A, rhs_of(name) if b is None else b, shifts,
                             dots=gpu_order.GpuDots(A.shape[0], ["mscg.pq"], geo), **kw)
    return _REF[key]


def solve(op, b, shifts, reltol=1e-6, abstol=1e-8, **kw):
    from pykrylov_amd import ShiftedCG
    s = ShiftedCG(op, reltol=reltol, abstol=abstol)
    s.solve(b, shifts, **kw)
    return s


def check_bits(s, want, what):
    got = (s.nMatvec, s.nIter, s.converged, s.definite, s.breakdown)
    assert got == (want.nMatvec, want.nIter, want.converged, want.definite, want.breakdown), (what, got, want[7:12])
    assert list(s.shiftIters) == list(want.shiftIters), (what, s.shiftIters, want.shiftIters)
    assert same(s.residHistory, want.history) and same(s.shiftResidHistory, want.history2), what
    assert same(s.zeta, want.zeta) and same(s.residNorms, want.residNorms), what
    for k in range(len(want.xs)):
        assert same(s.xs[k], want.xs[k]), (what, k)
    assert same(s.x, want.xs[0]) and s.bestSolution is s.x
    assert same(s.residNorm, want.residNorm) and same(s.residNorm0, want.residNorm0), what


@pytest.mark.parametrize("ns", [1, 8, 9, 32])
@pytest.mark.parametrize("name", ["poisson2d_12", "poisson2d_31", "1138bus"])
def test_bits(name, ns):
    """Less than one workgroup, an odd n (the tail lane), five tiles with irregular rows; one column, a full group, a group
    boundary, four groups."""
    shifts = geometric(ns)
    kw = dict(reltol=1e-10, matvec_max=200)
    op = device_op(matrix(name), True)
    got = solve(op, rhs_of(name), shifts, **kw)
    want = reference(name, op, shifts, **kw)
    check_bits(got, want, (name, ns))
    assert got.nIter >= 10 and got.workspace_bytes == 8 * (3 + 2 * ns) * op.shape[0]
    if ns > 1:                                               # some froze early, and on 1138bus some never
        assert 1 <= got.shiftIters[-1] < got.nIter
        assert (got.shiftIters[0] == -1) == (name == "1138bus")
    op.free()


def test_equal_to_pcg_and_cg_at_a_zero_shift():
    from pykrylov_amd import CG
    name = "poisson2d_31"
    b = rhs_of(name)
    op = device_op(matrix(name), True)
    for kw in (dict(), dict(matvec_max=9)):
        m = solve(op, b, [0.0], reltol=1e-10, **kw)
        p = pcg_solve(op, b, reltol=1e-10, **kw)
        c = CG(op, reltol=1e-10)
        c.solve(b, **kw)
        for other in (p, c):
            assert (m.nMatvec, m.converged) == (other.nMatvec, other.converged) and m.nMatvec > 2
            assert same(m.x, other.x) and same(m.residHistory, other.residHistory) and same(m.residNorm, other.residNorm)
        assert m.nIter == p.nIter and same(m.shiftResidHistory, p.residHistory) and m.zeta[0] == 1.0
    assert m.nMatvec == 9 and not m.converged
    op.free()
    # the brick march, where CG runs fused passes
    name = "march_const"
    op = device_op(matrix(name), True)
    set_format(op, 9)
    m = solve(op, rhs_of(name), [0.0, 0.25], reltol=1e-10, matvec_max=12)
    p = pcg_solve(op, rhs_of(name), reltol=1e-10, matvec_max=12)
    assert fmt_of(op) == 9 and m.nMatvec == p.nMatvec == 12
    assert same(m.x, p.x) and same(m.residHistory, p.residHistory)
    check_bits(m, reference(name, op, [0.0, 0.25], reltol=1e-10, matvec_max=12), "format 9")
    op.free()


def test_grid_stride_and_odd_tail():
    """n beyond 512 workgroups x 512 entries: every lane takes a second pair, and the odd tail; two groups."""
    name = "poisson2d_513"
    A = matrix(name)
    assert A.shape[0] > 512 * 512 and A.shape[0] % 2 == 1
    shifts = geometric(9)
    op = device_op(A, True)
    kw = dict(reltol=1e-14, matvec_max=6)
    got = solve(op, rhs_of(name), shifts, **kw)
    check_bits(got, reference(name, op, shifts, **kw), name)
    assert got.nMatvec == 6
    op.free()


def _run(op, b, shifts, **params):
    """A run through DeviceRun that hands back what `ShiftedCG` does not keep: (result, x_k, p_k, record)."""
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    ns = len(shifts)
    with DeviceRun(op, _lib.MK_MSCG, b, abstol=0.0, check_curvature=1, shifts=shifts, **params) as run:
        res = run.run()
        xs = [run.vector(2 + k) for k in range(ns)]
        ps = [run.vector(2 + ns + k) for k in range(ns)]
        rec = run.vector(2 + 2 * ns).reshape(ns, 3)
    return res, xs, ps, rec


def test_a_frozen_column_is_not_written_again():
    name = "1138bus"
    b = rhs_of(name)
    op = device_op(matrix(name), True)
    shifts = [0.0, 1000.0]
    res, xs, ps, rec = _run(op, b, shifts, reltol=1e-8, matvec_max=100)
    want = reference(name, op, shifts, abstol=0.0, reltol=1e-8, matvec_max=100)
    at = int(rec[1, 2])
    assert res.nMatvec == 100 and res.converged == 0 and res.aux[2] == 1 and rec[0, 2] == -1
    assert 1 <= at < 50 and at == want.shiftIters[1]
    assert same(xs[1], want.xs[1]) and same(xs[0], want.xs[0]) and same(ps[1], want.ps[1]) and same(ps[0], want.ps[0])
    # a run that ends at the freeze pass: a column written after its freeze would differ from it
    res2, xs2, ps2, rec2 = _run(op, b, shifts, reltol=1e-8, matvec_max=at)
    assert res2.nMatvec == at and rec2[1, 2] == at
    assert same(ps2[1], ps[1]) and same(xs2[1], xs[1]) and same(rec2[1], rec[1])
    assert not same(ps2[0], ps[0]) and not same(xs2[0], xs[0])
    op.free()
    # the last group entirely frozen while the first is not: eight small shifts and a huge one
    shifts = [float(s) for s in np.geomspace(1e-4, 1e-2, 8)] + [1e6]
    op = device_op(matrix(name), True)
    got = solve(op, b, shifts, reltol=1e-8, matvec_max=60)
    want = reference(name, op, shifts, reltol=1e-8, matvec_max=60)
    check_bits(got, want, "last group frozen")
    assert 1 <= got.shiftIters[8] < 10 and all(got.shiftIters[:8] == -1) and got.nMatvec == 60
    op.free()


def test_every_storage_format_gives_the_same_bits():
    name = "poisson2d_31"
    shifts = geometric(9)
    kw = dict(reltol=1e-10, matvec_max=40)
    seen = set()
    for fmt in (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8):
        op = device_op(matrix(name), True)
        if fmt >= 0:
            set_format(op, fmt)
        got = solve(op, rhs_of(name), shifts, **kw)
        check_bits(got, reference(name, op, shifts, **kw), ("format", fmt))
        seen.add(fmt_of(op))
        op.free()
    assert 0 in seen and len(seen) >= 3, seen


def test_halt_cases():
    name = "poisson2d_12"
    A = matrix(name)
    n = A.shape[0]
    shifts = geometric(9)
    op = device_op(A, True)
    z = solve(op, np.zeros(n), shifts)
    check_bits(z, reference(name, op, shifts, rhs=np.zeros(n)), "rhs = 0")
    assert z.converged and z.nMatvec == 0 and z.nIter == 0 and not z.xs.any() and z.residHistory == [0.0]
    assert list(z.shiftIters) == [0] * 9
    for mm in (0, 1, 7):
        got = solve(op, rhs_of(name), shifts, reltol=1e-14, matvec_max=mm)
        want = reference(name, op, shifts, reltol=1e-14, matvec_max=mm)
        assert want.nMatvec == mm and not want.converged and len(want.history) == mm + 1
        check_bits(got, want, ("matvec_max", mm))
    # converged in the middle of a batch of passes, and a second solve on the same object
    want = reference(name, op, shifts, reltol=1e-10)
    assert want.converged and 16 < want.nIter < 48 and want.nIter != 32
    got = solve(op, rhs_of(name), shifts, reltol=1e-10)
    check_bits(got, want, "converged inside a batch")
    b2 = A.matvec(np.cos(np.arange(n)))
    got.solve(b2, shifts[:3], matvec_max=9)
    check_bits(got, reference(name, op, shifts[:3], reltol=1e-10, matvec_max=9, rhs=b2), "second solve")
    op.free()


def test_finish_twice_and_iterate_after_the_halt_leave_every_x_alone():
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    name = "1138bus"
    shifts = geometric(9)
    op = device_op(matrix(name), True)
    want = reference(name, op, shifts, reltol=1e-10, matvec_max=40)
    with DeviceRun(op, _lib.MK_MSCG, rhs_of(name), abstol=1e-8, reltol=1e-10, matvec_max=40, check_curvature=1,
                   shifts=shifts) as run:
        res = run.run()
        assert res.halted and res.nMatvec == 40 and res.aux[0] == 9
        xs = [run.vector(2 + k) for k in range(9)]
        assert all(same(x, w) for x, w in zip(xs, want.xs)) and same(run.x(), want.xs[0])
        run.finish()
        run.finish()
        assert run.iterate(3) == 0
        run.finish()
        assert all(same(run.vector(2 + k), xs[k]) for k in range(9))
        assert same(run.history(), want.history) and same(run.history2(), want.history2)
    op.free()


def test_breakdowns():
    b = rhs_of("poisson2d_12")
    # -A: the curvature test stops the first pass with nothing updated
    name = "neg_poisson2d_12"
    op = device_op(matrix(name), True)
    shifts = [0.0, 1.0]
    got = solve(op, b, shifts)
    want = reference(name, op, shifts, rhs=b)
    check_bits(got, want, "-A")
    assert not got.definite and got.breakdown == 1 and got.nMatvec == 1 and got.nIter == 0 and not got.xs.any()
    assert same(got.infiniteDescent, want.p) and same(got.infiniteDescent, b)
    on = solve(op, b, shifts, check_curvature=False, matvec_max=20)
    check_bits(on, reference(name, op, shifts, rhs=b, check_curvature=False, matvec_max=20), "no curvature test")
    assert on.definite and on.nIter > 1 and on.infiniteDescent is None
    op.free()
    # an indefinite diagonal matrix whose first <p, A p> is negative
    d = np.array([1.0, -3.0, 2.0, -4.0, 1.0])
    D = csr_ref.from_coo(np.arange(5), np.arange(5), d, (5, 5))
    op = device_op(D, True)
    rhs = np.arange(1.0, 6.0)
    got = solve(op, rhs, shifts)
    want = ref.mscg(D, rhs, shifts)
    assert got.breakdown == want.breakdown == 1 and not got.definite and same(got.infiniteDescent, want.p)
    op.free()
    # c I and sigma = -c: alpha(0) = 1 / c, so 1 + sigma alpha is exactly zero in the first pass
    c = 4.0
    D = csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, c), (5, 5))
    op = device_op(D, True)
    shifts = [1.0, -c]
    got = solve(op, rhs, shifts)
    want = ref.mscg(D, rhs, shifts)
    assert want.breakdown == 2
    check_bits(got, want, "1 + sigma alpha = 0")
    assert got.breakdown == 2 and got.definite and not got.converged and got.nMatvec == 1 and got.nIter == 0
    assert not got.xs.any() and list(got.shiftIters) == [-1, -1]
    op.free()
    # ... and the library goes on working
    op = device_op(matrix("poisson2d_12"), True)
    check_bits(solve(op, b, shifts[:1], reltol=1e-10), reference("poisson2d_12", op, shifts[:1], reltol=1e-10), "afterwards")
    op.free()


def test_matrix_free_operator():
    from pykrylov_amd import LinearOperator
    name = "1138bus"
    A = matrix(name)
    n = A.shape[0]
    calls = [0]
    shifts = geometric(9)

    def mv(v):
        calls[0] += 1
        return A.matvec(v)
    got = solve(LinearOperator(n, n, matvec=mv, symmetric=True), rhs_of(name), shifts, reltol=1e-10, matvec_max=60)
    assert calls[0] == got.nMatvec == 60
    op = device_op(A, True)
    set_format(op, 0)
    twin = solve(op, rhs_of(name), shifts, reltol=1e-10, matvec_max=60)
    assert same(twin.xs, got.xs) and same(twin.residHistory, got.residHistory) and same(twin.zeta, got.zeta)
    assert list(twin.shiftIters) == list(got.shiftIters)
    # ... and a right-hand side that already lives on the device
    from pykrylov_amd import _lib
    d_b = _lib.DeviceArray.from_numpy(rhs_of(name))
    dev = solve(op, d_b, shifts, reltol=1e-10, matvec_max=60)
    assert same(dev.xs, twin.xs)
    d_b.free()
    op.free()


def test_errors_through_the_c_abi():
    from pykrylov_amd import _lib
    name = "poisson2d_12"
    A = matrix(name)
    n = A.shape[0]
    op = device_op(A, True)
    lib = _lib.init()
    ARG, UNSUPPORTED = -2, -5

    def block(kind, nsigma, sigma=()):
        blk = _lib.MkParamsShifts()
        blk.base.struct_size = ctypes.sizeof(_lib.MkParamsShifts)
        blk.base.kind, blk.base.abstol, blk.base.reltol, blk.base.matvec_max, blk.base.check_curvature = kind, 1e-8, 1e-6, 10, 1
        blk.nsigma = nsigma
        for k, s in enumerate(sigma):
            blk.sigma[k] = s
        return blk

    h = ctypes.c_void_p()
    for blk in (block(_lib.MK_MSCG, 0), block(_lib.MK_MSCG, 33), block(_lib.MK_MSCG, 2, [0.0, float("nan")]),
                block(_lib.MK_MSCG, 1, [float("inf")])):
        assert lib.mk_solver_create(op.handle, ctypes.byref(blk.base), ctypes.byref(h)) == ARG
    short = _lib.MkParams(struct_size=ctypes.sizeof(_lib.MkParams), kind=_lib.MK_MSCG, abstol=1e-8, reltol=1e-6, matvec_max=10)
    assert lib.mk_solver_create(op.handle, ctypes.byref(short), ctypes.byref(h)) == ARG       # no shifts in the short block
    _lib.check(lib.mk_csr_set_row_block(op.handle, 1))
    good = block(_lib.MK_MSCG, 2, [0.0, 0.5])
    assert lib.mk_solver_create(op.handle, ctypes.byref(good.base), ctypes.byref(h)) == UNSUPPORTED
    _lib.check(lib.mk_csr_set_row_block(op.handle, 0))
    _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(good.base), ctypes.byref(h)))
    d = _lib.DeviceArray.from_numpy(np.ones(n))
    assert lib.mk_solver_set_precon_diag(h, d.ptr) == UNSUPPORTED
    assert lib.mk_solver_set_precon_csr(h, op.handle) == UNSUPPORTED
    assert lib.mk_solver_set_pcg(h, 0) == UNSUPPORTED
    d_b = _lib.DeviceArray.from_numpy(rhs_of(name))
    assert lib.mk_solver_setup(h, d_b.ptr, d.ptr) == ARG                                      # a guess
    res = _lib.MkResult()
    _lib.check(lib.mk_solver_solve(h, d_b.ptr, None, ctypes.byref(res)))
    want = reference(name, op, [0.0, 0.5], matvec_max=10)
    assert res.nMatvec == 10 and res.itn == 10 and res.aux[0] == 2 and res.aux[1] == 0 and res.aux[3] == 8 * 7 * n
    assert same(res.residNorm, want.residNorm) and res.aux[2] == sum(want.shiftIters >= 0)
    p, ln = ctypes.c_void_p(), ctypes.c_int64()
    for index in (3 + 2 * 2, -1, 100):
        assert lib.mk_solver_vector(h, index, ctypes.byref(p), ctypes.byref(ln)) == ARG
    _lib.check(lib.mk_solver_vector(h, 2 + 2 * 2, ctypes.byref(p), ctypes.byref(ln)))
    assert ln.value == 6
    _lib.check(lib.mk_solver_vector(h, 3, ctypes.byref(p), ctypes.byref(ln)))
    assert ln.value == n and same(_lib.download(p.value, n), want.xs[1])
    _lib.check(lib.mk_solver_destroy(h))
    # every other kind takes the long block too and does not read its tail: PCG with garbage there
    runs = []
    for sigma in ([0.0] * 32, [float("nan"), float("inf")] + [1e300] * 30):
        blk = block(_lib.MK_PCG, -7 if sigma[0] != 0.0 else 0, sigma)
        _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(blk.base), ctypes.byref(h)))
        _lib.check(lib.mk_solver_solve(h, d_b.ptr, None, ctypes.byref(res)))
        px = ctypes.c_void_p()
        _lib.check(lib.mk_solver_x(h, ctypes.byref(px)))
        runs.append((res.nMatvec, res.residNorm, _lib.download(px.value, n)))
        _lib.check(lib.mk_solver_destroy(h))
    assert runs[0][0] == runs[1][0] == 10 and same(runs[0][1], runs[1][1]) and same(runs[0][2], runs[1][2])
    assert same(runs[0][2], pcg_solve(op, rhs_of(name), matvec_max=10).x)
    d.free()
    d_b.free()
    op.free()
