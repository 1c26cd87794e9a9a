"""Device Chebyshev filter (pykrylov_amd.tools.cheb_filter, csrc/mk_chebfilt.hip) and the filtered cycle of thick-restart
Lanczos (mk_params_filter, csrc/mk_trlan.hip) bit for bit against the NumPy restatement (tests/_chebfilt_ref.py) in the
device's summation order: set-up, applies in every storage format met here and in both buffer parities, filtered solves at
both ends of the spectrum, the budget halts, repeated solves, the wrappers and the errors.  Floats are compared as bit
patterns throughout."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref, gpu_order
from tests import _chebfilt_ref as ref
from test_gpu_ilu import device_op, same
from test_gpu_lanczos import fmt_of, set_format
from test_gpu_trlan import matrix

pytestmark = pytest.mark.gpu

DEGREES = (1, 2, 3, 5)     # the first-step form alone; the first use of y_{j-2}; the owned buffers reused in both parities
SIDES = ("SA", "LA")
_EIG, _APPLY, _RUN = {}, {}, {}


def eigs(name):
    """The DISTINCT eigenvalues, ascending (dense): a single-vector Lanczos method returns one copy of a multiple eigenvalue,
    and poisson2d's spectrum is full of pairs."""
    if name not in _EIG:
        ev = np.linalg.eigvalsh(matrix(name).to_dense())
        _EIG[name] = ev[np.concatenate(([True], np.diff(ev) > 1e-9 * ev[-1]))]
    return _EIG[name]


def plain_interval(A, side):
    """An interval for the applies from the Gershgorin interval alone: the far three quarters of it unwanted (its far end
    left to the device), the reference point a twentieth of its width outside the wanted end."""
    lo, hi = ref.gershgorin(A)
    w = hi - lo
    return ((lo + 0.25 * w, None), lo - 0.05 * w) if side == "SA" else ((None, hi - 0.25 * w), hi + 0.05 * w)


def applied(name, A, side, degree):
    """The restated apply to a fixed vector, once per (matrix, side, degree)."""
    key = (name, side, degree)
    if key not in _APPLY:
        x = np.random.default_rng(17).standard_normal(A.shape[0])
        iv, a0 = plain_interval(A, side)
        a, b = ref.interval(A, *iv)
        _APPLY[key] = (x, ref.apply(A, x, degree, a, b, a0))
    return _APPLY[key]


def check_applies(name, A, op, what):
    from pykrylov_amd import tools
    for side in SIDES:
        iv, a0 = plain_interval(A, side)
        for k in DEGREES:
            x, want = applied(name, A, side, k)
            F = tools.cheb_filter(op, degree=k, interval=iv, ref=a0)
            assert same(F * x, want), (what, side, k)
            F.free()


# ---------------------------------------------------------------------------------------------- 1. set-up
@pytest.mark.parametrize("name", ["varcoef_7_5_3", "poisson2d_31", "1138bus"])
def test_coefficients_and_the_gershgorin_interval_are_the_restatements(name):
    from pykrylov_amd import tools
    A = matrix(name)
    op = device_op(A, True)
    lo, hi = ref.gershgorin(A)
    w = hi - lo
    for k, iv, a0 in ((1, (None, None), lo - 1.0), (7, (None, None), hi + 0.5), (128, (lo + 0.125 * w, None), lo - 0.01 * w),
                      (16, (None, hi - 0.125 * w), hi + 0.01 * w), (5, (0.25, 1.5), 1.75)):
        F = tools.cheb_filter(op, degree=k, interval=iv, ref=a0)
        a, b = ref.interval(A, *iv)
        assert F.interval == (a, b) and F.ref == a0 and F.degree == k and F.side == ("LA" if a0 > b else "SA"), (name, k, F.interval)
        c, e, p, q = F.coefficients
        rc, re_, rp, rq = ref.coefficients(a, b, a0, k)
        assert c == rc and e == re_ and same(p, rp) and same(q, rq) and len(p) == len(q) == k
        info = F.info
        assert (info["rows"], info["degree"], info["side"], info["launches"]) == (A.shape[0], k, int(a0 > b), k)
        assert (info["a_default"], info["b_default"]) == (int(iv[0] is None), int(iv[1] is None))
        assert info["bytes"] >= min(k - 1, 2) * 8 * A.shape[0] and info["bytes"] < 2 * 8 * (A.shape[0] + 2) + 64
        assert F.symmetric and F.shape == A.shape and F.pilotMatvec == 0
        F.free()
    op.free()


# ---------------------------------------------------------------------------------------------- 2. applies
@pytest.mark.parametrize("fmt", [0, -1], ids=["format0", "default_format"])
@pytest.mark.parametrize("name", ["varcoef_7_5_3", "poisson2d_31", "1138bus"])
def test_apply_bits(name, fmt):
    """n = 105 (less than one workgroup, the scalar tail), 961 and irregular rows; on the plain CSR kernel and in the format
    the builder chooses."""
    A = matrix(name)
    op = device_op(A, True)
    if fmt >= 0:
        set_format(op, fmt)
    check_applies(name, A, op, (name, fmt))
    if fmt == 0:
        assert fmt_of(op) == 0
    op.free()


@pytest.mark.parametrize("fmt", [9, 10, 11])
def test_apply_bits_on_the_march_formats(fmt):
    """The 128 x 8 x 7 grid forced into the brick-march formats: 9 and 10 run the steps as the pipelined march kernel with
    y_{j-2}[r] prefetched (in the first step the prefetch reads the input vector and its value is dropped); 11 has no kernel
    for this epilogue and takes the CSR gather kernel on the same arrays."""
    name = "march_const" if fmt == 9 else "march_varcoef"
    A = matrix("march_const") if fmt == 9 else _march_varcoef()
    op = device_op(A, True)
    set_format(op, fmt)
    x = applied(name, A, "SA", 1)[0]
    assert same(op * x, A.matvec(x)) and fmt_of(op) == fmt
    check_applies(name, A, op, ("march", fmt))
    assert fmt_of(op) == fmt
    op.free()


def _march_varcoef():
    if "march_varcoef" not in _EIG:
        _EIG["march_varcoef"] = csr_ref.poisson3d_varcoef(128, 8, 7)
    return _EIG["march_varcoef"]


def test_apply_bits_where_the_product_grid_strides():
    name = "poisson1d_300001"
    A = matrix(name)
    ntiles = (A.shape[0] + gpu_order.BLOCK - 1) // gpu_order.BLOCK
    assert gpu_order.grid_spmv(ntiles) < ntiles                  # every workgroup takes more than one tile
    op = device_op(A, True)
    from pykrylov_amd import tools
    for side, k in (("SA", 3), ("LA", 2)):
        iv, a0 = plain_interval(A, side)
        x, want = applied(name, A, side, k)
        F = tools.cheb_filter(op, degree=k, interval=iv, ref=a0)
        assert same(F * x, want), (side, k)
        F.free()
    op.free()


# ---------------------------------------------------------------------------------------------- 3. the input, and twice
def test_the_input_is_unchanged_and_two_applies_agree():
    from pykrylov_amd import _lib, tools
    name = "poisson2d_31"
    A = matrix(name)
    op = device_op(A, True)
    iv, a0 = plain_interval(A, "SA")
    for k in DEGREES:
        x, want = applied(name, A, "SA", k)
        F = tools.cheb_filter(op, degree=k, interval=iv, ref=a0)
        d_in, d_out = _lib.DeviceArray.from_numpy(x), _lib.DeviceArray(A.shape[0])
        F.apply_device(d_in, d_out)
        first = d_out.to_numpy()
        assert same(d_in.to_numpy(), x) and same(first, want), k
        F.apply_device(d_in, d_out)
        assert same(d_in.to_numpy(), x) and same(d_out.to_numpy(), first), k
        assert same(F * x, first)
        F.apply_device(d_in, d_in)                               # (the result is formed in the object's own vector)
        assert same(d_in.to_numpy(), first), k
        d_in.free()
        d_out.free()
        F.free()
    op.free()


# ---------------------------------------------------------------------------------------------- 4 - 7. the filtered cycle
RELTOL = 1e-8


def cut(name, which, nev):
    """An interval from the dense eigenvalues: the cut two eigenvalues behind the nev wanted ones, the far end Gershgorin's
    (left to the device), the reference point a hundredth of the spectrum's width outside the wanted end."""
    ev = eigs(name)
    w = ev[-1] - ev[0]
    return ((float(ev[nev + 2]), None), float(ev[0] - 0.01 * w)) if which == "SA" else \
        ((None, float(ev[-3 - nev])), float(ev[-1] + 0.01 * w))


def reference(name, nev, which, degree, geometry=None, **kw):
    key = (name, nev, which, degree, repr(geometry)) + tuple(sorted(kw.items()))
    if key not in _RUN:
        A = matrix(name)
        iv, a0 = cut(name, which, nev)
        a, b = ref.interval(A, *iv)
        dots = gpu_order.GpuDots(A.shape[0], (), geometry=geometry)          # (no dot of this loop is fused into a product)
        _RUN[key] = ref.trlan_filtered(A, nev, which, degree, a, b, a0, reltol=RELTOL, dots=lambda x, y: dots(x, y, "trlan"), **kw)
    return _RUN[key]


def solve(op, name, nev, which, degree, **kw):
    from pykrylov_amd import ThickRestartLanczos, tools
    iv, a0 = cut(name, which, nev)
    F = tools.cheb_filter(op, degree=degree, interval=iv, ref=a0)
    s = ThickRestartLanczos(op, reltol=RELTOL, abstol=0.0)
    s.solve(nev, which=which, filter=F, **kw)
    F.free()
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


def true_residuals(A, s):
    return np.array([np.linalg.norm(A.matvec(s.X[i]) - s.w[i] * s.X[i]) for i in range(len(s.w))])


@pytest.mark.parametrize("degree", [2, 5])
@pytest.mark.parametrize("which", SIDES)
@pytest.mark.parametrize("nev,ncv", [(1, 8), (4, 16)])
@pytest.mark.parametrize("name", ["varcoef_7_5_3", "poisson2d_31"])
def test_filtered_solve_bits_and_true_residuals(name, nev, ncv, which, degree):
    """`w`, `X`, `residNorms`, `residHistory` and the counts are the restatement's; the host's own ||A x - w x|| of the downloaded
    vectors is at most 2 reltol lambda_max."""
    A = matrix(name)
    op = device_op(A, True)
    kw = dict(ncv=ncv, matvec_max=3000)
    s = solve(op, name, nev, which, degree, **kw)
    want = reference(name, nev, which, degree, geometry=gpu_order.launch_geometry(op), **kw)
    check_bits(s, want, (name, nev, ncv, which, degree))
    lam = eigs(name)[-1]
    true = true_residuals(A, s)
    print(name, nev, ncv, which, degree, "products", s.nMatvec, "steps", s.nIter, "cycles", s.cycles, "true residual / lambda_max",
          np.max(true) / lam)
    assert s.converged and s.outside == 0 and s.filter_degree == degree and s.pilotMatvec == 0
    assert np.max(true) <= 2.0 * RELTOL * lam
    ev = eigs(name)
    assert np.max(np.abs(s.w - (ev[:nev] if which == "SA" else ev[-nev:]))) <= 1e-12 * lam
    assert s.nMatvec == degree * s.nIter + nev * len(want.verified)
    op.free()


def test_filtered_solve_bits_on_a_march_format():
    name = "march_const"
    A = matrix(name)
    op = device_op(A, True)
    set_format(op, 9)
    lo, hi = ref.gershgorin(A)
    from pykrylov_amd import ThickRestartLanczos, tools
    iv, a0 = (1.0, None), -0.25
    F = tools.cheb_filter(op, degree=3, interval=iv, ref=a0)
    s = ThickRestartLanczos(op, reltol=RELTOL)
    kw = dict(ncv=9, matvec_max=9 * 3 + 2 + 4 * 3 + 2)            # two cycles, each verified only if it is the last
    s.solve(2, which="SA", filter=F, **kw)
    assert fmt_of(op) == 9
    dots = gpu_order.GpuDots(A.shape[0], (), geometry=gpu_order.launch_geometry(op))
    want = ref.trlan_filtered(A, 2, "SA", 3, 1.0, hi, a0, reltol=RELTOL, dots=lambda x, y: dots(x, y, "trlan"), **kw)
    check_bits(s, want, "format 9")
    assert s.cycles == 2 and s.nMatvec == 41 and not s.converged
    F.free()
    op.free()


@pytest.mark.parametrize("cycles", [1, 2, 3])
def test_budget_halts(cycles):
    """A budget for exactly one, two or three cycles: not converged, never exceeded, and the residuals returned are true
    residuals (the last cycle the budget allows is verified on A)."""
    name, nev, ncv, d = "1138bus", 4, 16, 2
    A = matrix(name)
    op = device_op(A, True)
    keep = ref.default_keep(nev, ncv)
    mm = ncv * d + nev + (cycles - 1) * ((ncv - keep) * d + nev) + 3          # (3 short of one more product of slack: no more cycle)
    kw = dict(ncv=ncv, matvec_max=mm)
    want = reference(name, nev, "SA", d, **kw)
    s = solve(op, name, nev, "SA", d, **kw)
    check_bits(s, want, ("matvec_max", mm))
    assert not s.converged and s.cycles == cycles and s.nMatvec <= mm and s.nMatvec == d * s.nIter + nev
    true = true_residuals(A, s)
    assert np.max(np.abs(s.residNorms - true)) <= 1e-12 * eigs(name)[-1]
    assert s.residNorm == np.max(s.residNorms) > s.threshold
    op.free()


def test_a_second_solve_and_finish_twice_change_nothing():
    from pykrylov_amd import _lib, tools
    from pykrylov_amd.generic import DeviceRun
    name, nev, ncv, d = "varcoef_7_5_3", 4, 16, 5
    A = matrix(name)
    op = device_op(A, True)
    kw = dict(ncv=ncv, matvec_max=3000)
    want = reference(name, nev, "LA", d, **kw)
    iv, a0 = cut(name, "LA", nev)
    F = tools.cheb_filter(op, degree=d, interval=iv, ref=a0)
    from pykrylov_amd import ThickRestartLanczos
    s = ThickRestartLanczos(op, reltol=RELTOL)
    for _ in range(2):
        s.solve(nev, which="LA", filter=F, **kw)
        check_bits(s, want, "solve")
    with DeviceRun(op, _lib.MK_TRLAN, None, abstol=0.0, reltol=RELTOL, matvec_max=3000, eig=(nev, ncv, 1, 0, 1),
                   filter=(d,) + F.interval + (F.ref,)) as run:
        res = run.run()
        assert res.converged and res.nMatvec == want.nMatvec and res.itn == want.nIter
        X = np.stack([run.vector(i) for i in range(nev)])
        assert same(X, want.X) and same(run.x(), want.X[0])
        run.finish()
        assert run.iterate(3) == 0
        res = run.finish()
        assert res.nMatvec == want.nMatvec and same(np.stack([run.vector(i) for i in range(nev)]), X)
        assert same(run.history(), want.history) and same(run.vector(nev).reshape(nev, 3)[:, 0], want.w)
    F.free()
    op.free()


# ---------------------------------------------------------------------------------------------- 8. the wrappers
def test_eigsh_with_a_degree_and_solve_with_the_object_agree():
    import pykrylov_amd
    from pykrylov_amd import ThickRestartLanczos, tools
    name = "poisson2d_31"
    A = matrix(name)
    op = device_op(A, True)
    w, X = pykrylov_amd.eigsh(op, k=3, which="SA", tol=RELTOL, filter=5)
    F = tools.cheb_filter_for(op, 3, "SA", degree=5)
    assert F.degree == min(5, tools.cheb_filter_degree_cap(F.interval[0], F.interval[1], F.ref)) and F.pilotMatvec == 20
    assert F.side == "SA" and F.interval[1] == ref.gershgorin(A)[1] and F.interval[0] >= eigs(name)[3] and F.ref < F.interval[0]
    s = ThickRestartLanczos(op, reltol=RELTOL, abstol=0.0)
    s.solve(3, which="SA", filter=F)
    assert s.converged and same(s.w, w) and same(s.X.T, X)
    assert s.filter_degree == F.degree and s.filter_interval == F.interval and s.pilotMatvec == 20 and s.outside == 0
    lam = eigs(name)[-1]
    assert np.max(np.abs(w - eigs(name)[:3])) <= 1e-12 * lam and np.max(true_residuals(A, s)) <= 2.0 * RELTOL * lam
    F.free()
    # a hand-given interval that covers wanted eigenvalues: they are damped, not found, and the result says so
    ev = eigs(name)
    bad = tools.cheb_filter(op, degree=5, interval=(float(0.5 * (ev[0] + ev[1])), None), ref=float(ev[0] - 0.1))
    s.solve(3, which="SA", filter=bad, matvec_max=1500)
    assert s.outside >= 1 and not s.converged
    bad.free()
    op.free()


# ---------------------------------------------------------------------------------------------- 9. errors
def test_errors():
    from pykrylov_amd import LinearOperator, ThickRestartLanczos, _lib, tools
    A = matrix("varcoef_7_5_3")
    n = A.shape[0]
    op = device_op(A, True)
    lib = _lib.init()
    h = ctypes.c_void_p()
    nan = float("nan")

    def block(kind, k, a, b, a0, which=0, mm=400, restart=0):
        f = _lib.MkParamsFilter()
        p = f.eig.base
        p.struct_size, p.kind, p.reltol, p.matvec_max, p.restart = ctypes.sizeof(_lib.MkParamsFilter), kind, 1e-8, mm, restart
        f.eig.nev, f.eig.ncv, f.eig.which, f.eig.keep, f.eig.seed = 2, 9, which, 0, 1
        f.degree, f.a, f.b, f.a0 = k, a, b, a0
        return f

    def create(k, a, b, a0, operator=op, kind=_lib.MK_TRLAN, **kw):
        f = block(kind, k, a, b, a0, **kw)
        return lib.mk_solver_create(operator.handle, ctypes.byref(f.eig.base), ctypes.byref(h))
    # part 1: a >= b, a0 inside or not finite, an infinite end, the degree, a matrix that is not square
    for args in ((4, 2.0, 2.0, 0.0), (4, 3.0, 2.0, 0.0), (4, 1.0, 2.0, 1.5), (4, 1.0, 2.0, 1.0), (4, 1.0, 2.0, nan),
                 (4, 1.0, 2.0, float("inf")), (4, 1.0, float("inf"), 0.0), (0, 1.0, 2.0, 0.0), (129, 1.0, 2.0, 0.0),
                 (4, nan, nan, 1.0)):                                                        # (a0 inside the Gershgorin interval)
        assert create(*args) == -2, args                                                     # MK_ERR_ARG
    R = csr_ref.from_coo(np.arange(4), np.arange(4), np.ones(4), (4, 6))
    rect = device_op(R, False)
    assert create(2, 1.0, 2.0, 0.0, rect) == -2
    _lib.check(lib.mk_csr_set_row_block(op.handle, 1))
    assert create(2, 1.0, 2.0, 0.0) == -5                                                    # MK_ERR_UNSUPPORTED
    _lib.check(lib.mk_csr_set_row_block(op.handle, 0))
    # part 2: another kind; the other side; a restart that is neither the solver nor the probe; a budget below the first cycle
    for kind in (_lib.MK_CG, _lib.MK_MINRES, _lib.MK_LOBPCG, _lib.MK_TRSVD):
        assert create(2, 1.0, 2.0, 0.0, kind=kind) == -5
    assert create(2, 1.0, 2.0, 0.0, which=1) == -2
    assert create(2, 1.0, 2.0, 0.0, restart=2) == -2
    assert create(2, 1.0, 2.0, 0.0, mm=19) == 0
    assert lib.mk_solver_setup(h, None, None) == -2                                          # 9 * 2 + 2 = 20 products do not fit
    p, ln = ctypes.c_void_p(), ctypes.c_int64()
    assert lib.mk_solver_vector(h, 3, ctypes.byref(p), ctypes.byref(ln)) == 0 and ln.value == 5 + 2 * 2 + 8    # the table
    assert lib.mk_solver_vector(h, 4, ctypes.byref(p), ctypes.byref(ln)) == -2
    _lib.check(lib.mk_solver_destroy(h))
    # the probe: `which` means nothing, it needs a vector, and its result is the solver's own vector
    d = _lib.DeviceArray.from_numpy(np.ones(n))
    assert create(2, 1.0, 2.0, 0.0, which=1, restart=1) == 0
    assert lib.mk_solver_setup(h, None, None) == -2
    assert lib.mk_solver_setup(h, d.ptr, None) == 0 and lib.mk_solver_x(h, ctypes.byref(p)) == 0 and p.value != d.ptr
    assert same(_lib.download(p.value, n), ref.apply(A, np.ones(n), 2, 1.0, 2.0, 0.0)) and same(d.to_numpy(), np.ones(n))
    _lib.check(lib.mk_solver_destroy(h))
    other = device_op(A, True)
    # part 3: the Python checks
    for kw in (dict(degree=0), dict(degree=129), dict(degree=2.0), dict(interval=(2.0, 1.0)), dict(interval=(1.0, float("inf"))),
               dict(interval=1.0), dict(ref=None), dict(ref=1.5), dict(ref=float("nan"))):
        with pytest.raises(ValueError):
            tools.cheb_filter(op, **dict(dict(degree=4, interval=(1.0, 2.0), ref=0.0), **kw))
    unsym = device_op(A, False)
    with pytest.raises(ValueError, match="symmetric"):
        tools.cheb_filter(unsym, 4, (1.0, 2.0), 0.0)
    with pytest.raises(ValueError, match="Ritz values"):
        tools.cheb_filter_for(op, 4, "SA", steps=4)
    with pytest.raises(ValueError, match="which"):
        tools.cheb_filter_for(op, 4, "SM")
    G = tools.cheb_filter(op, 4, (1.0, None), 0.0)
    with pytest.raises(ValueError, match="DeviceArray"):
        G.apply_device(d, np.ones(n))
    with pytest.raises(ValueError, match="other"):
        ThickRestartLanczos(op).solve(2, which="LA", filter=G)
    with pytest.raises(ValueError, match="another matrix"):
        ThickRestartLanczos(other).solve(2, which="SA", filter=G)
    with pytest.raises(ValueError, match="matrix-free or composed"):
        ThickRestartLanczos(LinearOperator(n, n, matvec=A.matvec, symmetric=True)).solve(2, filter=G)
    with pytest.raises(ValueError, match="matvec_max"):
        ThickRestartLanczos(op).solve(2, which="SA", ncv=9, filter=G, matvec_max=37)
    G.free()
    with pytest.raises(ValueError, match="freed"):
        ThickRestartLanczos(op).solve(2, which="SA", filter=G)
    # the library goes on working
    x = np.random.default_rng(1).standard_normal(n)
    assert same(op * x, A.matvec(x))
    for o in (op, other, rect, unsym):
        o.free()
    d.free()
