"""Device Lanczos spectrum estimate (pykrylov_amd.tools.lanczos, csrc/mk_lanczos.hip) and the Chebyshev preconditioner built on
its interval (``tools.chebyshev(interval='lanczos')``): alpha, beta and the step count bit for bit against the NumPy
restatement (tests/_lanczos_ref.py) in the device's summation order, in every storage format met here; early stop, clamping,
launch count; the preconditioner's interval, coefficients and applies; solves on the device route against the host route;
that the interval helps; errors.  Floats are compared as bit patterns throughout."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref, gpu_order, krylov_ref as kr
from tests import _cheb_ref as cheb_ref, _lanczos_ref as ref
from test_gpu_ilu import _solve, device_op, ref_matrix, same

pytestmark = pytest.mark.gpu

MATRICES = ("poisson2d_12", "poisson2d_100", "1138bus", "varcoef_20_20_5", "diagonal")
STEPS = (1, 2, 10)

_MAT, _REF = {}, {}


def matrix(name):
    if name not in _MAT:
        if name == "poisson2d_12":
            _MAT[name] = csr_ref.poisson2d(12)
        elif name == "2.5I_5":
            _MAT[name] = csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, 2.5), (5, 5))
        elif name == "poisson1d_3":
            _MAT[name] = csr_ref.poisson1d(3)
        elif name == "one_row":
            _MAT[name] = csr_ref.from_coo(np.arange(1), np.arange(1), np.full(1, 2.0), (1, 1))
        elif name == "march_const":
            _MAT[name] = csr_ref.poisson3d(128, 8, 7)
        elif name == "march_var":
            _MAT[name] = csr_ref.poisson3d_varcoef(128, 8, 7)
        else:
            _MAT[name] = ref_matrix(name)
    return _MAT[name]


def set_format(op, fmt):
    from pykrylov_amd import _lib
    _lib.check(_lib.init().mk_csr_set_format(op.handle, fmt))


def fmt_of(op):
    from pykrylov_amd import _lib
    fmt = ctypes.c_int32()
    _lib.check(_lib.init().mk_csr_format_info(op.handle, ctypes.byref(fmt), None, None, None, None))
    return fmt.value


def geometry_of(op):
    """(grid, tile order) of the product launches the fused dot <v, A v> is summed in.  Format 11 has no kernel for the
    Lanczos epilogue: its steps run as the CSR gather kernel, on the march's grid, in the matrix's tile order."""
    from pykrylov_amd import _lib
    if fmt_of(op) == 11:
        g, m = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.init().mk_csr_launch_info(op.handle, ctypes.byref(g), ctypes.byref(m)))
        assert m.value in (0, 1, 2)
        return g.value, m.value
    return gpu_order.launch_geometry(op)


def reference(name, steps, scaled, geo, start=None):
    """The restatement in the device's summation order, computed once per (matrix, steps, scaling, launch geometry)."""
    key = (name, steps, scaled, geo, None if start is None else start.tobytes())
    if key not in _REF:
        A = matrix(name)
        _REF[key] = ref.lanczos(A, steps=steps, scale_diag=scaled, seed=1, start=start, dots=ref.GpuDots(A.shape[0], geo))
    return _REF[key]


def check_bits(got, want, what):
    assert got.steps == want.steps == got.info["steps"], (what, got.steps, want.steps)
    assert same(got.alpha, want.alpha), (what, got.alpha, want.alpha)
    assert same(got.beta, want.beta), (what, got.beta, want.beta)
    assert same(got.ritz, want.ritz) and same(got.residuals, want.residuals) and got.bounds == want.bounds, what
    assert got.info["nonfinite"] == 0 and got.info["bytes"] > 0


@pytest.mark.parametrize("fmt", [0, -1], ids=["format0", "default_format"])
@pytest.mark.parametrize("name", MATRICES)
def test_alpha_beta_and_steps_bits(name, fmt):
    """One tile, many workgroups, an odd n, irregular rows; scaled and not; 1, 2 and 10 steps; on the plain CSR kernel and in
    the format the builder chooses."""
    from pykrylov_amd import tools
    A = matrix(name)
    op = device_op(A, True)
    if fmt >= 0:
        set_format(op, fmt)
    geo = geometry_of(op)
    for scaled in (False, True):
        for steps in STEPS:
            got = tools.lanczos(op, steps=steps, scale_diag=scaled)
            check_bits(got, reference(name, steps, scaled, geo), (name, fmt, scaled, steps))
            assert got.info["launches"] <= 2 * steps + 3, got.info
            if name == "diagonal" and scaled:
                assert got.steps == 1                            # D^-1/2 A D^-1/2 = I: breakdown after one step
            else:
                assert got.steps == steps
    if fmt == 0:
        assert fmt_of(op) == 0
    op.free()


@pytest.mark.parametrize("fmt", [9, 10, 11])
def test_bits_on_the_march_formats(fmt):
    """Small 3-D Poisson matrices forced into the brick-march formats, the way tests/test_gpu_cheb.py does it: 9 and 10 run L1
    as the pipelined march kernel with r1[r] prefetched, 11 takes the CSR gather kernel on the same arrays."""
    from pykrylov_amd import tools
    name = "march_const" if fmt == 9 else "march_var"
    A = matrix(name)
    op = device_op(A, True)
    set_format(op, fmt)
    x = np.random.default_rng(3).standard_normal(A.shape[0])
    assert same(op * x, A.matvec(x)) and fmt_of(op) == fmt
    geo = geometry_of(op)
    assert (isinstance(geo[1], tuple) and geo[1][0] == "pencil") == (fmt != 11), geo
    for steps, scaled in ((1, False), (10, False), (2, True), (10, True)):
        got = tools.lanczos(op, steps=steps, scale_diag=scaled)
        check_bits(got, reference(name, steps, scaled, geo), (fmt, steps, scaled))
        assert got.steps == steps and got.info["launches"] <= 2 * steps + 3
    assert fmt_of(op) == fmt
    op.free()


@pytest.mark.parametrize("name", ["poisson2d_100", "1138bus"])
def test_given_start_vector(name):
    from pykrylov_amd import tools
    A = matrix(name)
    op = device_op(A, True)
    geo = geometry_of(op)
    start = np.random.default_rng(8).standard_normal(A.shape[0])
    for scaled in (False, True):
        got = tools.lanczos(op, steps=6, scale_diag=scaled, start=start)
        check_bits(got, reference(name, 6, scaled, geo, start), (name, scaled))
    # the default start vector given explicitly: the same run
    a = tools.lanczos(op, steps=6, start=ref.start_vector(A.shape[0], 1))
    b = tools.lanczos(op, steps=6, seed=1)
    c = tools.lanczos(op, steps=6, seed=2)
    assert same(a.alpha, b.alpha) and same(a.beta, b.beta) and not same(b.alpha, c.alpha)
    op.free()


def test_early_stop_clamping_and_launches():
    from pykrylov_amd import tools
    for name, scaled, steps, m in (("2.5I_5", False, 10, 1), ("2.5I_5", True, 10, 1), ("diagonal", True, 10, 1),
                                   ("poisson1d_3", False, 10, 3), ("poisson1d_3", True, 10, 3), ("one_row", False, 10, 1),
                                   ("one_row", True, 4, 1)):
        A = matrix(name)
        op = device_op(A, True)
        got = tools.lanczos(op, steps=steps, scale_diag=scaled)
        assert got.steps == m and len(got.alpha) == m and len(got.beta) == m + 1, (name, scaled, got.steps)
        check_bits(got, reference(name, steps, scaled, geometry_of(op)), (name, scaled))
        # two launches per step of min(steps, n) enqueued steps, and at most three more
        assert got.info["launches"] <= 2 * min(steps, A.shape[0]) + 3 <= 2 * steps + 3, got.info
        op.free()
    op = device_op(matrix("2.5I_5"), True)
    got = tools.lanczos(op)
    assert got.ritz[0] == got.alpha[0] and abs(got.alpha[0] - 2.5) <= 1e-15 and got.beta[1] <= 2.0 ** -26 * 2.5
    op.free()


@pytest.mark.parametrize("name,scaled", [("poisson2d_100", False), ("poisson2d_100", True), ("1138bus", False), ("1138bus", True)])
def test_chebyshev_on_the_lanczos_interval(name, scaled):
    """`interval` equals the restatement's bounds, `coefficients` those of _cheb_ref for them, `M * x` the reference apply
    with them bit for bit; a given end is kept and only the other one estimated; `interval_source` says which."""
    from pykrylov_amd import tools
    A = matrix(name)
    op = device_op(A, True)
    geo = geometry_of(op)
    want = reference(name, 10, scaled, geo)
    lo, hi = want.bounds
    x = np.random.default_rng(11).standard_normal(A.shape[0])
    for k in (2, 5):
        M = tools.chebyshev(op, degree=k, scale_diag=scaled, interval="lanczos")
        assert M.interval == (lo, hi) and M.interval_source == ("lanczos", "lanczos"), (M.interval, (lo, hi))
        assert M.lanczos.steps == 10 and M.lanczos.bounds == (lo, hi)
        c0, c1, c2 = M.coefficients
        r0, r1, r2 = cheb_ref.coefficients(lo, hi, k)
        assert c0 == r0 and same(c1, r1) and same(c2, r2)
        assert same(M * x, cheb_ref.apply(A, x, k, lo, hi, scaled)), (name, scaled, k)
        M.free()
    # other steps / seed reach the estimate
    w20 = reference(name, 20, scaled, geo)
    M = tools.chebyshev(op, degree=2, scale_diag=scaled, interval="lanczos", steps=20)
    assert M.interval == w20.bounds and M.lanczos.steps == 20
    M.free()
    # a given lmax is kept, only lmin is estimated; and the other way round
    big = 1.5 * hi
    M = tools.chebyshev(op, degree=3, scale_diag=scaled, interval="lanczos", lmax=big)
    assert M.interval == (lo, big) and M.interval_source == ("lanczos", "given")
    assert same(M * x, cheb_ref.apply(A, x, 3, lo, big, scaled))
    M.free()
    small = 0.5 * lo
    M = tools.chebyshev(op, degree=3, scale_diag=scaled, interval="lanczos", lmin=small)
    assert M.interval == (small, hi) and M.interval_source == ("given", "lanczos")
    M.free()
    # the default is what it was
    M = tools.chebyshev(op, degree=3, scale_diag=scaled)
    assert M.interval == cheb_ref.interval(A, scale_diag=scaled) and M.interval_source == ("gershgorin", "gershgorin")
    assert M.lanczos is None
    M.free()
    M = tools.chebyshev(op, degree=3, scale_diag=scaled, lmin=0.5, lmax=3.0)
    assert M.interval_source == ("given", "given")
    M.free()
    M = tools.chebyshev(op, degree=3, scale_diag=scaled, lmax=3.0)
    assert M.interval_source == ("gershgorin", "given") and M.interval == (3.0 / 30.0, 3.0)
    M.free()
    op.free()


def test_chebyshev_degenerate_interval_falls_back_to_the_ratio():
    """A one-eigenvalue Krylov space (2.5 I; the scaled diagonal matrix): bounds[0] is not below bounds[1] (1 - 2^-26), so
    lmin = lmax / ratio."""
    from pykrylov_amd import tools
    for name, scaled, ratio in (("2.5I_5", False, 30.0), ("diagonal", True, 10.0)):
        A = matrix(name)
        op = device_op(A, True)
        want = reference(name, 10, scaled, geometry_of(op))
        lo, hi = want.bounds
        assert want.steps == 1 and not lo < hi * (1.0 - 2.0 ** -26)
        M = tools.chebyshev(op, degree=2, scale_diag=scaled, interval="lanczos", ratio=ratio)
        assert M.interval == (hi / ratio, hi) and M.interval_source == ("lanczos", "lanczos"), M.interval
        x = np.arange(1.0, A.shape[0] + 1.0)
        assert same(M * x, cheb_ref.apply(A, x, 2, hi / ratio, hi, scaled))
        M.free()
        op.free()


def _host_twin(M):
    from pykrylov_amd import LinearOperator
    n = M.shape[0]
    calls = [0]

    def mv(v):
        calls[0] += 1
        return M * v
    return LinearOperator(n, n, matvec=mv, symmetric=True), calls


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("solver", ["minres", "cg"])
def test_solver_with_the_device_object_matches_the_callback_path(solver, scaled):
    """precon=M (interval='lanczos') on the device route against the same object called back on the host: iteration counts,
    histories and x byte-identical."""
    from pykrylov_amd import tools
    A = matrix("poisson2d_100")
    op = device_op(A, True)
    rhs = A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))
    M = tools.chebyshev(op, degree=3, scale_diag=scaled, interval="lanczos")
    host, calls = _host_twin(M)
    k0, h0, x0 = _solve(solver, op, rhs, M)
    k1, h1, x1 = _solve(solver, op, rhs, host)
    assert calls[0] > 1 and k0 > 1
    assert k0 == k1 and same(h0, h1) and same(x0, x1), (solver, scaled, k0, k1)
    M.free()
    op.free()


def _minres_itn(op, rhs, M):
    from pykrylov_amd import Minres
    s = Minres(op)
    s.solve(rhs, precon=M, show=False, check=False, etol=0.0, rtol=1e-10)
    return s.itn, s.istop


def test_it_helps_minres_on_1138bus():
    """1138bus, not scaled, degree 8, MINRES, rtol 1e-10, right-hand side of ones: fewer iterations with the Lanczos interval
    than with the default one (on the CPU, np.dot order: 443 against 649)."""
    from pykrylov_amd import tools
    A = matrix("1138bus")
    op = device_op(A, True)
    rhs = np.ones(A.shape[0])
    M0 = tools.chebyshev(op, degree=8)
    M1 = tools.chebyshev(op, degree=8, interval="lanczos")
    k0, _ = _minres_itn(op, rhs, M0)
    k1, _ = _minres_itn(op, rhs, M1)
    print("MINRES 1138bus, chebyshev(8): %d iterations on the default interval %r, %d on the Lanczos interval %r"
          % (k0, M0.interval, k1, M1.interval))
    assert k1 < k0
    M0.free()
    M1.free()
    op.free()


def test_it_helps_minres_on_poisson2d_100(monkeypatch):
    """poisson2d(100), degree 4: as many iterations as the CPU restatement of MINRES preconditioned by the reference apply on
    the same interval, in the device's summation order -- and at most the 38 of the default interval."""
    from pykrylov_amd import tools
    A = matrix("poisson2d_100")
    n = A.shape[0]
    rhs = np.ones(n)
    op = device_op(A, True)
    M = tools.chebyshev(op, degree=4, interval="lanczos")
    lo, hi = M.interval
    assert (lo, hi) == reference("poisson2d_100", 10, False, geometry_of(op)).bounds
    k, istop = _minres_itn(op, rhs, M)
    monkeypatch.setattr(kr, "_sq", lambda a: a * a)              # the reference's pow(x, 2) is not always x*x
    red = kr.Reductions(gpu_order.GpuDots(n, gpu_order.SPMV_SITES["minres"]))
    want = kr.minres(A, rhs, precon=cheb_ref.HostCheb(A, 4, lo, hi), check=False, etol=0.0, rtol=1e-10, red=red)
    print("MINRES poisson2d_100, chebyshev(4, interval='lanczos') on %r: %d iterations, CPU restatement %d" % ((lo, hi), k, want["itn"]))
    assert k == want["itn"] and istop == want["istop"] == 1
    assert k <= 38
    M.free()
    op.free()


def test_errors():
    from pykrylov_amd import _lib, tools
    A = matrix("poisson2d_12")
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    diag = rows == A.indices
    # a negative diagonal entry in row 7: D^-1/2 does not exist
    neg = device_op(csr_ref.from_coo(rows, A.indices, np.where(diag & (rows == 7), -4.0, A.data), A.shape), True)
    with pytest.raises(_lib.MkError, match="row 7 has no positive diagonal"):
        tools.lanczos(neg, scale_diag=True)
    with pytest.raises(_lib.MkError, match="row 7 has no positive diagonal"):
        tools.chebyshev(neg, scale_diag=True, interval="lanczos")
    assert tools.lanczos(neg).steps == 10                        # unscaled: no diagonal is needed ...
    with pytest.raises(ValueError, match="Ritz value"):         # ... but this matrix is indefinite
        tools.chebyshev(neg, interval="lanczos", steps=40)
    # a missing diagonal in row 5 and a stored zero in row 3: the smallest such row is named
    keep = ~((rows == 5) & (A.indices == 5))
    data = np.where((rows == 3) & (A.indices == 3), 0.0, A.data)
    B = device_op(csr_ref.from_coo(rows[keep], A.indices[keep], data[keep], A.shape), True)
    with pytest.raises(_lib.MkError, match="row 3 has no positive diagonal"):
        tools.lanczos(B, scale_diag=True)
    # a matrix holding an inf: the run stops on the device, the call returns with an error that gives the step
    bad = A.data.copy()
    bad[10] = np.inf
    I = device_op(csr_ref.from_coo(rows, A.indices, bad, A.shape), True)
    for scaled in (False, True):
        with pytest.raises(_lib.MkError, match="step 1 is not finite"):
            tools.lanczos(I, scale_diag=scaled)
    good = tools.lanczos(device_op(A, True), steps=3)           # the library goes on working
    assert good.steps == 3
    S = B + B                                                   # a composite: no arrays of its own
    with pytest.raises((_lib.MkError, TypeError), match="to_csr_arrays"):
        tools.lanczos(S)
    B.local_size = A.shape[0] // 2                              # what the package recognises a row-partitioned operator by
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        tools.lanczos(B)
    del B.local_size
    with pytest.raises(ValueError, match="symmetric"):
        tools.lanczos(device_op(A, False))
    lib = _lib.init()
    al, be = (ctypes.c_double * 4)(), (ctypes.c_double * 5)()
    assert lib.mk_csr_lanczos(B.handle, 0, 0, 1, None, al, be, None, 0) == -2        # MK_ERR_ARG: steps < 1
    assert lib.mk_csr_lanczos(B.handle, 4, 0, 1, 8, al, be, None, 0) == -2           # a start vector that is not 16-byte aligned
    for o in (S, B, I, neg):
        o.free()
