"""Every fused epilogue of the product kernel in every storage format 0 .. 8 and across the launches of a column-blocked product.
mk_spmv_kernel is instantiated once per (epilogue type, kernel variant), and each variant implements the epilogue contract --
`xin`, `row`, `row_x`, `pre`, the fused partial sums, the carry across column-block launches -- in its own file, so one pairing
can break while every other stays right.  Here the epilogues of the Lanczos estimate (LzEpi), of the Chebyshev preconditioner
(MkChebEpi) and filter (MkChebFiltEpi), of the thick-restart SVD (SvEpiU, SvEpiPlain) and of the least-squares loops (EpiU, EpiV)
run on the matrices of tests/_storage_matrices.py, forced into each storage, and are compared bit for bit with their NumPy
restatements in the operator's own launch geometry -- also on matrices with empty rows and all-empty tiles, where an epilogue
must still run for a row without entries, and on matrices with rows that lack the diagonal entry `row_x` takes x[r] from.  The
older loops run here on the matrices with empty rows only: they are run through the storages by
tests/test_gpu_nontemporal.py, the AMG epilogue by tests/test_gpu_amg.py
(_storage_matrices.EPILOGUES has the whole table).  Every case asserts its storage before and after the run: a request that
degrades is a failure."""
import numpy as np
import pytest

from oracle import gpu_order, krylov_ref as kr, lls_ref
from tests import _cheb_ref as cheb_ref, _chebfilt_ref as filt_ref, _lanczos_ref as lanczos_ref, _storage_matrices as sm
from tests import _trsvd_ref as trsvd_ref
from test_gpu_formats import blocked, colblocks, fmt_info
from test_gpu_ilu import device_op, same
from test_gpu_lanczos import check_bits as check_lanczos, geometry_of, set_format
from test_gpu_lls import run_device, run_oracle
from test_gpu_nontemporal import BUDGET, LOOPS, run_loop, run_oracle as run_loop_oracle, same_run
from test_gpu_trsvd import check_bits as check_svd

pytestmark = pytest.mark.gpu

CB = "cb"                                                    # the column-blocked matrix: storage 0 in three launches
SQUARE = sm.SQUARE + ((CB, "colblocks", "plain"),)
SQUARE_IDS = ["%s-%s" % c[:2] for c in SQUARE]
RECT_IDS = ["%d-%s" % (c[0], c[2]) for c in sm.RECT]
SQUARE_EPILOGUES = ("lanczos", "chebyshev", "filter")
RECT_EPILOGUES = ("svd", "lls")
REACHED = {e: set() for e in SQUARE_EPILOGUES + RECT_EPILOGUES}
_REF = {}


def cached(key, make):
    """A restatement's result, computed once per (matrix, geometry, arguments)."""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def check_storage(op, fmt):
    if fmt == CB:
        assert fmt_info(op)["fmt"] == 0 and colblocks(op) >= 3, (fmt_info(op), colblocks(op))
    else:
        assert fmt_info(op)["fmt"] == fmt and colblocks(op) == 0, (fmt_info(op), fmt)


def square_op(fmt, name):
    op = device_op(sm.mat(name), True)
    set_format(op, 0 if fmt == CB else fmt)
    if fmt == CB:
        blocked(op, sm.COLBLOCK_KB)
    check_storage(op, fmt)
    return op


def rect_op(fmt, fmt_t, name):
    """A and its transposed copy (a matrix of its own), each forced into its storage."""
    op = device_op(sm.mat(name), False)
    set_format(op, fmt)
    set_format(op.T, fmt_t)
    check_rect(op, fmt, fmt_t)
    return op


def check_rect(op, fmt, fmt_t):
    assert fmt_info(op)["fmt"] == fmt and fmt_info(op.T)["fmt"] == fmt_t, (fmt_info(op), fmt_info(op.T), fmt, fmt_t)


# ------------------------------------------------------------------------------------------------ Lanczos (LzEpi)
@pytest.mark.parametrize("fmt,name,kind", SQUARE, ids=SQUARE_IDS)
def test_lanczos(fmt, name, kind):
    """LzEpi scales every gathered entry by 1 / beta (`xin`), takes xin(y[i]) from the kernel (`row_x`) and fuses <v, A v>:
    alpha, beta and the Ritz values of 1, 2 and 10 steps, scaled by the diagonal where every row has a positive one, and of 10
    steps from a start vector holding signed zeros and denormals (the scaled gather then multiplies pads and denormals)."""
    from pykrylov_amd import tools
    A = sm.mat(name)
    n = A.shape[0]
    op = square_op(fmt, name)
    geo = geometry_of(op)
    runs = [(s, sc, None) for sc in ((False, True) if kind == "plain" else (False,)) for s in (1, 2, 10)]
    runs += [(10, sc, sm.denormal_start(n)) for sc in ((False, True) if kind == "plain" else (False,))]
    for steps, scaled, start in runs:
        want = cached(("lanczos", name, geo, steps, scaled, start is None),
                      lambda: lanczos_ref.lanczos(A, steps=steps, scale_diag=scaled, seed=1, start=start,
                                                  dots=lanczos_ref.GpuDots(n, geo)))
        got = tools.lanczos(op, steps=steps, scale_diag=scaled, start=start)
        check_lanczos(got, want, (fmt, name, steps, scaled, start is None))
        assert got.steps == steps, (fmt, name, steps, scaled, got.steps)
    check_storage(op, fmt)
    REACHED["lanczos"].add(fmt)
    op.free()


# ------------------------------------------------------------------------------------------------ Chebyshev (MkChebEpi)
@pytest.mark.parametrize("fmt,name,kind", SQUARE, ids=SQUARE_IDS)
def test_chebyshev_preconditioner(fmt, name, kind):
    """`M * v` of tools.chebyshev(degree=4) on the Gershgorin interval, with and (where every row has a positive diagonal
    entry) without the diagonal scaling."""
    from pykrylov_amd import tools
    A = sm.mat(name)
    op = square_op(fmt, name)
    v = np.random.default_rng(11).standard_normal(A.shape[0])
    for scaled in ((False, True) if kind == "plain" else (False,)):
        lmin, lmax = cheb_ref.interval(A, scale_diag=scaled)
        want = cached(("cheb", name, scaled), lambda: cheb_ref.apply(A, v, 4, lmin, lmax, scaled))
        M = tools.chebyshev(op, degree=4, scale_diag=scaled)
        assert M.interval == (lmin, lmax), (M.interval, lmin, lmax)
        got = M * v
        assert np.isfinite(want).all() and same(got, want), (fmt, name, scaled)
        M.free()
    check_storage(op, fmt)
    REACHED["chebyshev"].add(fmt)
    op.free()


# ------------------------------------------------------------------------------------------------ filter (MkChebFiltEpi)
@pytest.mark.parametrize("fmt,name,kind", SQUARE, ids=SQUARE_IDS)
def test_chebyshev_filter(fmt, name, kind):
    """`F * v` of the degree-8 filter that damps the upper 70 % of the Gershgorin interval [a, b], reference point a."""
    from pykrylov_amd import tools
    A = sm.mat(name)
    op = square_op(fmt, name)
    v = np.random.default_rng(17).standard_normal(A.shape[0])
    a, b = cached(("gershgorin", name), lambda: filt_ref.interval(A))
    cut = a + 0.3 * (b - a)
    want = cached(("filter", name), lambda: filt_ref.apply(A, v, 8, cut, b, a))
    F = tools.cheb_filter(op, degree=8, interval=(cut, None), ref=a)
    assert F.interval == (cut, b) and F.ref == a, (F.interval, cut, b)
    got = F * v
    assert np.isfinite(want).all() and same(got, want), (fmt, name)
    F.free()
    check_storage(op, fmt)
    REACHED["filter"].add(fmt)
    op.free()


# ------------------------------------------------------------------------------------------------ SVD (SvEpiU, SvEpiPlain)
@pytest.mark.parametrize("reorth", ["full", "one-sided"])
@pytest.mark.parametrize("fmt,fmt_t,name", sm.RECT, ids=RECT_IDS)
def test_svd(fmt, fmt_t, name, reorth):
    """Two triplets, a basis of nine, 40 products: the one-sided mode fuses <u, u> into A's product and subtracts beta * prev
    in the epilogue; A' u runs in the transposed copy's storage."""
    from pykrylov_amd import ThickRestartSVD
    A = sm.mat(name)
    assert A.shape[0] > A.shape[1]
    op = rect_op(fmt, fmt_t, name)
    kw = dict(ncv=9, matvec_max=40, reorth=reorth)
    geo = gpu_order.launch_geometry(op)
    want = cached(("svd", name, repr(geo), reorth),
                  lambda: trsvd_ref.trsvd(A, 2, dots=gpu_order.GpuDots(A.shape[0], [trsvd_ref.SITE_UU], geometry=geo), **kw))
    s = ThickRestartSVD(op, reltol=1e-10, abstol=0.0)
    s.solve(2, **kw)
    check_svd(s, want, (fmt, name, reorth))
    assert s.nMatvec > 30, s.nMatvec                         # (the run did not end early)
    check_rect(op, fmt, fmt_t)
    REACHED["svd"].add((fmt, fmt_t))
    op.free()


# ------------------------------------------------------------------------------------------------ least squares (EpiU, EpiV ...)
class Dots(object):
    """The inner products of the least-squares loops on the device: those fused into a product of A (`.beta`, rows = m) in the
    launch geometry of A, those fused into a product of A' (`.alpha`, `.alpha0`, rows = n) in the transposed copy's."""

    def __init__(self, shape, geo, geo_t):
        self.tiles = [(k + gpu_order.BLOCK - 1) // gpu_order.BLOCK for k in shape]
        self.geo, self.geo_t = geo, geo_t

    def __call__(self, a, b, site):
        if site.endswith(".beta"):
            return gpu_order.total(gpu_order.spmv_partials(a, b, self.tiles[0], *self.geo))
        if site.endswith(".alpha") or site.endswith(".alpha0"):
            return gpu_order.total(gpu_order.spmv_partials(a, b, self.tiles[1], *self.geo_t))
        return gpu_order.stream_dot(a, b)


@pytest.mark.parametrize("solver,damp", sm.LLS_RUNS, ids=["%s-damp%g" % c for c in sm.LLS_RUNS])
@pytest.mark.parametrize("fmt,fmt_t,name", sm.RECT, ids=RECT_IDS)
def test_least_squares(fmt, fmt_t, name, solver, damp, monkeypatch):
    """25 passes of LSQR, LSMR, CRAIG and CRAIG-MR (etol = 0: none ends on its error estimate): every scalar and x, and r of
    CRAIG, against the oracle."""
    monkeypatch.setattr(lls_ref, "_sq", lambda a: a * a)
    A = sm.mat(name)
    b = sm.lls_rhs(A, solver)
    op = rect_op(fmt, fmt_t, name)
    geo, geo_t = gpu_order.launch_geometry(op), gpu_order.launch_geometry(op.T)
    got, s = run_device(solver, op, b, damp, 0.0, **sm.lls_arguments(solver))
    ref = cached(("lls", name, repr(geo), repr(geo_t), solver, damp),
                 lambda: run_oracle(solver, A, b, damp, 0.0, red=kr.Reductions(Dots(A.shape, geo, geo_t)),
                                    **sm.lls_arguments(solver)))
    assert (got["istop"], got["itn"]) == (ref["istop"], ref["itn"]) and got["itn"] == 25, (got["istop"], got["itn"], ref["itn"])
    assert same(got["x"], ref["x"]), (fmt, name, solver, damp)
    for k, v in got.items():
        if k not in ("x", "r", "istop", "itn"):
            assert same(v, ref[k]), (fmt, name, solver, damp, k, v, ref[k])
    if solver == "craig":
        assert same(got["r"], ref["r"])
    check_rect(op, fmt, fmt_t)
    REACHED["lls"].add((fmt, fmt_t))
    op.free()


# ------------------------------------------------------------------------------------------------ the older loops, empty rows
HOLES = [c[:2] for c in sm.SQUARE if c[2] == "holes"]


@pytest.mark.parametrize("solver", LOOPS)
@pytest.mark.parametrize("fmt,name", HOLES, ids=["%d-%s" % c for c in HOLES])
def test_older_loops_on_empty_rows_and_tiles(fmt, name, solver, monkeypatch):
    """BiCGSTAB, CGS, TFQMR, MINRES and SYMMLQ on the matrices with empty rows and all-empty tiles (storages 0 .. 3; the system
    is consistent and definite on the rows that have entries): an epilogue runs for a row without entries too -- MINRES'
    t[i] = 0 - c r1[i].  The right-hand side A 1 is zero in the empty rows, so the loops' vectors stay zero there: this case
    checks the fused sums and the rows beside the empty ones; the stale-vector defect of a kernel that skips a tile without
    nonzeros shows in test_lanczos, test_chebyshev_preconditioner and test_chebyshev_filter, whose vectors are not zero
    there (tried with such a storage-3 kernel: those six cases fail, these pass)."""
    monkeypatch.setattr(kr, "_sq", lambda a: a * a)
    A = sm.mat(name)
    op = square_op(fmt, name)
    rhs = A.matvec(np.ones(A.shape[0]))
    got = run_loop(solver, op, rhs)
    assert BUDGET - 2 <= got[0] <= BUDGET + 2 and np.isfinite(got[2]).all(), (solver, fmt, name, got[0])
    want = cached(("loop", name, geometry_of(op), solver), lambda: run_loop_oracle(solver, A, rhs, op))
    assert same_run(got, want), (solver, fmt, name)
    check_storage(op, fmt)
    op.free()


# ------------------------------------------------------------------------------------------------ what was reached
def test_every_storage_was_reached():
    """Every storage 0 .. 8 and the column blocks for the square epilogues -- a case the tests above have not run is built now,
    which asserts its storage --, and which storages the rectangular epilogues ran in, for A and for the transposed copy."""
    for fmt, name, _ in SQUARE:
        if not all(fmt in REACHED[e] for e in SQUARE_EPILOGUES):
            square_op(fmt, name).free()
            for e in SQUARE_EPILOGUES:
                REACHED[e].add(fmt)
    for fmt, fmt_t, name in sm.RECT:
        if not all((fmt, fmt_t) in REACHED[e] for e in RECT_EPILOGUES):
            rect_op(fmt, fmt_t, name).free()
            for e in RECT_EPILOGUES:
                REACHED[e].add((fmt, fmt_t))
    for e in SQUARE_EPILOGUES:
        print("%-10s storages %s" % (e, sorted(REACHED[e], key=str)))
        assert REACHED[e] == set(range(9)) | {CB}, (e, REACHED[e])
    for e in RECT_EPILOGUES:
        print("%-10s (storage of A, of A') %s" % (e, sorted(REACHED[e])))
        assert {f for f, _ in REACHED[e]} >= sm.RECT_STORAGES <= {f for _, f in REACHED[e]}, (e, REACHED[e])
