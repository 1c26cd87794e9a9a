"""The non-temporal (NT) code outside CG.  Beyond 256 MiB per vector `mk_stream_nt` (csrc/mk_device.h) switches a product to
the NT kernel variants (6 = MK_FMT_PAT_STREAM_NT for storage 5, 9 = MK_FMT_WIDE_NT for storage 6 and 7, the NT loads of the
march kernels 11 .. 16) and the epilogues of BiCGSTAB, CGS, MINRES, SYMMLQ, the least-squares loops and the Chebyshev steps to
the inline-asm non-temporal store of `mk_store_stream` (csrc/mk_solver.h).  The flag is launch uniform and changes cache policy
only, so it is forced here on small matrices (`mk_csr_set_tile_order(handle, -1, 0, 0, 1)`) and everything must keep the bits of
the same run with the flag off -- and those of the oracle.  Every case asserts the storage format and the flag it ran with."""
import numpy as np
import pytest

from oracle import csr_ref, gpu_order, krylov_ref as kr, lls_ref
from tests import _cheb_ref as cheb_ref, _storage_matrices as sm
from test_gpu_formats import MATS, banded, blocked, colblocks, fmt_info
from test_gpu_lls import run_device
from test_gpu_tile_order import get_order, set_order
from test_gpu_wide import fixed_width_random_band

pytestmark = pytest.mark.gpu


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).tobytes()


def symmetrised(A):
    """(A + A') / 2 with the sparsity of both."""
    n = A.shape[0]
    T = A.transpose()
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    trows = np.repeat(np.arange(n), np.diff(T.indptr))
    return csr_ref.from_coo(np.concatenate([rows, trows]), np.concatenate([A.indices, T.indices]),
                            np.concatenate([0.5 * A.data, 0.5 * T.data]), (n, n))


def symmetric_slots(n, k, block, rng):
    """A symmetric matrix without row patterns whose rows all have about 2 k + 1 entries (the symmetrised twin of
    fixed_width_random_band has rows of 50 entries beside rows of 16 and is refused by the slot format): k times, the rows of
    every block of `block` rows are matched by a random permutation p, and the entries (r, p(r)) and (p(r), r) share a value.
    The diagonal, 2 sqrt(2 k) + 1 + [0, 1), keeps the matrix definite but not so well conditioned that 30 products solve it."""
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [2.0 * np.sqrt(2.0 * k) + 1.0 + rng.random(n)]
    for _ in range(k):
        p = np.arange(n)
        for lo in range(0, n, block):
            hi = min(n, lo + block)
            p[lo:hi] = lo + rng.permutation(hi - lo)
        w = rng.standard_normal(n)
        r = np.flatnonzero(p != np.arange(n))
        rows += [r, p[r]]
        cols += [p[r], r]
        vals += [w[r], w[r]]
    return csr_ref.from_coo(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), (n, n))


def with_diagonal_shifted(A, by):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return csr_ref.RefCsr(A.indptr, A.indices, np.where(A.indices == rows, A.data + by, A.data), A.shape)


def _band(offsets):
    n = 20000                                                # 78 tiles and a last one of 32 rows
    r, c, v = banded(n, offsets, np.random.default_rng(21))
    return csr_ref.from_coo(r, c, v, (n, n))


def _rows_without_a_diagonal_entry(every_seventh_has_one):
    """Path graph with all-distinct weights plus diagonal entries on every seventh row only (the structure of
    test_gpu_formats.py::test_pattern_format_rows_without_a_diagonal_entry) or on all rows but every seventh."""
    n = 6001
    rng = np.random.default_rng(4)
    i = np.arange(n - 1)
    dg = np.arange(0, n, 7) if every_seventh_has_one else np.arange(n)[np.arange(n) % 7 != 0]
    w = rng.standard_normal(n - 1)
    return csr_ref.from_coo(np.concatenate([i, i + 1, dg]), np.concatenate([i + 1, i, dg]),
                            np.concatenate([w, w, 3.0 + rng.random(len(dg))]), (n, n))


def _rect_wide():
    """The 4000 x 3600 matrix of test_gpu_wide.py::test_lsqr_on_a_wide_rectangular_operator."""
    S = fixed_width_random_band(4000, 14, 700, np.random.default_rng(18))
    keep = S.indices < 3600
    rows = np.repeat(np.arange(4000), np.diff(S.indptr))
    return csr_ref.from_coo(rows[keep], S.indices[keep], S.data[keep], (4000, 3600))


def _tall_band():
    """A band matrix with all-distinct values less the last 10 % of its columns: the rows below them are short or empty."""
    n = 9000
    r, c, v = banded(n, (-300, -1, 0, 1, 300), np.random.default_rng(6), ncols=8100)
    return csr_ref.from_coo(r, c, v, (n, 8100))


BUILDERS = {
    "varcoef": lambda: csr_ref.poisson3d_varcoef(64, 10, 5),                 # 12 tiles and a half
    "varcoef_small": lambda: csr_ref.poisson3d_varcoef(33, 9, 4),            # lines that divide no tile
    "varcoef_b": lambda: csr_ref.poisson3d_varcoef(64, 10, 5, seed=8),
    "band_even": lambda: _band((-300, -1, 1, 300)),                           # tiles of width 4: pairs only
    "band_odd": lambda: _band((-300, -1, 0, 1, 300)),                         # width 5: pairs and a last single column
    "slots": lambda: fixed_width_random_band(7000, 16, 900, np.random.default_rng(16)),
    # (the same with diagonal entries of 6 .. 7 instead of 16 .. 17: the loops do not converge within their budget)
    "slots_slow": lambda: with_diagonal_shifted(mat("slots"), -10.0),
    "slots_sym": lambda: symmetric_slots(7000, 8, 512, np.random.default_rng(3)),
    "s27_var_ragged": lambda: csr_ref.stencil27(64, 10, 5, seed=7),           # 12 tiles and a half
    "s27_var_cube": lambda: csr_ref.stencil27(40, 40, 12, seed=7),
    "s27_var": lambda: csr_ref.stencil27(256, 6, 5, seed=7),
    "s27_var_b": lambda: csr_ref.stencil27(256, 6, 5, seed=9),
    "s27_const": lambda: csr_ref.stencil27(256, 6, 5, seed=0),
    "poisson2d": lambda: csr_ref.poisson2d(150),
    "banded_dict": lambda: MATS["banded_dict"][0],
    "banded_manyvalues": lambda: MATS["banded_manyvalues"][0],
    "scattered": lambda: csr_ref.random_diagdom(5003),
    "scattered_sym": lambda: symmetrised(mat("scattered")),
    "bricks": lambda: csr_ref.poisson3d(128, 8, 9),
    "bricks_var": lambda: csr_ref.poisson3d_varcoef(128, 8, 9),
    "general": lambda: csr_ref.poisson3d(101, 9, 11),
    "general_var": lambda: csr_ref.poisson3d_varcoef(101, 9, 11, seed=3),
    "diagonal_on_every_7th_row": lambda: _rows_without_a_diagonal_entry(True),
    "no_diagonal_on_every_7th_row": lambda: _rows_without_a_diagonal_entry(False),
    "rect_wide": _rect_wide,
    "tall_band": _tall_band,
    "big_scattered": lambda: csr_ref.random_diagdom(700001, seed=4),
    "band_sym_distinct": lambda: sm.mat("band_distinct"),                      # symmetric, 35 tiles and a last one of 41 rows
    "band_sym_dict": lambda: sm.mat("band_dict"),
}
_MATS = {}


def mat(name):
    if name not in _MATS:
        _MATS[name] = BUILDERS[name]()
    return _MATS[name]


def forced(A, fmt, nt, symmetric=False):
    """The operator in storage `fmt` with the NT flag `nt`; both are asserted (a request that degrades is a failure)."""
    from pykrylov_amd import CsrOperator, _lib
    op = CsrOperator(A.indptr, A.indices, A.data, A.shape, symmetric=symmetric)
    _lib.check(_lib.init().mk_csr_set_format(op.handle, fmt))
    set_order(op, -1, 0, 0, nt)
    check(op, fmt, nt)
    return op


def check(op, fmt, nt):
    assert fmt_info(op)["fmt"] == fmt, (fmt_info(op), fmt)
    assert get_order(op)[3] == nt, (get_order(op), nt)


def pair(name, fmt, symmetric=False):
    """The same arrays twice, in the same storage: NT off and on."""
    A = mat(name)
    return A, forced(A, fmt, 0, symmetric), forced(A, fmt, 1, symmetric)


def xs(n, seed=3):
    rng = np.random.default_rng(seed)
    return (np.ones(n), rng.standard_normal(n), 1e200 * rng.standard_normal(n))


def same_ints(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64))


# ------------------------------------------------------------------------------------------------ 1. products
# (storage, matrix): several tiles and a ragged last one wherever the format allows it
PRODUCTS = [(5, "varcoef"), (5, "varcoef_small"), (5, "band_even"), (5, "band_odd"), (6, "slots"), (6, "slots_sym"),
            (7, "s27_var_cube"), (7, "s27_var_ragged"), (7, "s27_var"), (8, "s27_const"), (4, "poisson2d"),
            (2, "banded_dict"), (1, "banded_manyvalues"), (0, "scattered"), (3, "scattered"), (9, "bricks"),
            (10, "bricks_var"), (11, "bricks_var"), (9, "general"), (10, "general_var"), (11, "general_var")]


@pytest.mark.parametrize("fmt,name", PRODUCTS, ids=["%d-%s" % c for c in PRODUCTS])
def test_products_keep_their_bits(fmt, name):
    """`op * x`, `op.T * u` and two row programs with the flag on: the oracle's scalar loop, compared as integers."""
    from pykrylov_amd import DiagonalOperator, IdentityOperator
    A, op0, op1 = pair(name, fmt)
    m, n = A.shape
    for op, nt in ((op0, 0), (op1, 1)):
        set_order(op.T, -1, 0, 0, nt)                        # (the transposed copy is a matrix of its own)
        assert get_order(op.T)[3] == nt
        for x, u in zip(xs(n), xs(m, seed=4)):
            assert same_ints(op * x, A.matvec(x)), (fmt, name, nt)
            assert same_ints(op.T * u, A.rmatvec(u)), (fmt, name, nt)
        check(op, fmt, nt)
    rng = np.random.default_rng(5)
    d, x = rng.standard_normal(n), rng.standard_normal(n)
    c1 = 2.5 * op1 + DiagonalOperator(d)                     # composed operators read their base matrix's flag
    c2 = op1 - 1.5 * IdentityOperator(n)
    assert get_order(c1)[3] == 1 and get_order(c2)[3] == 1
    assert same_ints(c1 * x, 2.5 * A.matvec(x) + d * x)
    assert same_ints(c2 * x, A.matvec(x) - 1.5 * x)
    check(op1, fmt, 1)
    op0.free()
    op1.free()


SUMS = [(5, "varcoef", "varcoef_b"), (6, "slots_slow", "slots_sym"), (7, "s27_var", "s27_var_b")]


@pytest.mark.parametrize("fmt,a,b", SUMS, ids=["%d-%s-%s" % c for c in SUMS])
def test_device_sums_and_products_of_two_nt_operators(fmt, a, b):
    """`opA + opB` and `opA * opB` on the device.  The automatic rule of mk_stream_nt leaves composites out; an explicit
    request on one counts, and it is what the fused epilogue of a solver on the sum stores with."""
    import pykrylov_amd
    A, B = mat(a), mat(b)
    n = A.shape[0]
    opA, opB = forced(A, fmt, 1), forced(B, fmt, 1)
    x = np.random.default_rng(7).standard_normal(n)
    S, P = opA + opB, opA * opB
    assert type(S).__name__ == type(P).__name__ == "_PairCsrOperator"
    assert get_order(S)[3] == 0 and get_order(P)[3] == 0     # (small composites: off by default)
    assert same_ints(S * x, A.matvec(x) + B.matvec(x))
    assert same_ints(P * x, A.matvec(B.matvec(x)))
    rhs = A.matvec(np.ones(n)) + B.matvec(np.ones(n))
    runs = []
    for nt in (0, 1):
        set_order(S, -1, 0, 0, nt)
        assert get_order(S)[3] == nt
        assert same_ints(S * x, A.matvec(x) + B.matvec(x))
        s = pykrylov_amd.BiCGSTAB(S, abstol=0.0, reltol=1e-15)
        s.solve(rhs, matvec_max=30)
        runs.append((s.nMatvec, bits(s.residNorm), bits(s.x)))
    assert runs[0][0] >= 28 and runs[0] == runs[1]
    set_order(P, -1, 0, 0, 1)
    assert get_order(P)[3] == 1
    assert same_ints(P * x, A.matvec(B.matvec(x)))
    check(opA, fmt, 1)
    check(opB, fmt, 1)
    for o in (S, P, opA, opB):
        o.free()


def test_column_blocks():
    """Scattered columns and an x of 5.6 MB, cut into three column blocks: products only."""
    A = mat("big_scattered")
    n = A.shape[0]
    want = [A.matvec(x) for x in xs(n, seed=8)]
    for nt in (0, 1):
        op = blocked(forced(A, 0, nt))
        assert colblocks(op) == 3
        check(op, 0, nt)
        for x, y in zip(xs(n, seed=8), want):
            assert same_ints(op * x, y), nt
        op.free()


# ------------------------------------------------------------------------------------------------ 2. the loops
LOOPS = ("bicgstab", "cgs", "tfqmr", "minres", "symmlq")
SYMMETRIC_LOOPS = ("minres", "symmlq")
# storage -> (matrix for the three nonsymmetric loops, matrix for MINRES and SYMMLQ)
LOOP_MATRICES = {5: ("varcoef", "varcoef"), 6: ("slots_slow", "slots_sym"), 7: ("s27_var", "s27_var"),
                 8: ("s27_const", "s27_const"), 4: ("poisson2d", "poisson2d"), 0: ("scattered", "scattered_sym"),
                 3: ("scattered", "scattered_sym"), 9: ("bricks", "bricks"), 10: ("bricks_var", "bricks_var"),
                 # (storage 1 and 2 have no NT kernel variant, but the epilogue's store has its NT branch there too)
                 1: ("band_sym_distinct", "band_sym_distinct"), 2: ("band_sym_dict", "band_sym_dict")}
BUDGET = 30                                                  # products: no matrix here is solved to 1e-15 by then


def run_loop(solver, op, rhs, precon=None, budget=BUDGET):
    """(count, history, x) of a run that ends on its budget of products."""
    import pykrylov_amd
    if solver == "minres":
        s = pykrylov_amd.Minres(op)
        s.solve(rhs, precon=precon, show=False, check=False, etol=0.0, rtol=1e-15, itnlim=budget)
        return s.itn, np.array(s.residHistory), s.x
    if solver == "symmlq":
        s = pykrylov_amd.Symmlq(op, precon=precon)
        s.solve(rhs, matvec_max=budget, rtol=1e-15)
        return s.nMatvec, np.array([s.residNorm]), s.x
    cls = {"bicgstab": pykrylov_amd.BiCGSTAB, "cgs": pykrylov_amd.CGS, "tfqmr": pykrylov_amd.TFQMR}[solver]
    s = cls(op, precon=precon, abstol=0.0, reltol=1e-15)
    s.solve(rhs, matvec_max=budget)
    return s.nMatvec, np.array([s.residNorm]), s.x               # (these loops keep no history)


def run_oracle(solver, A, rhs, op, budget=BUDGET):
    red = kr.Reductions(gpu_order.GpuDots(A.shape[0], gpu_order.SPMV_SITES[solver], gpu_order.launch_geometry(op)))
    if solver == "minres":
        ref = kr.minres(A, rhs, check=False, etol=0.0, rtol=1e-15, itnlim=budget, red=red)
        return ref["itn"], ref["residHistory"], ref["x"]
    if solver == "symmlq":
        ref = kr.symmlq(A, rhs, matvec_max=budget, rtol=1e-15, red=red)
    else:
        ref = getattr(kr, solver)(A, rhs, abstol=0.0, reltol=1e-15, matvec_max=budget, red=red)
    return ref["nMatvec"], np.array([ref["residNorm"]]), ref["x"]


def same_run(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and bits(a[1]) == bits(b[1]) \
        and bits(a[2]) == bits(b[2])


@pytest.mark.parametrize("fmt", sorted(LOOP_MATRICES))
@pytest.mark.parametrize("solver", LOOPS)
def test_every_loop_that_carries_the_flag(solver, fmt, monkeypatch):
    """Product count, history (MINRES; the last residual norm elsewhere) and iterate with the flag on equal those with it
    off -- and those of the oracle in the operator's launch geometry, in every storage: a defect of an epilogue in one kernel
    variant that is the same with and without the flag does not pass.  TFQMR has no such store, but its products switch
    kernel variant like the others'."""
    monkeypatch.setattr(kr, "_sq", lambda a: a * a)
    sym = solver in SYMMETRIC_LOOPS
    A, op0, op1 = pair(LOOP_MATRICES[fmt][1 if sym else 0], fmt, symmetric=sym)
    rhs = A.matvec(np.ones(A.shape[0]))
    r0, r1 = run_loop(solver, op0, rhs), run_loop(solver, op1, rhs)
    check(op0, fmt, 0)
    check(op1, fmt, 1)
    assert BUDGET - 2 <= r0[0] <= BUDGET + 2 and np.isfinite(r0[2]).all(), (solver, fmt, r0[0])
    assert same_run(r0, r1), (solver, fmt, r0[0], r1[0])
    assert same_run(r1, run_oracle(solver, A, rhs, op1)), (solver, fmt)
    op0.free()
    op1.free()


# ------------------------------------------------------------------------------------------------ 3. MINRES' row_x hook
@pytest.mark.parametrize("fmt,name", [(5, "no_diagonal_on_every_7th_row"), (7, "no_diagonal_on_every_7th_row"),
                                      (6, "diagonal_on_every_7th_row")])
def test_minres_row_x_hook(fmt, name, monkeypatch):
    """MINRES takes s * y[i] from the diagonal entry's LDS slot; a row without a diagonal entry loads it.  Both kinds of
    rows store v and t through the NT branch.  (The pattern formats pad by at most 12.5 %: storage 5 and 7 take the matrix
    in which every seventh row lacks the diagonal entry; the one in which only every seventh row has it -- the structure of
    test_gpu_formats.py::test_pattern_format_rows_without_a_diagonal_entry with all-distinct values -- gets the slot format,
    which has no diagonal cell and loads y[i] in every row.)"""
    monkeypatch.setattr(kr, "_sq", lambda a: a * a)
    A, op0, op1 = pair(name, fmt, symmetric=True)
    rhs = A.matvec(np.linspace(1.0, 2.0, A.shape[0]))
    r0, r1 = run_loop("minres", op0, rhs, budget=60), run_loop("minres", op1, rhs, budget=60)
    check(op0, fmt, 0)
    check(op1, fmt, 1)
    assert r0[0] == 60 and same_run(r0, r1)
    assert same_run(r1, run_oracle("minres", A, rhs, op1, budget=60))
    op0.free()
    op1.free()


# ------------------------------------------------------------------------------------------------ 4. least squares
LLS = ("lsqr", "lsmr", "craig", "craigmr")
LLS_MATRICES = {"rect_wide": 6, "tall_band": 5}


def lls_record(solver, A, fmt, nt, b):
    op = forced(A, fmt, nt)
    set_order(op.T, -1, 0, 0, nt)                            # (a matrix of its own: the call is not refused)
    assert get_order(op.T)[3] == nt
    got, s = run_device(solver, op, b, 0.0, 0.0, itnlim=25)
    check(op, fmt, nt)
    assert get_order(op.T)[3] == nt
    op.free()
    return got


@pytest.mark.parametrize("name", sorted(LLS_MATRICES))
@pytest.mark.parametrize("solver", LLS)
def test_least_squares_loops(solver, name):
    """EpiU stores u (and Mu) through the NT branch; A' u runs the NT variant of the transposed copy's kernel."""
    A = mat(name)
    b = A.matvec(np.ones(A.shape[1]))                        # consistent (CRAIG needs that)
    if solver in ("lsqr", "lsmr"):
        b = b + 1e-3 * np.random.default_rng(18).standard_normal(A.shape[0])
    g0, g1 = (lls_record(solver, A, LLS_MATRICES[name], nt, b) for nt in (0, 1))
    assert g0["itn"] == g1["itn"] == 25 and g0["istop"] == g1["istop"]
    assert sorted(g0) == sorted(g1)
    for k in g0:
        assert bits(g0[k]) == bits(g1[k]), (solver, name, k)
    if solver == "lsqr" and name == "rect_wide":                 # as test_gpu_wide.py::test_lsqr_on_a_wide_rectangular_operator
        ref = lls_ref.lsqr(A.matvec, A.transpose().matvec, A.shape, b.copy(), itnlim=25, etol=0.0)
        assert g1["itn"] == ref["itn"] and g1["istop"] == ref["istop"]
        assert np.linalg.norm(g1["x"] - ref["x"]) <= 1e-11 * np.linalg.norm(ref["x"])


# ------------------------------------------------------------------------------------------------ 5. Chebyshev steps
@pytest.mark.parametrize("fmt,name", [(5, "varcoef"), (7, "s27_var"), (9, "bricks")])
def test_chebyshev_steps(fmt, name, monkeypatch):
    """MkChebEpi stores d_j through the NT branch: the apply against the NumPy restatement, MINRES preconditioned by it
    against the same run with the flag off."""
    from pykrylov_amd import tools
    monkeypatch.setattr(kr, "_sq", lambda a: a * a)
    A, op0, op1 = pair(name, fmt, symmetric=True)
    n = A.shape[0]
    v = np.random.default_rng(11).standard_normal(n)
    lmin, lmax = cheb_ref.interval(A)
    want = cheb_ref.apply(A, v, 4, lmin, lmax)
    rhs = A.matvec(np.ones(n))
    runs = []
    for op, nt in ((op0, 0), (op1, 1)):
        M = tools.chebyshev(op, degree=4)
        assert M.interval == (lmin, lmax)
        assert bits(M * v) == bits(want), (fmt, name, nt)
        runs.append(run_loop("minres", op, rhs, precon=M, budget=12))
        check(op, fmt, nt)
        M.free()
    assert runs[0][0] == 12 and same_run(runs[0], runs[1])
    op0.free()
    op1.free()


# ------------------------------------------------------------------------------------------------ 6. diagonal preconditioner
@pytest.mark.parametrize("fmt,name", [(5, "varcoef"), (7, "s27_var")])
@pytest.mark.parametrize("solver", ["bicgstab", "minres"])
def test_diagonal_preconditioner_inside_the_kernels(solver, fmt, name):
    from pykrylov_amd import DiagonalOperator
    A, op0, op1 = pair(name, fmt, symmetric=solver == "minres")
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    dinv = 1.0 / A.data[A.indices == rows]                   # (positive: MINRES needs a definite preconditioner)
    assert dinv.shape == (n,) and (dinv > 0).all()
    rhs = A.matvec(np.ones(n))
    r0 = run_loop(solver, op0, rhs, precon=DiagonalOperator(dinv))
    r1 = run_loop(solver, op1, rhs, precon=DiagonalOperator(dinv))
    plain = run_loop(solver, op1, rhs)
    check(op0, fmt, 0)
    check(op1, fmt, 1)
    assert BUDGET - 2 <= r0[0] <= BUDGET + 2 and same_run(r0, r1)
    assert not np.array_equal(plain[2], r1[2])               # (the preconditioner did take part)
    op0.free()
    op1.free()
