"""Matrices that reach every storage format 0 .. 8 of the product kernel, for the tests that run each fused epilogue in each
storage (tests/test_gpu_epilogue_storage.py, tests/test_gpu_nontemporal.py), and the table EPILOGUES that says where every
epilogue type of pykrylov_amd/csrc is run through the storages.  The square matrices are symmetric bit for bit.  What the GPU
tests rely on -- symmetry, empty rows and tiles, row lengths, distinct values, rows without a diagonal entry, that no loop ends
before its budget -- is asserted on the CPU by tests/test_storage_matrices_cpu.py.  No test functions here.

The builders that tests/test_gpu_nontemporal.py already has are imported from there (inside the functions: that module imports
the band matrices of this one)."""
import numpy as np

from oracle import csr_ref

N_BAND = 9001                                                # 35 tiles of 256 rows and a last one of 41
BAND_OFFSETS = (1, 300)
N_COLBLOCKS = 20011
COLBLOCK_KB = 64                                             # x = 160 088 B in blocks of 65 536 B: 3 column blocks
_CACHE = {}


def _nt():
    import test_gpu_nontemporal
    return test_gpu_nontemporal


def _formats():
    import test_gpu_formats
    return test_gpu_formats


def sym_band(distinct, holes=False):
    """Symmetric band matrix with the offsets (0, +-1, +-300): the diagonal 4 (+ [0, 0.25) when `distinct`), the off-diagonal
    entries drawn from three constants (four with `holes`) or all distinct in (-1, -0.5]; the entries (i, i + o) and (i + o, i)
    share one value.  Diagonally dominant, so definite where no row is empty.  With `holes` the entry (i, i + o) and its mirror
    image are left out where (i + o) % 5 == 0 -- every fifth entry of an off-diagonal, at a phase that depends on the offset --
    and the rows and columns 1000 .. 1999 and those with r % 11 == 3 are removed entirely, diagonal entry included."""
    n = N_BAND
    rng = np.random.default_rng(31 + 2 * int(holes) + int(distinct))
    alive = np.ones(n, dtype=bool)
    if holes:
        alive[1000:2000] = False
        alive[np.arange(n) % 11 == 3] = False
    d = np.flatnonzero(alive)
    consts = np.array([-1.0, -0.75, -0.5, 0.5][:4 if holes else 3])
    rows, cols = [d], [d]
    vals = [4.0 + 0.25 * rng.random(len(d)) if distinct else np.full(len(d), 4.0)]
    for o in BAND_OFFSETS:
        i = np.arange(n - o)
        keep = alive[i] & alive[i + o]
        if holes:
            keep &= (i + o) % 5 != 0
        i = i[keep]
        w = -(0.5 + 0.5 * rng.random(len(i))) if distinct else rng.choice(consts, size=len(i))
        rows += [i, i + o]
        cols += [i + o, i]
        vals += [w, w]
    return csr_ref.from_coo(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), (n, n))


def _with_distinct_values(A, seed):
    """The pattern of `A` with all-distinct values in +-[0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    v = (0.5 + rng.random(A.nnz)) * rng.choice([-1.0, 1.0], size=A.nnz)
    return csr_ref.RefCsr(A.indptr, A.indices, v, A.shape)


def _scattered_tall():
    """5003 x 3001: a unit diagonal block on top (full column rank) and four scattered entries in every row."""
    R, C = 5003, 3001
    rng = np.random.default_rng(23)
    rows = np.concatenate([np.arange(C), np.repeat(np.arange(R), 4)])
    cols = np.concatenate([np.arange(C), rng.integers(0, C, 4 * R)])
    vals = np.concatenate([np.ones(C), rng.random(4 * R) - 0.5])
    return csr_ref.from_coo(rows, cols, vals, (R, C))


def _less_columns(A):
    """`A` less the last 10 % of its columns: the rows that lose entries are shorter than the others."""
    m, n = A.shape
    k = n - n // 10
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    keep = A.indices < k
    return csr_ref.from_coo(rows[keep], A.indices[keep], A.data[keep], (m, k))


def _no_diagonal_few_values():
    """The structure of `no_diagonal_on_every_7th_row` (a path graph; every seventh row lacks the diagonal entry) with its
    weights drawn from three constants: the all-distinct weights of the original have no dictionary, and a request for
    storage 4 (pattern byte + dictionary of <= 256 values) degrades to 1 with them."""
    A = _nt().mat("no_diagonal_on_every_7th_row")
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    w = np.array([1.0, -0.5, 0.75])[np.minimum(rows, A.indices) % 3]
    return csr_ref.RefCsr(A.indptr, A.indices, np.where(rows == A.indices, 3.0, w), A.shape)


def _slots_tall():
    """Two symmetric slot matrices of 3584 rows on top of each other: every row has about 15 entries and every column about
    30, so that A and the transposed copy both take the slot format (the transposed copy of `rect_wide`, whose columns are
    ragged, is refused by it)."""
    nt = _nt()
    S1 = nt.symmetric_slots(3584, 7, 512, np.random.default_rng(41))
    S2 = nt.with_diagonal_shifted(nt.symmetric_slots(3584, 7, 512, np.random.default_rng(42)), -4.0)
    return csr_ref.RefCsr(np.concatenate([S1.indptr, S1.indptr[-1] + S2.indptr[1:]]), np.concatenate([S1.indices, S2.indices]),
                          np.concatenate([S1.data, S2.data]), (2 * 3584, 3584))


BUILDERS = {
    "band_dict": lambda: sym_band(False),
    "band_distinct": lambda: sym_band(True),
    "holes_dict": lambda: sym_band(False, holes=True),
    "holes_distinct": lambda: sym_band(True, holes=True),
    "colblocks": lambda: _nt().symmetrised(csr_ref.random_diagdom(N_COLBLOCKS, seed=2)),
    "rect_odd_cols": lambda: _formats().MATS["rect_odd_cols"][0],
    "rect_odd_distinct": lambda: _with_distinct_values(mat("rect_odd_cols"), 29),
    "scattered_tall": _scattered_tall,
    "no_diagonal_few_values": _no_diagonal_few_values,
    "slots_tall": _slots_tall,
    "poisson2d_tall": lambda: _less_columns(mat("poisson2d")),
    "s27_var_tall": lambda: _less_columns(mat("s27_var")),
    "s27_const_tall": lambda: _less_columns(mat("s27_const")),
}


def mat(name):
    """The matrix `name` of this module or of tests/test_gpu_nontemporal.py, built once."""
    if name not in BUILDERS:
        return _nt().mat(name)
    if name not in _CACHE:
        _CACHE[name] = BUILDERS[name]()
    return _CACHE[name]


# storage -> the symmetric matrices that run in it.  "plain": every row has a positive diagonal entry (scale_diag=True is run
# there too); "holes": empty rows and three all-empty tiles; "nodiag": rows without a diagonal entry.
SQUARE = (
    (0, "scattered_sym", "plain"), (3, "scattered_sym", "plain"),
    (1, "band_distinct", "plain"), (2, "band_dict", "plain"),
    (4, "poisson2d", "plain"), (5, "varcoef", "plain"), (6, "slots_sym", "plain"), (7, "s27_var", "plain"),
    (8, "s27_const", "plain"),
    (1, "holes_distinct", "holes"), (2, "holes_dict", "holes"),
    (0, "holes_distinct", "holes"), (3, "holes_distinct", "holes"), (0, "holes_dict", "holes"), (3, "holes_dict", "holes"),
    (4, "no_diagonal_few_values", "nodiag"), (5, "no_diagonal_on_every_7th_row", "nodiag"),
    (7, "no_diagonal_on_every_7th_row", "nodiag"), (6, "diagonal_on_every_7th_row", "nodiag"),
)
SQUARE_NAMES = tuple(sorted({name for _, name, _ in SQUARE} | {"colblocks"}))

# (storage of A, storage of the transposed copy, matrix) of the rectangular epilogues: all nine storages are reached on both
# sides.  What the builder refused on the way (MK_DEBUG_PLAN=1): the transposed copy of `rect_wide` asked for 6 stays in plain
# CSR (its rows have 4 .. 29 entries: too ragged for the slot format, and the builder gives no other reason), hence
# `slots_tall`; asked for 4, `tall_band` (all-distinct values: no dictionary) ends in 1, `rect_odd_cols` in 2 ("too many
# distinct patterns") and the 27-point matrices in 0, hence `poisson2d_tall`.
RECT = (
    (6, 0, "rect_wide"), (6, 6, "slots_tall"), (5, 5, "tall_band"), (2, 2, "rect_odd_cols"), (1, 1, "rect_odd_distinct"),
    (0, 0, "scattered_tall"), (3, 3, "scattered_tall"), (4, 4, "poisson2d_tall"), (7, 7, "s27_var_tall"),
    (8, 8, "s27_const_tall"),
)
RECT_NAMES = tuple(sorted({name for _, _, name in RECT}))
RECT_STORAGES = set(range(9))


def lls_rhs(A, solver):
    """The right-hand side of tests/test_gpu_nontemporal.py::test_least_squares_loops: consistent (CRAIG needs that), with a
    little noise for LSQR and LSMR."""
    b = A.matvec(np.ones(A.shape[1]))
    if solver in ("lsqr", "lsmr"):
        b = b + 1e-3 * np.random.default_rng(18).standard_normal(A.shape[0])
    return b


# (solver, damp) of the least-squares runs, and their arguments: 25 passes, and nothing may end a run before them -- the error
# estimate is off (etol = 0) and so are the tolerances of LSQR and LSMR, whose damped runs would stop after 24 passes otherwise
LLS_RUNS = (("lsqr", 0.0), ("lsqr", 0.1), ("lsmr", 0.0), ("lsmr", 0.1), ("craig", 0.0), ("craigmr", 0.0))


def lls_arguments(solver):
    return dict(itnlim=25, atol=0.0, btol=0.0) if solver in ("lsqr", "lsmr") else dict(itnlim=25)


def denormal_start(n):
    """A Lanczos start vector holding -0.0, 2**-1060 and -2**-1070 at strides 5, 7 and 11: the gather scaled by 1 / beta then
    multiplies signed zeros and denormals."""
    v = np.random.default_rng(12).standard_normal(n)
    v[::5] = -0.0
    v[::7] = 2.0 ** -1060
    v[::11] = -2.0 ** -1070
    return v


# Every struct of pykrylov_amd/csrc that declares `double xin(` -- the epilogue types mk_spmv_kernel is instantiated for and
# their wrappers -- and the test case that runs it through the storage formats.  tests/test_storage_matrices_cpu.py compares
# the keys with the sources: a new epilogue type needs a row here, that is, a test over the storages.
_LOOPS = "test_gpu_nontemporal.py::test_every_loop_that_carries_the_flag"
_NEW = "test_gpu_epilogue_storage.py::"
EPILOGUES = {
    "MkPlainEpi": "test_gpu_nontemporal.py::test_products_keep_their_bits",
    "CgSpmvEpiT": "test_gpu_formats.py::test_solver_results_do_not_depend_on_the_format, test_gpu_wide.py, test_gpu_varcoef.py",
    "CgFusedEpiT": "test_gpu_pencil.py (march only: storages 9 .. 11)",
    "BEpi": _LOOPS + "[bicgstab-*], [cgs-*]",
    "DEpi": _LOOPS + "[bicgstab-*], [cgs-*]",
    "EpiP4": _LOOPS + "[tfqmr-*]",
    "EpiP6": _LOOPS + "[tfqmr-*]",
    "EpiK1": _LOOPS + "[minres-*], [symmlq-*]",
    "EpiS2": _LOOPS + "[symmlq-*]",
    "EpiFinR": _LOOPS + "[symmlq-*]",
    "LzEpi": _NEW + "test_lanczos",
    "MkChebEpi": _NEW + "test_chebyshev_preconditioner",
    "MkChebFiltEpi": _NEW + "test_chebyshev_filter",
    "SvEpiU": _NEW + "test_svd[*-one-sided]",
    "SvEpiPlain": _NEW + "test_svd",
    "EpiU": _NEW + "test_least_squares",
    "EpiV": _NEW + "test_least_squares",
    "MkAmgEpi": "test_gpu_amg.py::test_apply_bits",
    "MkPartialOf": _NEW + "test_lanczos[colblocks] (the launches before the last of a column-blocked product)",
    "MkAccumOf": "test_gpu_blkop.py (block operators: plain products of the blocks)",
    "MkAddOf": "test_gpu_nontemporal.py::test_device_sums_and_products_of_two_nt_operators",
    "MkNoXin": "test_gpu_nontemporal.py::test_device_sums_and_products_of_two_nt_operators",
}
