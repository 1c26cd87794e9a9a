"""Infinities and NaNs in x, in every storage format that pads (csrc/mk_spmv_fmt*.h, mk_format.hip).  The windowed, pattern,
wide and resident formats (storage 1 .. 8 and 3) fill short rows with +0.0 entries that point at a zero cell and keep values
in dictionaries; the scalar loop they restate computes `0 * inf = NaN` for a STORED zero and nothing at all for an entry a row
does not have.  So an infinity in x must turn into NaN exactly in the rows that hold a stored 0.0 / -0.0 in its column, into
+-inf in the rows that hold another value there, and must not reach any other row: a builder that drops a stored zero, or a
pad that reads a live window cell, fails here and nowhere else (every other product check uses finite x).  The references are
proved on the CPU first, in the tests themselves."""
import numpy as np
import pytest

from oracle import csr_ref, krylov_ref as kr
from test_gpu_formats import MATS, banded, fmt_info
from test_gpu_nontemporal import _rows_without_a_diagonal_entry, run_loop, run_oracle, same_run
from test_gpu_tile_order import get_order, set_order
from test_gpu_wide import fixed_width_random_band

pytestmark = pytest.mark.gpu

SPECIAL = (0.0, -0.0, 2.0 ** -1060)                          # stored zeros of both signs and a denormal
STORAGES = (0, 1, 2, 3, 4, 5, 6, 7, 8)


def with_values(A, data):
    """The sparsity of A with these values, bit for bit (csr_ref.from_coo adds duplicates up from +0.0, which turns a
    -0.0 into +0.0)."""
    return csr_ref.RefCsr(A.indptr, A.indices, np.asarray(data, dtype=np.float64), A.shape)


def sprinkled(A, seed, share=0.08):
    """A with `share` of its off-diagonal entries replaced by the special values in turn, and the zeros it already
    stores given alternating signs."""
    rng = np.random.default_rng(seed)
    data = A.data.copy()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    pick = np.flatnonzero((rows != A.indices) & (rng.random(A.nnz) < share))
    data[pick] = np.asarray(SPECIAL)[np.arange(len(pick)) % 3]
    zeros = np.flatnonzero(data == 0.0)
    data[zeros[::2]] = 0.0
    data[zeros[1::2]] = -0.0
    return with_values(A, data)


def _band_structure(n=9000, holes=False):
    """Five diagonals; with `holes` every fifth row lacks one of its entries, another one from row to row (short rows in
    the middle of every tile: the formats pad them, and what a row lacks differs)."""
    r, c, _ = banded(n, (-300, -1, 0, 1, 300), np.random.default_rng(5))
    if holes:
        keep = ~((r % 5 == 0) & (c - r == np.array([-300, -1, 0, 1, 300])[(r // 5) % 5]))
        r, c = r[keep], c[keep]
    return csr_ref.from_coo(r, c, np.ones(len(r)), (n, n))


def _banded_dict():
    """MATS["banded_dict"]'s kind: every value drawn from a small set, here with both zeros and a denormal in it."""
    S = _band_structure()
    return with_values(S, np.random.default_rng(6).choice([-1.0, 4.0, 0.5, -0.0, 0.0, 2.0 ** -1060], size=S.nnz))


def _banded_by_offset(holes=False):
    """One value per diagonal (few row patterns: the pattern + dictionary format takes it)."""
    S = _band_structure(holes=holes)
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    value = {-300: -1.0, -1: 0.0, 0: 4.0, 1: -0.0, 300: 2.0 ** -1060}
    return with_values(S, [value[int(o)] for o in S.indices - rows])


def _banded_manyvalues(holes=False):
    S = _band_structure(holes=holes)
    return sprinkled(with_values(S, np.random.default_rng(7).standard_normal(S.nnz)), 8)


def _ragged_rows():
    """The matrix of test_gpu_wide.py::test_ragged_rows_pad_up_to_half: odd rows keep half of their entries."""
    rng = np.random.default_rng(15)
    n = 6000
    A = fixed_width_random_band(n, 24, 900, rng)
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    drop = (rows % 2 == 1) & (A.indices != rows) & (rng.random(A.nnz) < 0.5)
    return csr_ref.from_coo(rows[~drop], A.indices[~drop], A.data[~drop], (n, n))


def _stencil27(seed):
    """27-point operator on a 64 x 10 x 5 grid (12 tiles and a half) whose east entries are stored +0.0, whose west entries
    -0.0 and whose north entries a denormal: the same change in every row, so the rows keep their few patterns."""
    mx = 64
    A = csr_ref.stencil27(mx, 10, 5, seed=seed)
    off = A.indices - np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    data = A.data.copy()
    data[off == 1] = 0.0
    data[off == -1] = -0.0
    data[off == mx] = 2.0 ** -1060
    return with_values(A, data)


BUILDERS = {
    "banded_dict": _banded_dict,
    "banded_by_offset": _banded_by_offset,
    "banded_manyvalues": _banded_manyvalues,
    "banded_by_offset_holes": lambda: _banded_by_offset(holes=True),
    "banded_manyvalues_holes": lambda: _banded_manyvalues(holes=True),
    "banded_plus_dense_rows": lambda: sprinkled(MATS["banded_plus_dense_rows"][0], 9),
    "rect_odd_cols": lambda: sprinkled(MATS["rect_odd_cols"][0], 10),
    "ragged_rows": lambda: sprinkled(_ragged_rows(), 11),
    "stencil27_const": lambda: _stencil27(0),
    "stencil27_var": lambda: _stencil27(7),
    "scattered": lambda: sprinkled(csr_ref.random_diagdom(5003), 12),
}
NAMES = sorted(BUILDERS)
_CACHE = {}


def problem(name):
    """Per matrix, once: the matrix, its transpose, and for both the three input vectors with their reference products."""
    if name not in _CACHE:
        A = BUILDERS[name]()
        _CACHE[name] = (A, vectors(A, 1), vectors(A.transpose(), 2))
    return _CACHE[name]


def vectors(A, seed):
    """x with +inf in three columns -- one that holds a stored zero in some row, the last one, one on a boundary of the
    128-double window chunks -- and x with a single NaN, each with the scalar loop's product.  The reference is checked
    here: a stored zero meets an infinity and gives NaN, some row is +-inf, more than half of the rows stay finite.
    Three columns are few: a pad that read a live cell of the window would have to hit one of them.  So a third x is +inf
    EVERYWHERE but in the columns of a few short rows (rows the formats pad up to the longest row of their tile), whose
    sums must stay finite -- whatever else a pad of theirs reads is an infinity."""
    m, n = A.shape
    rng = np.random.default_rng(seed)
    zero_cols = np.unique(A.indices[A.data == 0.0])
    assert len(zero_cols) > 0
    ja = int(zero_cols[len(zero_cols) // 2])
    jc = 128 * max(1, (n // 3) // 128)
    x = rng.standard_normal(n)
    x[[ja, n - 1, jc]] = np.inf
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    with np.errstate(invalid="ignore", over="ignore"):
        y = A.matvec(x)
    met = (A.data == 0.0) & np.isinf(x[A.indices])           # stored zeros that meet an infinity
    assert met.any() and np.isnan(y[rows[met]]).all()
    assert np.isinf(y).any() and np.isfinite(y).sum() > m // 2
    x2 = rng.standard_normal(n)
    x2[ja] = np.nan
    with np.errstate(invalid="ignore"):
        y2 = A.matvec(x2)
    assert np.isnan(y2).any() and np.isfinite(y2).sum() > m // 2
    length = np.diff(A.indptr)
    longest = np.repeat(np.maximum.reduceat(length, np.arange(0, m, 256)), 256)[:m]
    short = np.flatnonzero((length > 0) & (length < longest))
    assert len(short) > 0
    pick = np.unique(short[np.linspace(0, len(short) - 1, 16).astype(np.int64)])
    x3 = np.full(n, np.inf)
    for r in pick:
        x3[A.indices[A.indptr[r]:A.indptr[r + 1]]] = rng.standard_normal(length[r])
    with np.errstate(invalid="ignore"):
        y3 = A.matvec(x3)
    assert np.isfinite(y3[pick]).all() and np.isfinite(y3).sum() < m // 2
    return (x, y), (x2, y2), (x3, y3)


def same_product(got, ref):
    fin = np.isfinite(ref)
    inf = np.isinf(ref)
    return (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), inf)
            and np.array_equal(got[inf], ref[inf])           # (the sign of an infinity)
            and np.array_equal(got[fin], ref[fin]) and np.array_equal(np.signbit(got[fin]), np.signbit(ref[fin])))


REACHED = {}                                                 # (matrix, storage asked for) -> storage of A, storage of A'


def build(name, want):
    from pykrylov_amd import CsrOperator, _lib
    A = problem(name)[0]
    op = CsrOperator(A.indptr, A.indices, A.data, A.shape)
    _lib.check(_lib.init().mk_csr_set_format(op.handle, want))
    _lib.check(_lib.init().mk_csr_set_format(op.T.handle, want))      # (the transposed copy is a matrix of its own)
    REACHED[name, want] = (fmt_info(op)["fmt"], fmt_info(op.T)["fmt"])
    return op


@pytest.mark.parametrize("want", STORAGES)
@pytest.mark.parametrize("name", NAMES)
def test_nonfinite_x_reaches_the_rows_of_the_scalar_loop(name, want):
    A, forward, backward = problem(name)
    op = build(name, want)
    got = REACHED[name, want]
    assert got[0] <= max(want, 3) and got[1] <= max(want, 3), (name, want, got)       # requests only degrade
    for nt in ((-1, 1) if got[0] in (5, 6, 7) or got[1] in (5, 6, 7) else (-1,)):     # NT kernel variants once more
        if nt == 1:
            set_order(op, -1, 0, 0, 1)
            set_order(op.T, -1, 0, 0, 1)
            assert get_order(op)[3] == 1 and get_order(op.T)[3] == 1
        for x, y in forward:
            assert same_product(op * x, y), (name, want, got, nt)
        for u, z in backward:
            assert same_product(op.T * u, z), (name, want, got, nt)
    assert (fmt_info(op)["fmt"], fmt_info(op.T)["fmt"]) == got
    op.free()


@pytest.mark.parametrize("fmt,every_seventh_has_one", [(5, False), (6, True)])
def test_minres_scaled_gather_on_padded_rows(fmt, every_seventh_has_one, monkeypatch):
    """MINRES' epilogue multiplies every gathered entry by 1 / beta on the fly (`xin`), the pads' zero cell included: on
    matrices whose rows are padded (rows of 2 entries among rows of 3), with a right-hand side -- the first product's input
    -- that holds -0.0 and denormals, the oracle's bits."""
    from pykrylov_amd import CsrOperator, _lib
    monkeypatch.setattr(kr, "_sq", lambda a: a * a)
    A = _rows_without_a_diagonal_entry(every_seventh_has_one)
    n = A.shape[0]
    assert len(np.unique(np.diff(A.indptr))) >= 2
    op = CsrOperator(A.indptr, A.indices, A.data, A.shape, symmetric=True)
    _lib.check(_lib.init().mk_csr_set_format(op.handle, fmt))
    assert fmt_info(op)["fmt"] == fmt
    rhs = A.matvec(np.linspace(1.0, 2.0, n))
    rhs[::5] = -0.0
    rhs[1::7] = 2.0 ** -1060
    rhs[3::11] = -2.0 ** -1070
    got = run_loop("minres", op, rhs, budget=10)
    assert got[0] == 10 and same_run(got, run_oracle("minres", A, rhs, op, budget=10))
    assert fmt_info(op)["fmt"] == fmt
    op.free()


def test_every_storage_was_reached():
    """Which storage every (matrix, request) ended in -- cases the tests above have not built are built now -- and that
    each of the nine took part, for A and for its transposed copy."""
    for name in NAMES:
        for want in STORAGES:
            if (name, want) not in REACHED:
                build(name, want).free()
    for name in NAMES:
        print("%-24s" % name, " ".join("%d->%d/%d" % ((want,) + REACHED[name, want]) for want in STORAGES))
    assert {f for f, _ in REACHED.values()} >= set(STORAGES), sorted({f for f, _ in REACHED.values()})
    assert {f for _, f in REACHED.values()} >= set(STORAGES), sorted({f for _, f in REACHED.values()})
