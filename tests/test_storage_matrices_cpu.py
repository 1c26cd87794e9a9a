"""What the GPU tests of the epilogue x storage grid (tests/test_gpu_epilogue_storage.py, tests/test_gpu_nontemporal.py) rely
on, asserted without a GPU: the structure of every matrix of tests/_storage_matrices.py, that every restatement run on them
with NumPy's dots meets the conditions of the GPU tests -- no Lanczos breakdown, finite Chebyshev applies, every loop still
running when its budget ends, so that a wrong kernel cannot hide behind an early stop --, and that the table of epilogue types
names every struct of pykrylov_amd/csrc with a `double xin(` member."""
import glob
import os
import re

import numpy as np
import pytest

from oracle import krylov_ref as kr
from tests import _cheb_ref as cheb_ref, _chebfilt_ref as filt_ref, _lanczos_ref as lanczos_ref, _storage_matrices as sm
from tests import _trsvd_ref as trsvd_ref
from test_gpu_lls import run_oracle
from test_gpu_nontemporal import BUDGET, LOOP_MATRICES, LOOPS, SYMMETRIC_LOOPS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pykrylov_amd", "csrc")

# name -> (empty rows, all-empty tiles of 256 rows, shortest row, longest row, more than 256 distinct values, rows that have
#          entries but no diagonal entry)
STRUCTURE = {
    "band_dict": (0, 0, 3, 5, False, 0),
    "band_distinct": (0, 0, 3, 5, True, 0),
    "holes_dict": (1727, 3, 0, 5, False, 0),
    "holes_distinct": (1727, 3, 0, 5, True, 0),
    "colblocks": (0, 0, 5, 20, True, 0),
    "scattered_sym": (0, 0, 5, 19, True, 0),
    "poisson2d": (0, 0, 3, 5, False, 0),
    "varcoef": (0, 0, 4, 7, True, 0),
    "slots_sym": (0, 0, 13, 17, True, 0),
    "s27_var": (0, 0, 8, 27, True, 0),
    "s27_const": (0, 0, 8, 27, False, 0),
    "no_diagonal_few_values": (0, 0, 1, 3, False, 858),
    "no_diagonal_on_every_7th_row": (0, 0, 1, 3, True, 858),
    "diagonal_on_every_7th_row": (0, 0, 1, 3, True, 5143),
    "rect_odd_cols": (903, 3, 0, 5, False, None),
    "rect_odd_distinct": (903, 3, 0, 5, True, None),
    "rect_wide": (0, 0, 2, 14, True, None),
    "slots_tall": (0, 0, 12, 15, True, None),
    "scattered_tall": (0, 0, 3, 5, True, None),
    "tall_band": (600, 3, 0, 5, True, None),
    "poisson2d_tall": (2100, 8, 0, 5, False, None),
    "s27_var_tall": (0, 0, 4, 27, True, None),
    "s27_const_tall": (0, 0, 4, 27, False, None),
}


def ints(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_the_table_names_every_matrix():
    assert set(STRUCTURE) == set(sm.SQUARE_NAMES) | set(sm.RECT_NAMES)
    assert {f for f, _, _ in sm.SQUARE} == set(range(9))     # no storage is left out for the square epilogues
    assert sm.RECT_STORAGES <= {f for f, _, _ in sm.RECT} and sm.RECT_STORAGES <= {f for _, f, _ in sm.RECT}
    assert sm.RECT_STORAGES >= set(range(9)) - {4, 7, 8}     # (only these may be left out for the rectangular ones)


@pytest.mark.parametrize("name", sorted(STRUCTURE))
def test_structure(name):
    A = sm.mat(name)
    m, n = A.shape
    empty, empty_tiles, shortest, longest, many, nodiag = STRUCTURE[name]
    length = np.diff(A.indptr)
    ip = A.indptr.astype(np.int64)
    starts = np.arange(0, m, 256)
    assert int((length == 0).sum()) == empty
    assert int((ip[np.minimum(starts + 256, m)] == ip[starts]).sum()) == empty_tiles
    assert (int(length.min()), int(length.max())) == (shortest, longest)
    assert (len(np.unique(ints(A.data))) > 256) == many, len(np.unique(ints(A.data)))
    assert np.isfinite(A.data).all()
    if name in sm.SQUARE_NAMES:                              # symmetric bit for bit
        T = A.transpose()
        assert m == n and np.array_equal(A.indptr, T.indptr) and np.array_equal(A.indices, T.indices)
        assert np.array_equal(ints(A.data), ints(T.data))
        d = cheb_ref.diagonal(A)
        assert int((np.isnan(d) & (length > 0)).sum()) == nodiag
        kinds = {k for _, nm, k in sm.SQUARE if nm == name} | ({"plain"} if name == "colblocks" else set())
        assert len(kinds) == 1
        kind = kinds.pop()
        assert (kind == "plain") == bool(np.all(d > 0))      # scale_diag=True runs exactly where it can
        assert (kind == "holes") == (empty > 0 and empty_tiles > 0) and (kind == "nodiag") == (nodiag > 0)
    else:
        assert m > n                                         # tall: the SVD loop takes A as it is


def test_the_band_matrices_have_a_ragged_last_tile():
    assert sm.N_BAND == 35 * 256 + 41 and 8 * sm.N_COLBLOCKS > 2 * 1024 * sm.COLBLOCK_KB
    assert -(-8 * sm.N_COLBLOCKS // (1024 * sm.COLBLOCK_KB)) == 3


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("name", sm.SQUARE_NAMES)
def test_lanczos_takes_all_its_steps(name):
    A = sm.mat(name)
    plain = bool(np.all(cheb_ref.diagonal(A) > 0))
    for scaled in ((False, True) if plain else (False,)):
        for start in (None, sm.denormal_start(A.shape[0])):
            got = lanczos_ref.lanczos(A, steps=10, scale_diag=scaled, start=start)
            assert got.steps == 10 and np.isfinite(got.alpha).all() and np.isfinite(got.beta).all(), (name, scaled)


def test_the_start_vector_holds_signed_zeros_and_denormals():
    v = sm.denormal_start(9001)
    assert np.signbit(v[5]) and v[5] == 0.0 and v[7] == 2.0 ** -1060 and v[11] == -2.0 ** -1070 and v[1] != 0.0
    assert 0.0 < abs(v[7]) < np.finfo(np.float64).tiny


@pytest.mark.parametrize("name", sm.SQUARE_NAMES)
def test_chebyshev_applies_are_finite(name):
    A = sm.mat(name)
    n = A.shape[0]
    plain = bool(np.all(cheb_ref.diagonal(A) > 0))
    for scaled in ((False, True) if plain else (False,)):
        lmin, lmax = cheb_ref.interval(A, scale_diag=scaled)
        z = cheb_ref.apply(A, np.random.default_rng(11).standard_normal(n), 4, lmin, lmax, scaled)
        assert np.isfinite(z).all() and z.any(), (name, scaled)
    a, b = filt_ref.interval(A)
    y = filt_ref.apply(A, np.random.default_rng(17).standard_normal(n), 8, a + 0.3 * (b - a), b, a)
    assert a < b and np.isfinite(y).all() and y.any(), name


def _products(solver, A, rhs):
    if solver == "minres":
        return kr.minres(A, rhs, check=False, etol=0.0, rtol=1e-15, itnlim=BUDGET)["itn"]
    if solver == "symmlq":
        return kr.symmlq(A, rhs, matvec_max=BUDGET, rtol=1e-15)["nMatvec"]
    return getattr(kr, solver)(A, rhs, abstol=0.0, reltol=1e-15, matvec_max=BUDGET)["nMatvec"]


@pytest.mark.parametrize("solver", LOOPS)
def test_the_older_loops_run_to_their_budget(solver):
    """On every matrix of test_gpu_nontemporal.py::test_every_loop_that_carries_the_flag, storages 1 and 2 included, and on
    the matrices with empty rows of test_gpu_epilogue_storage.py::test_older_loops_on_empty_rows_and_tiles."""
    names = sorted({pair[1 if solver in SYMMETRIC_LOOPS else 0] for pair in LOOP_MATRICES.values()})
    assert {"band_sym_distinct", "band_sym_dict"} <= set(names) and {1, 2} <= set(LOOP_MATRICES)
    for name in names + ["holes_dict", "holes_distinct"]:
        A = sm.mat(name)
        k = _products(solver, A, A.matvec(np.ones(A.shape[0])))
        assert BUDGET - 2 <= k <= BUDGET + 2, (solver, name, k)


@pytest.mark.parametrize("name", sm.RECT_NAMES)
def test_least_squares_loops_take_25_passes(name):
    A = sm.mat(name)
    for solver, damp in sm.LLS_RUNS:
        ref = run_oracle(solver, A, sm.lls_rhs(A, solver), damp, 0.0, **sm.lls_arguments(solver))
        assert ref["itn"] == 25 and np.isfinite(ref["x"]).all(), (name, solver, damp, ref["itn"], ref["istop"])


@pytest.mark.parametrize("name", sm.RECT_NAMES)
def test_svd_spends_its_products(name):
    A = sm.mat(name)
    for reorth in ("full", "one-sided"):
        r = trsvd_ref.trsvd(A, 2, ncv=9, matvec_max=40, reorth=reorth)
        assert r.nMatvec > 30 and r.breakdown == 0 and np.isfinite(r.history).all(), (name, reorth, r.nMatvec)


# ------------------------------------------------------------------------------------------------ the epilogue list
def epilogue_types():
    """Every struct of the kernel sources that declares a `double xin(` member."""
    found = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            text = f.read()
        for m in re.finditer(r"__device__\s+double\s+xin\(", text):
            found.add(re.findall(r"\bstruct\s+(\w+)[^;{]*\{", text[:m.start()])[-1])
    return found


def test_every_epilogue_type_has_a_test_over_the_storages():
    found = epilogue_types()
    assert {"LzEpi", "MkChebEpi", "MkChebFiltEpi", "SvEpiU", "SvEpiPlain", "EpiU", "EpiV", "MkAmgEpi", "MkPlainEpi"} <= found
    assert found == set(sm.EPILOGUES), (sorted(found - set(sm.EPILOGUES)), sorted(set(sm.EPILOGUES) - found))
    tests = os.path.dirname(os.path.abspath(__file__))
    for epi, where in sm.EPILOGUES.items():
        files = re.findall(r"test_\w+\.py", where)
        assert files and all(os.path.exists(os.path.join(tests, f)) for f in files), (epi, where)
        for f, t in re.findall(r"(test_\w+\.py)::(test_\w+)", where):
            with open(os.path.join(tests, f)) as src:
                assert "def %s(" % t in src.read(), (epi, f, t)
