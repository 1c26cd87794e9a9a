"""The NumPy restatement of the smoothed-aggregation AMG preconditioner (tests/_amg_ref.py) against the mathematics -- the
roots are a maximal independent set at distance 2, every node has an aggregate, P has the rows its rule implies, the coarse
matrix is P' A P, the cycle preconditions CG -- and the entry points and argument checks of `tools.amg`.  No device."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import csr_ref
from tests import _amg_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MATRICES = ("poisson2d_13", "poisson3d_8", "1138bus", "isolated")
ISOLATED_ROW = 37


def matrix(name):
    if name.startswith("poisson2d_"):
        return csr_ref.poisson2d(int(name.split("_")[1]))
    if name.startswith("poisson3d_"):
        return csr_ref.poisson3d(int(name.split("_")[1]))
    if name == "1138bus":
        return csr_ref.read_matrix_market(os.path.join(GOLDEN, "1138bus.mtx"))
    if name == "isolated":
        # poisson2d(9) with row and column ISOLATED_ROW cut off: that row stores its diagonal entry only
        A = csr_ref.poisson2d(9)
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        keep = (rows == A.indices) | ((rows != ISOLATED_ROW) & (A.indices != ISOLATED_ROW))
        return csr_ref.from_coo(rows[keep], A.indices[keep], A.data[keep], A.shape)
    raise KeyError(name)


_H = {}


def hierarchy(name, **kw):
    """The restated hierarchy of a matrix, built once per argument set and never modified."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _H:
        _H[key] = ref.build(matrix(name), **kw)
    return _H[key]


# ------------------------------------------------------------------ entry points and argument checks
NAMES = ("mk_amg_create", "mk_amg_destroy", "mk_amg_apply", "mk_amg_info", "mk_amg_level", "mk_amg_download", "mk_amg_coarse",
         "mk_solver_set_precon_amg", "mk_solver_set_lls_precon_amg")


def test_entry_points_are_declared_bound_and_exported():
    import pykrylov_amd
    from pykrylov_amd import _lib, tools
    header = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()                                             # (loading needs no GPU)
    for name in NAMES:
        assert re.search(r"MK_API int %s\(" % name, code), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert sorted(n for n in _lib.PROTOTYPES if "amg" in n) == sorted(NAMES)
    defines = dict(re.findall(r"#define (MK_AMG_[A-Z_]+) (\d+)", code))
    assert int(defines["MK_AMG_MAX_LEVELS"]) == 16 and _lib.MK_AMG_MAX_LEVELS == 16 and ref.MAX_LEVELS == 16
    assert int(defines["MK_AMG_MAX_COARSE"]) == 1024 and _lib.MK_AMG_MAX_COARSE == 1024 and ref.MAX_COARSE == 1024
    assert int(defines["MK_AMG_INFO_LEN"]) == _lib.MK_AMG_INFO_LEN
    assert lib.mk_version() == 100
    assert callable(tools.amg) and issubclass(tools.AmgPreconditioner, pykrylov_amd.LinearOperator)
    # the rules of the set-up are written out in the header
    for word in ("MIS(2)", "0x9E3779B97F4A7C15", "expand_cap", "Gershgorin", "stored order on ties"):
        assert word in header, word


def _fake_csr(shape, symmetric=True, local_size=None):
    """A CsrOperator shell without a device behind it: what the argument checks look at."""
    from pykrylov_amd.linop import CsrOperator
    op = object.__new__(CsrOperator)
    op.__dict__.update(_shape=shape, _symmetric=symmetric, _nargout=shape[0], _nargin=shape[1])
    if local_size is not None:
        op.local_size = local_size
    return op


def test_bad_arguments_are_refused_before_the_device_is_touched(monkeypatch):
    from pykrylov_amd import LinearOperator, _lib, tools

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "init", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    with pytest.raises(TypeError, match="CSR"):
        tools.amg(LinearOperator(4, 4, matvec=lambda v: v, symmetric=True))    # a callback operator
    with pytest.raises(ValueError, match="square"):
        tools.amg(_fake_csr((5, 4)))
    with pytest.raises(ValueError, match="symmetric"):
        tools.amg(_fake_csr((4, 4), symmetric=False))
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        tools.amg(_fake_csr((4, 4), local_size=2))
    ok = _fake_csr((4, 4))
    bad = dict(theta=(-0.1, np.nan, None, "a"), degree=(0, 65, 1.5, True), ratio=(1.0, 0.5, np.inf), omega=(0.0, -1.0, np.nan),
               coarse_max=(0, 1025, 2.0), max_levels=(0, 17, None), seed=(-1, 2 ** 64, 0.5), expand_cap=(-1, 2 ** 31, 1.5))
    for name, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=name):
                tools.amg(ok, **{name: v})


# ------------------------------------------------------------------ roots and aggregates
@pytest.mark.parametrize("name", MATRICES)
def test_roots_are_a_maximal_independent_set_at_distance_two(name):
    H = hierarchy(name, coarse_max=16)
    assert len(H.levels) >= 2
    for lv in H.levels[:-1]:
        A, strong, state = lv["A"], lv["strong"], lv["state"]
        n = A.shape[0]
        rows = np.repeat(np.arange(n), np.diff(A.indptr))
        G = np.zeros((n, n), dtype=np.int64)
        G[rows[strong], A.indices[strong]] = 1
        assert np.array_equal(G, G.T)                                 # (the strength graph of a symmetric matrix)
        reach = ((G + G @ G + np.eye(n, dtype=np.int64)) > 0)         # within two strong edges, itself included
        root = state == 2
        assert set(np.unique(state)) <= {0, 2} and root.any()
        assert (reach[np.ix_(root, root)].sum(axis=1) == 1).all(), "two roots within two strong edges"
        assert reach[:, root].any(axis=1).all(), "a node farther than two strong edges from every root"
        agg = lv["agg"]
        assert agg.shape == (n,) and agg.min() == 0 and agg.max() == lv["nagg"] - 1 == int(root.sum()) - 1
        assert np.array_equal(agg[root], np.arange(int(root.sum())))  # roots numbered in index order
        assert np.array_equal(np.unique(agg), np.arange(lv["nagg"]))
        # every node is within two strong edges of its aggregate's root
        root_of = np.flatnonzero(root)[agg]
        assert reach[np.arange(n), root_of].all()


def test_the_isolated_row_is_a_singleton():
    lv = hierarchy("isolated", coarse_max=16).levels[0]
    rows = np.repeat(np.arange(lv["A"].shape[0]), np.diff(lv["A"].indptr))
    assert not lv["strong"][rows == ISOLATED_ROW].any() and int(np.diff(lv["A"].indptr)[ISOLATED_ROW]) == 1
    assert lv["state"][ISOLATED_ROW] == 2
    assert int((lv["agg"] == lv["agg"][ISOLATED_ROW]).sum()) == 1
    P = lv["P"]
    lo, hi = P.indptr[ISOLATED_ROW], P.indptr[ISOLATED_ROW + 1]
    assert hi - lo == 1 and P.indices[lo] == lv["agg"][ISOLATED_ROW]


def test_the_hash_is_the_top_of_the_cell_field_word():
    """h30 is the top 30 bits of the word whose top 53 bits make the library's cell field (oracle.csr_ref.cell_field)."""
    idx = np.arange(1000)
    for seed in (1, 2, 12345):
        u53 = np.round((csr_ref.cell_field(idx, seed) - 0.5) * 2.0 ** 53).astype(np.uint64)
        assert np.array_equal(ref.h30(idx, seed), u53 >> np.uint64(23))
    assert len(np.unique(ref.h30(idx, 1))) > 990 and not np.array_equal(ref.h30(idx, 1), ref.h30(idx, 2))


# ------------------------------------------------------------------ hierarchy
@pytest.mark.parametrize("name", MATRICES)
def test_prolongator_pattern_and_galerkin_product(name):
    """Row i of P holds exactly the aggregates of i and of the stored entries of row i; the rows of T - (omega / lmax) D^-1 A T
    sum to what that matrix gives; A_1 equals the dense P' A P to a relative 1e-13 (two roundings per term over rows of at
    most 71 terms)."""
    H = hierarchy(name, coarse_max=16)
    for l, lv in enumerate(H.levels[:-1]):
        A, P, agg = lv["A"], lv["P"], lv["agg"]
        n = A.shape[0]
        for i in range(n):
            want = np.unique(np.concatenate([[agg[i]], agg[A.indices[A.indptr[i]:A.indptr[i + 1]]]]))
            assert np.array_equal(P.indices[P.indptr[i]:P.indptr[i + 1]], want), (l, i)
        Ad, Pd = A.to_dense(), P.to_dense()
        T = np.zeros((n, lv["nagg"]))
        T[np.arange(n), agg] = 1.0
        d = np.diag(Ad)
        want_p = T - ((4.0 / 3.0) / lv["lmax"]) * ((Ad @ T) / d[:, None])
        assert np.abs(Pd - want_p).max() <= 1e-14 * np.abs(want_p).max()
        assert np.array_equal(lv["R"].to_dense(), Pd.T)
        nxt = H.levels[l + 1]["A"].to_dense()
        want_a = Pd.T @ Ad @ Pd
        err = float(np.abs(nxt - want_a).max() / np.abs(want_a).max())
        print("%s level %d: |A_next - P' A P| / |P' A P| = %.3g" % (name, l + 1, err))
        assert err <= 1e-13
        assert np.array_equal(nxt != 0, nxt.T != 0)
    inv = H.inverse
    last = H.levels[-1]["A"].to_dense()
    assert inv is not None and np.abs(inv @ last - np.eye(len(last))).max() <= 1e-10


def test_the_stopping_rules():
    A = "poisson2d_13"
    assert len(hierarchy(A).levels) == 1 and hierarchy(A).inverse is not None          # 169 rows <= coarse_max = 256
    two = hierarchy(A, coarse_max=16, max_levels=2)
    assert len(two.levels) == 2 and two.inverse is None                                # the last level is larger: smoother alone
    full = hierarchy(A, coarse_max=16)
    assert len(full.levels) >= 3 and full.levels[-1]["A"].shape[0] <= 16
    assert [lv["A"].shape[0] for lv in two.levels] == [lv["A"].shape[0] for lv in full.levels[:2]]
    # a diagonal matrix has no strong entries: every node is a root, the level does not shrink
    D = csr_ref.from_coo(np.arange(40), np.arange(40), np.arange(1.0, 41.0), (40, 40))
    H = ref.build(D, coarse_max=16)
    assert len(H.levels) == 1 and H.levels[0]["nagg"] == 40 and H.inverse is None


def test_a_bad_diagonal_names_the_smallest_row():
    A = matrix("poisson2d_13")
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    for value in (-4.0, 0.0):
        data = np.where((rows == A.indices) & ((rows == 77) | (rows == 90)), value, A.data)
        with pytest.raises(ValueError, match="row 77 "):
            ref.build(csr_ref.RefCsr(A.indptr, A.indices, data, A.shape), coarse_max=16)
    keep = ~((rows == A.indices) & (rows == 5))
    with pytest.raises(ValueError, match="row 5 "):
        ref.build(csr_ref.from_coo(rows[keep], A.indices[keep], A.data[keep], A.shape), coarse_max=16)


# ------------------------------------------------------------------ iterations
def test_it_preconditions_cg():
    """Restated CG to a relative residual of 1e-10 on poisson2d(100), b = A ones: fewer than a quarter of the iterations with the
    default AMG cycle (DESIGN.md 3.11 has the counts)."""
    A = matrix("poisson2d_100")
    b = A.matvec(np.ones(A.shape[0]))
    x0, plain = ref.pcg(A, b)
    H = hierarchy("poisson2d_100")
    x1, with_amg = ref.pcg(A, b, H)
    print("poisson2d(100): %d iterations without, %d with AMG; levels %s, operator complexity %.3f"
          % (plain, with_amg, [lv["A"].shape[0] for lv in H.levels], H.operator_complexity))
    assert with_amg * 4 < plain
    assert np.abs(x1 - 1.0).max() <= 1e-7 and np.abs(x0 - 1.0).max() <= 1e-7
