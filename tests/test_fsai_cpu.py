"""The NumPy restatement of FSAI (tests/_fsai_ref.py) against the mathematics: every row of G is the normalised last row of
inv(A[P, P]), diag(G A G') = 1, the symbolic power is the boolean power, and G' G preconditions MINRES.  No device."""
import os

import numpy as np
import pytest

from oracle import csr_ref, krylov_ref as kr
from tests import _fsai_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MATRICES = ("poisson2d_12", "1138bus", "varcoef_20_20_5")


def matrix(name):
    if name == "poisson2d_12":
        return csr_ref.poisson2d(12)
    if name == "poisson2d_100":
        return csr_ref.poisson2d(100)
    if name == "1138bus":
        return csr_ref.read_matrix_market(os.path.join(GOLDEN, "1138bus.mtx"))
    if name == "varcoef_20_20_5":
        return csr_ref.poisson3d_varcoef(20, 20, 5)
    raise KeyError(name)


_G = {}


def factor(name, power):
    if (name, power) not in _G:
        A = matrix(name)
        _G[name, power] = (A, ref.factor(A, power=power))
    return _G[name, power]


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("name", MATRICES)
def test_rows_are_the_normalised_last_rows_of_the_local_inverses(name, power):
    """g_i = e_m' inv(A[P, P]) / sqrt((inv(A[P, P]))_mm) from numpy.linalg, to 1e-10 relative (in the row's largest
    entry)."""
    A, G = factor(name, power)
    D = A.to_dense()
    worst = 0.0
    for i in range(A.shape[0]):
        P = G.indices[G.indptr[i]:G.indptr[i + 1]]
        assert P[-1] == i and len(P) <= ref.MAX_ROW
        inv = np.linalg.inv(D[np.ix_(P, P)])
        want = inv[-1, :] / np.sqrt(inv[-1, -1])
        got = G.data[G.indptr[i]:G.indptr[i + 1]]
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print("%s power %d: largest relative row error %.3g" % (name, power, worst))
    assert worst <= 1e-10


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("name", MATRICES)
def test_the_diagonal_of_G_A_Gt_is_one(name, power):
    A, G = factor(name, power)
    Gd = G.to_dense()
    d = ((Gd @ A.to_dense()) * Gd).sum(axis=1)
    err = float(np.abs(d - 1.0).max())
    print("%s power %d: max |diag(G A G') - 1| = %.3g" % (name, power, err))
    assert err <= 1e-11


@pytest.mark.parametrize("name", MATRICES)
def test_the_power_2_pattern_is_the_lower_triangle_of_the_boolean_square(name):
    A = matrix(name)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    B = np.zeros(A.shape, dtype=bool)
    B[rows, A.indices] = True                                   # (the stored pattern: a stored zero is stored)
    want = np.tril((B.astype(np.int64) @ B.astype(np.int64)) > 0)
    ip, ix = ref.power_pattern(A.indptr, A.indices, 2)
    got = np.zeros(A.shape, dtype=bool)
    got[np.repeat(np.arange(A.shape[0]), np.diff(ip)), ix] = True
    assert np.array_equal(got, want) and int(ip[-1]) == int(want.sum())
    assert all(np.all(np.diff(ix[ip[i]:ip[i + 1]]) > 0) for i in range(A.shape[0]))
    ip1, ix1 = ref.power_pattern(A.indptr, A.indices, 1)
    assert np.array_equal(ip1, np.concatenate([[0], np.cumsum(np.tril(B).sum(axis=1))]))


def test_the_package_forms_the_same_symbolic_powers():
    """`tools._pattern_power` (NumPy, sorted keys) against the restatement's unions of rows, powers 2 and 3."""
    from pykrylov_amd.tools import _pattern_power
    for name in ("poisson2d_12", "1138bus"):
        A = matrix(name)
        for power in (2, 3):
            ip, ix = _pattern_power(A.indptr, A.indices, A.shape[0], power)
            rp, rx = ref.power_pattern(A.indptr, A.indices, power)
            assert np.array_equal(ip, rp) and np.array_equal(ix, rx), (name, power)


@pytest.mark.parametrize("name", ["poisson2d_100", "1138bus"])
def test_it_preconditions_minres(name):
    """MINRES, rtol = 1e-10, b = A ones: strictly fewer products with FSAI than without, and fewer with power 2 than with
    power 1.  (The ordering is asserted, not the counts.)"""
    A = matrix(name)
    b = A.matvec(np.ones(A.shape[0]))
    counts = []
    for precon in (None, ref.HostFsai(factor(name, 1)[1]), ref.HostFsai(factor(name, 2)[1])):
        out = kr.minres(A, b, precon=precon, check=False, etol=0.0, rtol=1e-10)
        assert out["istop"] in (1, 2), out["istop"]
        counts.append(int(out["nMatvec"]))
    print("MINRES %s: %d products without, %d with FSAI, %d with FSAI on the squared pattern" % ((name,) + tuple(counts)))
    assert counts[2] < counts[1] < counts[0]


def test_a_breakdown_names_the_smallest_row():
    A = csr_ref.poisson2d(12)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    data = np.where((rows == 77) & (A.indices == 77), -1.0, A.data)
    with pytest.raises(ValueError, match="row 77"):
        ref.factor(csr_ref.RefCsr(A.indptr, A.indices, data, A.shape))
