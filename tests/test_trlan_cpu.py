"""Thick-restart Lanczos without a device: the restatement of the library's Jacobi solver of the small eigenproblem against
LAPACK; the NumPy restatement of the device loop (tests/_trlan_ref.py) against dense eigenvalues on matrices with a simple
extreme spectrum, with its slow and edge cases; the host-side checks of `pykrylov_amd.ThickRestartLanczos`, which run before
any device is touched; the kind, the constant and the second long parameter block in the header."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import csr_ref
from tests import _trlan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

_MAT, _EIG = {}, {}


def matrix(name):
    if name not in _MAT:
        _MAT[name] = {"varcoef_7_5_3": lambda: csr_ref.poisson3d_varcoef(7, 5, 3),
                      "varcoef_20_20_5": lambda: csr_ref.poisson3d_varcoef(20, 20, 5),
                      "poisson3d_9_7_5": lambda: csr_ref.poisson3d(9, 7, 5),
                      "poisson1d_300": lambda: csr_ref.poisson1d(300),
                      "1138bus": lambda: csr_ref.read_matrix_market(os.path.join(GOLDEN, "1138bus.mtx")),
                      "2.5I_5": lambda: csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, 2.5), (5, 5))}[name]()
    return _MAT[name]


def dense_eigs(name):
    if name not in _EIG:
        _EIG[name] = np.linalg.eigvalsh(matrix(name).to_dense())
    return _EIG[name]


# ---------------------------------------------------------------------------------------------- the Jacobi restatement
def _small_matrices():
    rng = np.random.default_rng(11)
    out = [("1x1", np.array([[3.5]])), ("diagonal", np.diag(rng.standard_normal(17))), ("zero", np.zeros((6, 6)))]
    for m in (2, 3, 9, 24, 40):
        B = rng.standard_normal((m, m))
        out.append(("random_%d" % m, B + B.T))
    for m, k in ((8, 4), (16, 10), (32, 20), (40, 28)):          # what a restart leaves: diag, an arrow, a tridiagonal tail
        T = np.zeros((m, m))
        T[np.arange(k), np.arange(k)] = np.sort(rng.random(k))
        T[k, :k] = T[:k, k] = 1e-3 * rng.standard_normal(k)
        for j in range(k, m):
            T[j, j] = 2.0 + rng.random()
            if j + 1 < m:
                T[j, j + 1] = T[j + 1, j] = 1.0 + rng.random()
        out.append(("arrow_%d_%d" % (m, k), T))
    rep = np.diag([1.0, 1.0, 2.0, 2.0, 2.0])                     # repeated eigenvalues, coupled
    Q = np.linalg.qr(rng.standard_normal((5, 5)))[0]
    M = Q @ rep @ Q.T
    out.append(("repeated", 0.5 * (M + M.T)))
    return out


@pytest.mark.parametrize("name,T", _small_matrices(), ids=[nm for nm, _ in _small_matrices()])
def test_jacobi_restatement_against_lapack(name, T):
    theta, S, sweeps = ref.jacobi_eigh(T)
    m = T.shape[0]
    norm = np.linalg.norm(T, 2)
    want = np.linalg.eigvalsh(T)
    assert 1 <= sweeps <= 30
    assert np.all(np.diff(theta) >= 0)
    assert np.max(np.abs(theta - want)) <= 1e-13 * norm, (name, np.max(np.abs(theta - want)), norm)
    assert np.max(np.abs(S.T @ S - np.eye(m))) <= 1e-13
    assert np.max(np.abs(T @ S - S * theta[None, :])) <= 1e-13 * max(norm, 1.0) * m


def test_jacobi_sorts_ties_by_index_and_is_deterministic():
    theta, S, sweeps = ref.jacobi_eigh(np.diag([2.0, 1.0, 2.0, 1.0]))
    assert sweeps == 1 and list(theta) == [1.0, 1.0, 2.0, 2.0]
    assert np.array_equal(S, np.eye(4)[:, [1, 3, 0, 2]])
    rng = np.random.default_rng(2)
    B = rng.standard_normal((12, 12))
    a, b = ref.jacobi_eigh(B + B.T), ref.jacobi_eigh(B + B.T)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------------------------------------- the loop restatement
SIZES = [(1, 8), (4, 16), (8, 32), (16, 40)]
CASES = [(nm, w, nev, ncv) for nm in ("varcoef_7_5_3", "varcoef_20_20_5", "poisson3d_9_7_5") for w in ("SA", "LA")
         for nev, ncv in SIZES]
CASES += [("poisson1d_300", w, nev, ncv) for w in ("SA", "LA") for nev, ncv in SIZES[2:]]
CASES += [("1138bus", "LA", nev, ncv) for nev, ncv in SIZES]


def check_pairs(name, r, which, nev, reltol):
    A = matrix(name)
    ev = dense_eigs(name)
    lam = ev[-1]
    want = ev[:nev] if which == "SA" else ev[-nev:]
    assert r.converged and r.nconv == nev and not r.breakdown
    assert r.w.shape == (nev,) and r.X.shape == (nev, A.shape[0])
    assert np.max(np.abs(r.w - want)) <= 1e-12 * lam, np.max(np.abs(r.w - want)) / lam
    true = np.array([np.linalg.norm(A.matvec(r.X[i]) - r.w[i] * r.X[i]) for i in range(nev)])
    assert np.max(true) <= 2.0 * reltol * lam, np.max(true) / lam
    assert np.max(np.abs(r.residNorms - true)) <= 1e-10 * lam
    assert np.max(np.abs(r.X @ r.X.T - np.eye(nev))) <= 1e-12
    assert np.all(r.residNorms <= r.threshold) and np.all(r.pairIters >= 1) and np.all(r.pairIters <= r.cycles)
    assert len(r.history) == r.cycles and r.history[-1] == r.residNorm == np.max(r.residNorms)


@pytest.mark.parametrize("name,which,nev,ncv", CASES, ids=["%s-%s-%d-%d" % c for c in CASES])
def test_the_restatement_finds_the_extreme_pairs(name, which, nev, ncv):
    r = ref.trlan(matrix(name), nev, which, ncv=ncv, reltol=1e-10, abstol=0.0, matvec_max=2000)
    print(name, which, nev, ncv, "products", r.nMatvec, "cycles", r.cycles)
    assert r.nMatvec <= 2000 and r.nMatvec == r.nIter and r.ncv == ncv and r.keep == ref.default_keep(nev, ncv)
    check_pairs(name, r, which, nev, 1e-10)


def test_slow_case_runs_out_of_products_without_exceeding_them():
    r = ref.trlan(matrix("1138bus"), 4, "SA", ncv=16, reltol=1e-10, matvec_max=200)
    assert not r.converged and r.nMatvec <= 200 and r.residNorm > r.threshold and not r.breakdown
    assert r.nMatvec + (16 - r.keep) > 200                       # the next cycle did not fit
    assert r.w.shape == (4,) and np.all(np.diff(r.w) >= 0)


def test_breakdown_on_a_multiple_of_the_identity():
    A = matrix("2.5I_5")
    one = ref.trlan(A, 1, "SA", ncv=3)
    assert one.breakdown and one.converged and one.nIter == 1 and one.nMatvec == 1 and one.cycles == 1
    assert abs(one.w[0] - 2.5) <= 4 * 2.5 * 2.0 ** -52 and list(one.residNorms) == [0.0] and one.nconv == 1
    assert np.linalg.norm(A.matvec(one.X[0]) - 2.5 * one.X[0]) == 0.0
    two = ref.trlan(A, 2, "LA", ncv=3)
    assert two.breakdown and not two.converged and two.nconv == 1 and two.w.shape == (1,) and two.X.shape == (1, 5)


def test_a_basis_as_large_as_the_matrix_breaks_down_in_its_last_step():
    name = "varcoef_7_5_3"
    A = matrix(name)
    n = A.shape[0]
    r = ref.trlan(A, 4, "SA", ncv=n, reltol=1e-10)
    assert r.breakdown and r.converged and r.nIter == n and r.cycles == 1 and np.all(r.residNorms == 0.0)
    ev = dense_eigs(name)
    assert np.max(np.abs(r.w - ev[:4])) <= 1e-12 * ev[-1]
    true = [np.linalg.norm(A.matvec(r.X[i]) - r.w[i] * r.X[i]) for i in range(4)]
    assert max(true) <= 1e-10 * ev[-1]


def test_a_given_start_vector():
    name = "poisson3d_9_7_5"
    A = matrix(name)
    n = A.shape[0]
    v0 = np.cos(np.arange(n)) + 2.0
    r = ref.trlan(A, 4, "LA", ncv=16, start=v0, matvec_max=2000)
    assert r.residNorm0 == np.sqrt(np.dot(v0, v0))
    check_pairs(name, r, "LA", 4, 1e-10)
    other = ref.trlan(A, 4, "LA", ncv=16, matvec_max=2000)       # the hashed vector: another run
    assert other.history.tobytes() != r.history.tobytes()
    hashed = csr_ref.cell_field(np.arange(n), 1) - 1.0
    assert other.residNorm0 == np.sqrt(np.dot(hashed, hashed))


def test_argument_errors_of_the_restatement():
    A = matrix("varcoef_7_5_3")
    for kw in (dict(nev=0), dict(nev=8, ncv=8), dict(nev=2, ncv=106), dict(nev=4, ncv=16, keep=3), dict(nev=4, ncv=16, keep=16),
               dict(nev=4, ncv=16, matvec_max=15), dict(nev=2, which="SM")):
        with pytest.raises(ValueError):
            ref.trlan(A, **kw)
    with pytest.raises(ValueError):
        ref.trlan(csr_ref.poisson1d(300), 2, ncv=129)


# ---------------------------------------------------------------------------------------------- host logic
class Op(object):
    """An operator that never saw the device."""
    shape = (200, 200)

    def __mul__(self, x):
        return x


class Part(Op):
    shape = (400, 400)
    local_size = 200


class Wide(Op):
    shape = (200, 212)


class Unsym(Op):
    symmetric = False


def test_host_side_checks_run_before_any_device_is_touched(monkeypatch):
    from pykrylov_amd import ThickRestartLanczos, _lib, eigsh

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "init", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    with pytest.raises(ValueError, match="preconditioner"):
        ThickRestartLanczos(Op(), precon=Op()).solve(2)
    with pytest.raises(ValueError, match="square"):
        ThickRestartLanczos(Wide()).solve(2)
    with pytest.raises(ValueError, match="symmetric"):
        ThickRestartLanczos(Unsym()).solve(2)
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        ThickRestartLanczos(Part()).solve(2)
    for nev in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="nev"):
            ThickRestartLanczos(Op()).solve(nev)
    for ncv in (4, 3, 129, 201, 8.0):
        with pytest.raises(ValueError, match="ncv"):
            ThickRestartLanczos(Op()).solve(4, ncv=ncv)
    for keep in (3, 16, 17, 5.5):
        with pytest.raises(ValueError, match="keep"):
            ThickRestartLanczos(Op()).solve(4, ncv=16, keep=keep)
    for which in ("SM", "LM", "sa", None):
        with pytest.raises(ValueError, match="which"):
            ThickRestartLanczos(Op()).solve(4, which=which)
    for mm in (15, 0, -3, 1e3):
        with pytest.raises(ValueError, match="matvec_max"):
            ThickRestartLanczos(Op()).solve(4, ncv=16, matvec_max=mm)
    with pytest.raises(ValueError, match="start"):
        ThickRestartLanczos(Op()).solve(4, start=np.ones(199))
    with pytest.raises(ValueError, match="which"):
        eigsh(Op(), k=3, which="BE")


def test_defaults_of_ncv_and_keep():
    from pykrylov_amd import trlan
    assert [trlan.default_ncv(n, k) for n, k in ((1000, 1), (1000, 6), (1000, 10), (1000, 80), (15, 4), (30, 12))] == \
        [20, 20, 21, 128, 15, 25]
    assert [trlan.default_keep(k, m) for k, m in ((1, 20), (6, 20), (10, 21), (4, 5), (4, 16), (16, 40))] == [10, 13, 15, 4, 10, 28]
    for n, k in ((1000, 6), (50, 20), (10 ** 6, 60)):
        m = trlan.default_ncv(n, k)
        assert (m, trlan.default_keep(k, m)) == (ref.default_ncv(n, k), ref.default_keep(k, ref.default_ncv(n, k)))
    s = trlan.ThickRestartLanczos(Op())
    assert s.abstol == 0.0 and s.reltol == 1e-10
    assert trlan.ThickRestartLanczos(Op(), reltol=1e-6, abstol=1e-9).reltol == 1e-6


def test_the_kind_and_the_limit_are_in_the_header_and_no_function_was_added():
    from pykrylov_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    assert _lib.MK_TRLAN == 15 and re.search(r"\bMK_TRLAN = 15\b", hdr) and re.search(r"\bMK_MSCG = 14,", hdr)
    assert _lib.MK_TRLAN_MAX_NCV == 128 and re.search(r"#define MK_TRLAN_MAX_NCV 128\b", hdr)
    assert not [name for name in _lib.PROTOTYPES if "trlan" in name.lower() or "eig" in name.lower()]
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", code)
    assert declared and not [f for f in declared if "trlan" in f or "eig" in f]
    assert re.search(r"\}\s*mk_params_eig;", hdr)
    T = _lib.MkParamsEig
    base = ctypes.sizeof(_lib.MkParams)
    assert (T.base.offset, T.nev.offset, T.ncv.offset, T.which.offset, T.keep.offset, T.seed.offset) == \
        (0, base, base + 4, base + 8, base + 12, base + 16)
    assert ctypes.sizeof(T) == base + 24
    assert len({ctypes.sizeof(T), ctypes.sizeof(_lib.MkParamsShifts), base}) == 3      # struct_size tells the blocks apart


def test_the_eig_block_has_the_layout_the_c_compiler_gives_it(tmp_path):
    from pykrylov_amd import _lib
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mikrylov.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(mk_params_eig), offsetof(mk_params_eig, base),'
                   'offsetof(mk_params_eig, nev), offsetof(mk_params_eig, ncv), offsetof(mk_params_eig, which),'
                   'offsetof(mk_params_eig, keep), offsetof(mk_params_eig, seed), (int)MK_TRLAN, MK_TRLAN_MAX_NCV);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = _lib.MkParamsEig
    assert got == [ctypes.sizeof(T), T.base.offset, T.nev.offset, T.ncv.offset, T.which.offset, T.keep.offset, T.seed.offset,
                   _lib.MK_TRLAN, _lib.MK_TRLAN_MAX_NCV]
