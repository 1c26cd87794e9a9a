"""LOBPCG without a device: the NumPy restatement of the device loop (tests/_lobpcg_ref.py) against the dense spectrum counted
with multiplicity, with and without the restated AMG preconditioner; soft locking, the Cholesky fallback and the edge cases;
the host-side checks of `pykrylov_amd.LOBPCG`, which run before any device is touched; the kind and the constant in the header,
with no function added to the C ABI."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import csr_ref
from tests import _amg_ref, _lobpcg_ref as ref, _trlan_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

_MAT, _EIG, _AMG = {}, {}, {}


def matrix(name):
    if name not in _MAT:
        _MAT[name] = {"poisson2d_20": lambda: csr_ref.poisson2d(20),
                      "poisson3d_9_7_5": lambda: csr_ref.poisson3d(9, 7, 5),
                      "varcoef_7_5_3": lambda: csr_ref.poisson3d_varcoef(7, 5, 3),
                      "varcoef_20_20_5": lambda: csr_ref.poisson3d_varcoef(20, 20, 5),
                      "poisson1d_300": lambda: csr_ref.poisson1d(300),
                      "1138bus": lambda: csr_ref.read_matrix_market(os.path.join(GOLDEN, "1138bus.mtx")),
                      "2.5I_6": lambda: csr_ref.from_coo(np.arange(6), np.arange(6), np.full(6, 2.5), (6, 6))}[name]()
    return _MAT[name]


def dense_eigs(name):
    if name not in _EIG:
        _EIG[name] = np.linalg.eigvalsh(matrix(name).to_dense())
    return _EIG[name]


def amg(name):
    if name not in _AMG:
        M = _amg_ref.build(matrix(name))
        _AMG[name] = lambda r: M * r
    return _AMG[name]


# ---------------------------------------------------------------------------------------------- accuracy
SIZES = [(1, 2), (4, 8), (8, 12)]
CASES = []
for _nm in ("poisson2d_20", "poisson3d_9_7_5", "varcoef_7_5_3", "varcoef_20_20_5", "poisson1d_300", "1138bus"):
    for _nev, _nb in SIZES + ([(16, 16)] if _nm in ("poisson2d_20", "poisson3d_9_7_5") else []):
        for _which, _pre in (("SA", False), ("SA", True), ("LA", False)):
            if _nm == "1138bus" and _which == "SA" and not _pre:
                continue                                         # (asserted not to converge, below)
            if _nm == "poisson1d_300" and (_nev, _nb) == (1, 2) and not _pre:
                continue                                         # (needs more than 400 iterations)
            CASES.append((_nm, _which, _nev, _nb, _pre))


def check_pairs(name, r, which, nev, reltol):
    A = matrix(name)
    ev = dense_eigs(name)
    lam = ev[-1]
    want = ev[:nev] if which == "SA" else ev[-nev:]              # counted with multiplicity
    assert r.converged and r.nconv == nev and not r.breakdown
    assert r.w.shape == (nev,) and r.X.shape == (nev, A.shape[0])
    true = np.array([np.linalg.norm(A.matvec(r.X[i]) - r.w[i] * r.X[i]) for i in range(nev)])
    print(name, which, nev, "eigenvalue error", np.max(np.abs(r.w - want)) / lam, "true residual", np.max(true) / lam,
          "|residNorms - true|", np.max(np.abs(r.residNorms - true)) / lam, "orthonormality",
          np.max(np.abs(r.X @ r.X.T - np.eye(nev))))
    assert np.max(np.abs(r.w - want)) <= 1e-12 * lam
    assert np.max(true) <= 2.0 * reltol * lam
    assert np.max(np.abs(r.residNorms - true)) <= 1e-10 * lam
    assert np.max(np.abs(r.X @ r.X.T - np.eye(nev))) <= 1e-12
    assert np.all(r.residNorms <= r.threshold) and np.all(r.pairIters >= 0) and np.all(r.pairIters <= r.nIter)
    assert len(r.history) == r.nIter + 1 and r.history[-1] == r.residNorm == np.max(r.residNorms)


@pytest.mark.parametrize("name,which,nev,nb,pre", CASES, ids=["%s-%s-%d-%d-%s" % (c[:4] + ("amg" if c[4] else "none",)) for c in CASES])
def test_the_restatement_finds_the_extreme_pairs_with_multiplicity(name, which, nev, nb, pre):
    cap = 400 * nb + nb                                          # room for 400 iterations
    r = ref.lobpcg(matrix(name), nev, which, block=nb, reltol=1e-10, abstol=0.0, matvec_max=cap,
                   precon=amg(name) if pre else None)
    print(name, which, nev, nb, pre, "iterations", r.nIter, "products", r.nMatvec, "restarts", r.restarts)
    assert r.nIter <= 400 and r.nMatvec <= cap and r.nMatvec == nb + sum(r.actives) and r.block == nb
    check_pairs(name, r, which, nev, 1e-10)


def test_without_a_preconditioner_the_smallest_end_of_1138bus_does_not_converge():
    r = ref.lobpcg(matrix("1138bus"), 4, "SA", block=8, reltol=1e-10, matvec_max=400 * 8)
    assert not r.converged and r.nMatvec <= 400 * 8 and r.residNorm > r.threshold and not r.breakdown
    assert r.nMatvec + r.actives[-1] > 400 * 8                   # the next iteration did not fit


def test_the_double_eigenvalue_is_found_twice_where_lanczos_finds_it_once():
    name = "poisson2d_20"
    ev = dense_eigs(name)
    lam = ev[-1]
    assert abs(ev[1] - ev[2]) <= 1e-13 * lam and ev[2] < ev[3] - 1e-3 * lam
    r = ref.lobpcg(matrix(name), 4, "SA", block=8, precon=amg(name))
    assert r.converged and np.max(np.abs(r.w - ev[:4])) <= 1e-12 * lam
    assert abs(r.w[1] - ev[1]) <= 1e-12 * lam and abs(r.w[2] - ev[2]) <= 1e-12 * lam
    t = _trlan_ref.trlan(matrix(name), 4, "SA", ncv=40, matvec_max=4000)
    assert t.converged and abs(t.w[1] - ev[1]) <= 1e-10 * lam
    assert abs(t.w[2] - ev[2]) > 1e-3 * lam                      # one copy only: its third value is a later eigenvalue


# ---------------------------------------------------------------------------------------------- soft locking, restarts
def test_soft_locking_goes_on_with_fewer_active_columns():
    name = "poisson2d_20"
    r = ref.lobpcg(matrix(name), 2, "SA", block=4, precon=amg(name))
    assert r.converged and r.nMatvec == 4 + sum(r.actives) and len(r.actives) == r.nIter
    assert r.actives[0] == 4 and min(r.actives) < 4 and all(a >= b for a, b in zip(r.actives, r.actives[1:]))
    guard = r.lockIters[2:]
    assert np.any((guard >= 0) & (guard < r.nIter))              # a guard column was locked before the last wanted pair
    assert r.lockIters[0] >= 0 and r.pairIters[0] == r.lockIters[0] and r.pairIters[1] == r.nIter
    check_pairs(name, r, "SA", 2, 1e-10)


def test_a_start_block_with_two_equal_columns_takes_the_fallback():
    A = matrix("varcoef_7_5_3")
    n = A.shape[0]
    X0 = np.cos(np.outer(np.arange(1, 5), np.arange(n))) + np.arange(4)[:, None]
    good = ref.lobpcg(A, 2, "SA", block=4, start=X0)
    assert good.converged and not good.breakdown
    X0[3] = X0[1]
    r = ref.lobpcg(A, 2, "SA", block=4, start=X0)
    assert r.breakdown or r.restarts > 0
    assert r.breakdown and not r.converged and r.nIter == 0 and r.nMatvec == 4
    assert np.all(np.isfinite(r.w)) and np.all(np.isfinite(r.residNorms)) and np.all(np.isfinite(r.X))
    X0[3] = X0[1] * (1.0 + 1e-9 * np.cos(np.arange(n)))          # nearly equal: the pivot test, not a zero pivot
    r = ref.lobpcg(A, 2, "SA", block=4, start=X0)
    assert (r.breakdown or r.restarts > 0 or r.converged) and np.all(np.isfinite(r.w))


# ---------------------------------------------------------------------------------------------- edge cases
def test_edge_cases():
    A = csr_ref.poisson1d(6)
    ev = np.linalg.eigvalsh(A.to_dense())
    r = ref.lobpcg(A, 1, "SA", block=2)                          # n = 6, nb = 2: the largest block n allows
    assert r.converged and abs(r.w[0] - ev[0]) <= 1e-12 * ev[-1]
    one = ref.lobpcg(matrix("2.5I_6"), 2, "SA", block=2)         # the first Rayleigh-Ritz step is exact
    assert one.converged and one.nIter == 0 and one.nMatvec == 2 and len(one.history) == 1 and list(one.pairIters) == [0, 0]
    assert np.max(np.abs(one.w - 2.5)) <= 4 * 2.5 * 2.0 ** -52
    with pytest.raises(ValueError):
        ref.lobpcg(matrix("varcoef_7_5_3"), 2, block=4, matvec_max=3)
    for cap in (4, 5, 11, 30):                                   # stops mid-run, never exceeded
        r = ref.lobpcg(matrix("varcoef_7_5_3"), 2, "SA", block=4, matvec_max=cap)
        assert not r.converged and r.nMatvec <= cap < r.nMatvec + 4 and r.nMatvec == 4 + 4 * r.nIter
    for kw in (dict(nev=0), dict(nev=5, block=4), dict(nev=2, block=17), dict(nev=2, block=36), dict(nev=2, which="SM"),
               dict(nev=2, which="LA", precon=lambda v: v)):
        with pytest.raises(ValueError):
            ref.lobpcg(matrix("varcoef_7_5_3"), **kw)


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


class Small(Op):
    shape = (30, 30)


def test_host_side_checks_run_before_any_device_is_touched(monkeypatch):
    from pykrylov_amd import LOBPCG, _lib, lobpcg

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "init", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    with pytest.raises(ValueError, match="square"):
        LOBPCG(Wide()).solve(2)
    with pytest.raises(ValueError, match="symmetric"):
        LOBPCG(Unsym()).solve(2)
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        LOBPCG(Part()).solve(2)
    for nev in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="nev"):
            LOBPCG(Op()).solve(nev)
    for block in (3, 17, 8.0, 67):                               # nev > block, block > 16, not an integer
        with pytest.raises(ValueError, match="block"):
            LOBPCG(Op()).solve(4, block=block)
    with pytest.raises(ValueError, match="block"):
        LOBPCG(Small()).solve(4, block=11)                       # block > n // 3
    for which in ("SM", "LM", "sa", None):
        with pytest.raises(ValueError, match="which"):
            LOBPCG(Op()).solve(4, which=which)
    with pytest.raises(ValueError, match="preconditioner"):
        LOBPCG(Op(), precon=Op()).solve(2, which="LA")
    with pytest.raises(ValueError, match="guess"):
        LOBPCG(Op()).solve(2, guess=np.ones(200))
    for mm in (7, 0, -3, 1e3):
        with pytest.raises(ValueError, match="matvec_max"):
            LOBPCG(Op()).solve(4, block=8, matvec_max=mm)
    for start in (np.ones(200), np.ones((8, 199)), np.ones((7, 200)), np.ones((200, 8))):
        with pytest.raises(ValueError, match="start"):
            LOBPCG(Op()).solve(4, block=8, start=start)
    with pytest.raises(ValueError, match="which"):
        lobpcg(Op(), k=3, which="BE")
    with pytest.raises(ValueError, match="X0"):
        lobpcg(Op(), k=3, X0=np.ones(200))


def test_defaults():
    import importlib
    mod = importlib.import_module("pykrylov_amd.lobpcg")     # (the package's `lobpcg` is the wrapper function)
    assert [mod.default_block(n, k) for n, k in ((1000, 1), (1000, 4), (1000, 6), (1000, 10), (1000, 16), (30, 4), (6, 1))] == \
        [3, 6, 9, 15, 16, 6, 2]
    for n, k in ((1000, 6), (50, 12), (10 ** 6, 16), (9, 2)):
        assert mod.default_block(n, k) == ref.default_block(n, k)
    assert mod.MAX_BLOCK == ref.MAX_BLOCK == 16
    s = mod.LOBPCG(Op())
    assert s.abstol == 0.0 and s.reltol == 1e-10 and s.precon is None and s.precon_route == "none"
    assert mod.LOBPCG(Op(), reltol=1e-6, abstol=1e-9).reltol == 1e-6


# ---------------------------------------------------------------------------------------------- the header
# every function the header declared before this solver kind was added (include/mikrylov.h of the parent commit)
DECLARED = """mk_amg_apply mk_amg_coarse mk_amg_create mk_amg_destroy mk_amg_download mk_amg_info mk_amg_level mk_arena_reserve mk_axpby
mk_axpy mk_build_info mk_calib_stream mk_cheb_apply mk_cheb_coefficients mk_cheb_create mk_cheb_destroy mk_cheb_info
mk_comm_allreduce_host mk_comm_destroy mk_comm_info mk_comm_init mk_comm_init_host mk_comm_time_allreduce mk_comm_time_exchange
mk_comm_transport mk_comm_unique_id mk_csr_col_range mk_csr_colblocks mk_csr_comm_last_us mk_csr_compose mk_csr_create
mk_csr_create_block mk_csr_create_callback mk_csr_create_product mk_csr_create_reduced mk_csr_create_sum mk_csr_destroy
mk_csr_download mk_csr_download_rows mk_csr_format_info mk_csr_from_coo mk_csr_lanczos mk_csr_launch_info mk_csr_localize
mk_csr_march_info mk_csr_overlap_info mk_csr_pencil_info mk_csr_poisson2d mk_csr_poisson3d mk_csr_poisson3d_varcoef
mk_csr_set_colblocks mk_csr_set_exchange mk_csr_set_format mk_csr_set_row_block mk_csr_set_tile_order mk_csr_shape
mk_csr_stencil27 mk_csr_tile_order mk_csr_transpose mk_device_info mk_dot mk_exchange mk_free mk_fsai_apply mk_fsai_create
mk_fsai_destroy mk_fsai_download mk_fsai_factors mk_fsai_info mk_ic0_create mk_ilu0_create mk_ilu_apply mk_ilu_destroy
mk_ilu_download mk_ilu_info mk_init mk_last_error mk_lbfgs_apply mk_lbfgs_create mk_lbfgs_destroy mk_lbfgs_download
mk_lbfgs_forward_combine mk_lbfgs_forward_dots mk_lbfgs_gram mk_lbfgs_info mk_lbfgs_restart mk_lbfgs_store mk_malloc
mk_memcpy_d2d mk_memcpy_d2h mk_memcpy_h2d mk_memset mk_nrm2 mk_scal mk_shutdown mk_solver_create mk_solver_destroy
mk_solver_finish mk_solver_fused mk_solver_history mk_solver_history2 mk_solver_iterate mk_solver_set_idr
mk_solver_set_lls_precon mk_solver_set_lls_precon_amg mk_solver_set_lls_precon_bfgs mk_solver_set_lls_precon_callback
mk_solver_set_lls_precon_cheb mk_solver_set_lls_precon_csr mk_solver_set_lls_precon_fsai mk_solver_set_lls_precon_ilu
mk_solver_set_pcg mk_solver_set_precon_amg mk_solver_set_precon_callback mk_solver_set_precon_cheb mk_solver_set_precon_csr
mk_solver_set_precon_diag mk_solver_set_precon_fsai mk_solver_set_precon_ilu mk_solver_set_precon_lbfgs mk_solver_set_transpose
mk_solver_setup mk_solver_solve mk_solver_time_product mk_solver_time_spmv mk_solver_timing mk_solver_unapplied mk_solver_vector
mk_solver_x mk_spmv mk_sync mk_version""".split()


def test_the_kind_and_the_limit_are_in_the_header_and_no_function_was_added():
    from pykrylov_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    assert _lib.MK_LOBPCG == 16 and re.search(r"\bMK_LOBPCG = 16\b", hdr) and re.search(r"\bMK_TRLAN = 15,", hdr)
    assert _lib.MK_LOBPCG_MAX_BLOCK == 16 and re.search(r"#define MK_LOBPCG_MAX_BLOCK 16\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", code)))
    assert len(DECLARED) == 132 and declared == sorted(DECLARED)
    assert sorted(_lib.PROTOTYPES) == sorted(DECLARED)
    assert not [f for f in declared if "lobpcg" in f or "gram" in f.replace("mk_lbfgs_gram", "")]
    structs = re.findall(r"\}\s*(mk_[a-z0-9_]+);", code)
    assert "mk_params_eig" in structs and not [t for t in structs if "lobpcg" in t]


def test_the_eig_block_keeps_its_size(tmp_path):
    from pykrylov_amd import _lib
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mikrylov.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %d %d\\n", sizeof(mk_params_eig), sizeof(mk_params),'
                   'offsetof(mk_params_eig, ncv), offsetof(mk_params_eig, seed), (int)MK_LOBPCG, MK_LOBPCG_MAX_BLOCK);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = _lib.MkParamsEig
    base = ctypes.sizeof(_lib.MkParams)
    assert got == [base + 24, base, base + 4, base + 16, 16, 16]
    assert ctypes.sizeof(T) == base + 24 and T.ncv.offset == base + 4 and T.seed.offset == base + 16
