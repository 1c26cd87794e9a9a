"""Multi-shift CG without a device: the NumPy restatement of the device loop (tests/_mscg_ref.py) solves every shifted system
to the threshold it claims, is PCG's restatement bit for bit at a zero shift, takes a negative shift, leaves a frozen shift
alone; the host-side checks of `pykrylov_amd.ShiftedCG` run before any device is touched; the kind and the shift limit are in
the header and in the ctypes mirror, and no function was added for them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import csr_ref
from tests import _mscg_ref as ref
from tests import _pcg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MAT, _RUN = {}, {}


def matrix(name):
    if name not in _MAT:
        if name == "1138bus":
            _MAT[name] = csr_ref.read_matrix_market(os.path.join(ROOT, "tests", "golden", "1138bus.mtx"))
        else:
            _MAT[name] = csr_ref.poisson2d(int(name[10:]))
    return _MAT[name]


def rhs_of(A):
    return A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


CASES = {"poisson2d_30": ((0.0, 1e-3, 1e-2, 0.1, 0.5, 1.0, 2.0, 4.0, 10.0), 1e-10),
         "1138bus": ((0.0, 0.01, 0.1, 1.0, 10.0, 100.0, 1000.0), 1e-8)}


def run(name):
    """One run of the restatement per problem, shared by the tests and never changed by them."""
    if name not in _RUN:
        A = matrix(name)
        shifts, reltol = CASES[name]
        b = rhs_of(A)
        _RUN[name] = (A, b, ref.mscg(A, b, shifts, abstol=0.0, reltol=reltol, matvec_max=20 * A.shape[0]))
    return _RUN[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_restatement_solves_every_shifted_system(name):
    """True residuals against 4 x threshold (the margin between the recurrence's and the true residual)."""
    A, b, got = run(name)
    shifts = CASES[name][0]
    assert got.converged and got.breakdown == 0 and got.definite and got.nMatvec == got.nIter
    worst = 0.0
    for k, s in enumerate(shifts):
        true = np.linalg.norm(b - (A.matvec(got.xs[k]) + s * got.xs[k]))
        worst = max(worst, true / got.threshold)
        assert true <= 4.0 * got.threshold, (name, s, true, got.threshold)
        assert got.residNorms[k] <= got.threshold
    print("%s: %d passes, freezes at %s, largest true residual %.3f x threshold"
          % (name, got.nIter, list(got.shiftIters), worst))
    # a larger shift is a better conditioned system: it never freezes later, and the last freeze ends the run
    assert all(a >= b_ for a, b_ in zip(got.shiftIters[:-1], got.shiftIters[1:])), got.shiftIters
    assert got.shiftIters[0] == got.nIter and got.shiftIters[-1] < got.shiftIters[0] and got.shiftIters.min() >= 1
    assert len(got.history) == len(got.history2) == got.nIter + 1
    assert same(got.history2[0], got.history[0]) and np.all(got.history2 <= got.history)      # |zeta_k| <= 1 for sigma >= 0
    assert np.all(np.abs(got.zeta) <= 1.0) and got.zeta[0] == 1.0
    assert same(got.residNorm, got.residNorms.max())


@pytest.mark.parametrize("m", [12, 31])
def test_a_zero_shift_is_pcg_without_a_preconditioner_bit_for_bit(m):
    A = matrix("poisson2d_%d" % m)
    b = rhs_of(A)
    for kw in (dict(abstol=0.0, reltol=1e-10), dict(reltol=1e-14, matvec_max=7)):
        got = ref.mscg(A, b, [0.0], **kw)
        want = _pcg_ref.pcg(A, b, precon=None, **kw)
        assert (got.nMatvec, got.nIter, got.converged, got.definite, got.breakdown) == \
            (want.nMatvec, want.nIter, want.converged, want.definite, want.breakdown)
        assert same(got.x, want.x) and same(got.history, want.history) and same(got.history2, want.history)
        assert same(got.residNorm, want.residNorm) and got.zeta[0] == 1.0
    # ... and duplicates are independent columns with the same bits, beside another shift too
    one = ref.mscg(A, b, [0.0], abstol=0.0, reltol=1e-10)
    two = ref.mscg(A, b, [0.0, 0.5, 0.0], abstol=0.0, reltol=1e-10)
    assert same(two.xs[0], two.xs[2]) and same(two.xs[0], one.x) and same(two.history, one.history)


def test_a_negative_shift_that_keeps_the_matrix_definite():
    A = matrix("poisson2d_20")
    m = 20
    lam_min = 8.0 * np.sin(np.pi / (2 * (m + 1))) ** 2          # smallest eigenvalue of the 5-point Laplacian on m x m
    dense = np.zeros(A.shape)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    dense[rows, A.indices] = A.data
    assert abs(np.linalg.eigvalsh(dense)[0] - lam_min) <= 1e-12
    b = rhs_of(A)
    shifts = [-0.5 * lam_min, 0.0, 1.0]
    got = ref.mscg(A, b, shifts, abstol=0.0, reltol=1e-10)
    assert got.converged and got.breakdown == 0
    assert abs(got.zeta[0]) > 1.0 and got.zeta[1] == 1.0 and abs(got.zeta[2]) < 1.0
    assert got.shiftIters[0] >= got.shiftIters[1] >= got.shiftIters[2] >= 1
    for k, s in enumerate(shifts):
        assert np.linalg.norm(b - (A.matvec(got.xs[k]) + s * got.xs[k])) <= 4.0 * got.threshold


def test_a_frozen_shift_is_left_alone():
    """x_k and p_k of a frozen shift are those of a run stopped by matvec_max at its freeze pass."""
    A, b, full = run("poisson2d_30")
    shifts, reltol = CASES["poisson2d_30"]
    for k in (len(shifts) - 1, 4):
        at = int(full.shiftIters[k])
        assert 1 <= at < full.nIter
        cut = ref.mscg(A, b, shifts, abstol=0.0, reltol=reltol, matvec_max=at)
        assert cut.nMatvec == cut.nIter == at and not cut.converged
        assert same(cut.xs[k], full.xs[k]) and same(cut.ps[k], full.ps[k])
        assert cut.shiftIters[k] == at and same(cut.zeta[k], full.zeta[k]) and same(cut.residNorms[k], full.residNorms[k])
        assert not same(cut.xs[0], full.xs[0])


def test_halts_and_breakdowns_of_the_restatement():
    A = matrix("poisson2d_12")
    n = A.shape[0]
    b = rhs_of(A)
    z = ref.mscg(A, np.zeros(n), [0.0, 1.0])
    assert z.converged and z.nMatvec == 0 and not z.xs.any() and list(z.shiftIters) == [0, 0] and list(z.history) == [0.0]
    for mm in (0, 1, 7):
        got = ref.mscg(A, b, [0.0, 1.0, 50.0], reltol=1e-14, matvec_max=mm)
        assert got.nMatvec == mm == got.nIter and not got.converged
    neg = csr_ref.RefCsr(A.indptr, A.indices, -A.data, A.shape)
    got = ref.mscg(neg, b, [0.0, 1.0])
    assert got.breakdown == 1 and not got.definite and got.nMatvec == 1 and got.nIter == 0 and not got.xs.any() and same(got.p, b)
    # c I and sigma = -c: 1 + sigma alpha is exactly zero in the first pass
    c = 4.0
    D = csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, c), (5, 5))
    got = ref.mscg(D, np.arange(1.0, 6.0), [1.0, -c])
    assert got.breakdown == 2 and got.definite and got.nMatvec == 1 and got.nIter == 0 and not got.xs.any()
    assert not got.converged and list(got.shiftIters) == [-1, -1]


class Op(object):
    """An operator that never saw the device."""
    shape = (10, 10)

    def __mul__(self, x):
        return x


class Part(Op):
    shape = (20, 20)
    local_size = 10


class Wide(Op):
    shape = (10, 12)


def test_host_side_checks_run_before_any_device_is_touched():
    from pykrylov_amd import ShiftedCG
    b = np.ones(10)
    for shifts in ([], [0.1] * 33, [0.0, float("nan")], [float("inf")], None):
        with pytest.raises(ValueError, match="shift"):
            ShiftedCG(Op()).solve(b, shifts)
    with pytest.raises(ValueError, match="preconditioner"):
        ShiftedCG(Op(), precon=Op()).solve(b, [0.0])
    with pytest.raises(ValueError, match="guess"):
        ShiftedCG(Op()).solve(b, [0.0], guess=np.zeros(10))
    with pytest.raises(ValueError, match="square"):
        ShiftedCG(Wide()).solve(b, [0.0])
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        ShiftedCG(Part()).solve(b, [0.0])


def test_the_kind_and_the_limit_are_in_the_header_and_no_function_was_added():
    from pykrylov_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    assert _lib.MK_MSCG == 14 and re.search(r"\bMK_MSCG = 14\b", hdr) and "MK_PCG = 13" in hdr
    assert _lib.MK_MSCG_MAX_SHIFTS == 32 and re.search(r"#define MK_MSCG_MAX_SHIFTS 32\b", hdr)
    assert not [name for name in _lib.PROTOTYPES if "mscg" in name.lower()]
    assert not re.search(r"\bmk_\w*mscg\w*\s*\(", hdr)
    # the shifts travel in a longer block whose head is the unchanged mk_params
    assert re.search(r"\}\s*mk_params_shifts;", hdr)
    blk = _lib.MkParamsShifts()
    assert len(blk.sigma) == _lib.MK_MSCG_MAX_SHIFTS and _lib.MkParamsShifts.base.offset == 0
    assert _lib.MkParamsShifts.nsigma.offset == ctypes.sizeof(_lib.MkParams)
    assert _lib.MkParamsShifts.sigma.offset == ctypes.sizeof(_lib.MkParams) + 8
    assert ctypes.sizeof(blk) == ctypes.sizeof(_lib.MkParams) + 8 + 8 * _lib.MK_MSCG_MAX_SHIFTS


def test_the_long_block_has_the_layout_the_c_compiler_gives_it(tmp_path):
    from pykrylov_amd import _lib
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mikrylov.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(mk_params_shifts), offsetof(mk_params_shifts, base),'
                   'offsetof(mk_params_shifts, nsigma), offsetof(mk_params_shifts, sigma));return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = _lib.MkParamsShifts
    assert got == [ctypes.sizeof(T), T.base.offset, T.nsigma.offset, T.sigma.offset]
