"""What the GPU tests at the documented limits (tests/test_gpu_limits.py) rely on, asserted without a GPU: the table of
tests/_limits.py names every `MK_..._MAX...` macro of include/mikrylov.h with its value and an existing test; every restatement,
run in the device's summation order with the arguments of its GPU case, reaches the limit before it ends -- a full first cycle
of GMRES, a full cycle of IDR behind the build-up, a restart of the Lanczos loops, a third LOBPCG iteration, a wrapped L-BFGS
ring, a dense AMG level of several rows per lane, a split ILU run --; and `_ilu_ref.plan` against plans written out by hand."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests import _cheb_ref as cheb_ref, _ilu_ref as ilu_ref, _limits as lm

TESTS = os.path.join(ROOT, "tests")


def header_limits(text):
    """Every `#define MK_<...>_MAX<...> <integer>` of the header."""
    return {name: int(value) for name, value in re.findall(r"^#define\s+(MK_\w*_MAX\w*)\s+(\d+)\b", text, flags=re.M)}


# ------------------------------------------------------------------------------------------------ the table
def test_every_limit_of_the_header_has_a_test_at_its_value():
    with open(os.path.join(ROOT, "include", "mikrylov.h")) as f:
        found = header_limits(f.read())
    assert {"MK_GMRES_MAX_RESTART", "MK_IDR_MAX_S", "MK_TRLAN_MAX_NCV", "MK_LOBPCG_MAX_BLOCK", "MK_LBFGS_MAX_PAIRS",
            "MK_CHEB_MAX_DEGREE", "MK_AMG_MAX_COARSE", "MK_FSAI_MAX_ROW", "MK_MSCG_MAX_SHIFTS"} <= set(found)
    rows = {macro: (value, where) for macro, value, where in lm.LIMITS}
    assert len(rows) == len(lm.LIMITS)
    assert set(rows) == set(found), (sorted(set(found) - set(rows)), sorted(set(rows) - set(found)))
    for macro, (value, where) in rows.items():
        assert value == found[macro], (macro, value, found[macro])
        named = re.findall(r"(test_\w+\.py)::(test_\w+)", where)
        assert named, (macro, where)
        for f, t in named:
            with open(os.path.join(TESTS, f)) as src:
                assert "def %s(" % t in src.read(), (macro, f, t)


def test_the_header_parser_takes_the_limit_macros_only():
    text = "#define MK_A_MAX_B 7\n#define MK_VERSION 100\n  #define MK_C_MAX 9\n#define MK_D_MAX_E 12 /* note */\n#define MK_MAXIMUM 3\n"
    assert sorted(header_limits(text).items()) == [("MK_A_MAX_B", 7), ("MK_D_MAX_E", 12)]


def test_the_limits_inside_the_ilu_kernels_file():
    with open(os.path.join(ROOT, "pykrylov_amd", "csrc", "mk_ilu.hip")) as f:
        text = f.read()
    consts = dict(re.findall(r"constexpr int (MK_ILU_\w+) = (\d+);", text))
    assert int(consts["MK_ILU_RUN_MAX"]) == lm.ILU_RUN_MAX == ilu_ref.RUN_MAX
    assert int(consts["MK_ILU_FUSE_DEFAULT"]) == lm.ILU_FUSE_DEFAULT
    assert lm.ILU_BLOCK == ilu_ref.BLOCK == 256


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("reorth", [True, False], ids=["cgs2", "cgs1"])
@pytest.mark.parametrize("restart", lm.GMRES_RESTARTS)
def test_gmres_fills_its_first_cycle_and_restarts(restart, reorth):
    want = lm.gmres_reference(restart, reorth)
    assert not want.converged and want.restarts == 1 and want.nMatvec == lm.GMRES_ARGS["matvec_max"]
    assert want.last_steps >= 1 and want.nIter == restart + want.last_steps          # the first cycle ran all its steps
    assert np.isfinite(want.history).all() and np.isfinite(want.x).all()


@pytest.mark.parametrize("s", lm.IDR_S)
def test_idr_runs_a_full_cycle_behind_the_build_up(s):
    want = lm.idr_reference(s)
    assert want.s == s and want.breakdown == 0 and want.nMatvec > 2 * s and want.cycles >= 1
    assert np.isfinite(want.history).all()


@pytest.mark.parametrize("which", ["SA", "LA"])
def test_trlan_restarts_once_from_a_full_basis(which):
    want = lm.trlan_reference(which)
    assert want.cycles >= 2 and not want.breakdown and (want.ncv, want.keep) == (lm.TRLAN_NCV, lm.TRLAN_KEEP)
    assert want.keep % 16 != 0 and want.nMatvec == lm.TRLAN_ARGS["matvec_max"]
    assert want.nIter == want.nMatvec and np.isfinite(want.X).all()


@pytest.mark.parametrize("reorth", ["full", "one-sided"])
def test_trsvd_restarts_once_from_a_full_basis(reorth):
    want = lm.trsvd_reference(reorth)
    R, C = lm.trsvd_matrix().shape
    assert R % 2 == 1 and C % 2 == 1 and R > C >= lm.TRSVD_NCV
    assert want.cycles >= 2 and want.breakdown == 0 and (want.ncv, want.keep) == (lm.TRSVD_NCV, lm.TRSVD_KEEP)
    assert want.keep % 16 != 0 and want.nMatvec == lm.TRSVD_ARGS["matvec_max"] and 2 * want.nIter == want.nMatvec
    assert np.isfinite(want.U).all() and np.isfinite(want.V).all()


@pytest.mark.parametrize("block", lm.LOBPCG_BLOCKS)
def test_lobpcg_works_on_three_full_blocks(block):
    want = lm.lobpcg_reference(block)
    n = lm.lob.matrix(lm.LOBPCG_MATRIX).shape[0]
    assert n // 3 >= 16 and want.block == block
    assert want.nIter >= 3 and not want.breakdown and want.restarts == 0             # (a restart solves without P)
    assert list(want.actives[:3]) == [block] * 3                                     # no column locked: S has 3 x block columns
    assert np.isfinite(want.X).all()


@pytest.mark.parametrize("npairs", lm.LBFGS_NPAIRS)
def test_lbfgs_rings_are_full_and_wrapped(npairs):
    assert lm.LBFGS_POOL >= max(lm.LBFGS_NPAIRS) + 6 and lm.LBFGS_POOL >= npairs + max(lm.LBFGS_WRAPS)
    for scaling in (False, True):
        for wrap in lm.LBFGS_WRAPS:
            R, hv, cv, c1 = lm.lbfgs_reference(npairs, scaling, wrap)
            assert sum(t is not None for t in R.ys) == npairs and R.insert == wrap % npairs != 0
            assert np.isfinite(hv).all() and np.isfinite(cv).all() and np.isfinite(c1).all()
            assert (R.gamma != 1.0) == scaling


def test_chebyshev_applies_at_the_degree_limits_are_finite():
    from test_gpu_cheb import matrix
    from test_gpu_chebfilt import SIDES, applied, matrix as filter_matrix
    A = matrix(lm.CHEB_MATRIX)
    x = np.random.default_rng(11).standard_normal(A.shape[0])
    for scaled in (False, True):
        lmin, lmax = cheb_ref.interval(A, scale_diag=scaled)
        z = cheb_ref.apply(A, x, max(lm.CHEB_DEGREES), lmin, lmax, scaled)
        assert np.isfinite(z).all() and z.any()
    F = filter_matrix(lm.FILTER_MATRIX)
    for side in SIDES:
        y = applied(lm.FILTER_MATRIX, F, side, max(lm.FILTER_DEGREES))[1]
        assert np.isfinite(y).all() and y.any()


@pytest.mark.parametrize("name,rows", lm.AMG_CASES)
def test_amg_ends_in_a_dense_level_of_several_rows_per_lane(name, rows):
    A, H, x, z = lm.amg_reference(name)
    assert tuple(lv["A"].shape[0] for lv in H.levels) == rows
    assert 256 < rows[-1] <= lm.AMG_COARSE_MAX and H.inverse is not None and H.inverse.shape == (rows[-1], rows[-1])
    assert np.isfinite(z).all()
    assert max(r[-1] for _, r in lm.AMG_CASES) == lm.AMG_COARSE_MAX                # one case sits at the limit itself


# ------------------------------------------------------------------------------------------------ the ILU launch plans
PROFILE_17 = list(range(1, 18)) + list(range(16, 0, -1))     # the level widths of poisson2d(17): 1 .. 17 .. 1


def test_plan_against_plans_written_by_hand():
    plan = ilu_ref.plan
    assert plan([1] * 4500, 256) == [(0, 2048, 1), (2048, 4096, 1), (4096, 4500, 1)]
    assert plan([1] * 4096, 256) == [(0, 2048, 1), (2048, 4096, 1)]
    assert plan([1] * 2049, 1) == [(0, 2048, 1), (2048, 2049, 1)]
    assert plan(PROFILE_17, 16) == [(0, 16, 1), (16, 17, 1), (17, 33, 1)]
    assert plan(PROFILE_17, 17) == [(0, 33, 1)]
    assert plan(PROFILE_17, 1) == [(0, 1, 1)] + [(L, L + 1, 1) for L in range(1, 32)] + [(32, 33, 1)]
    assert plan(PROFILE_17, 0) == [(L, L + 1, 1) for L in range(33)]
    assert plan([600], 600) == [(0, 1, 1)] and plan([600], 0) == plan([600], 256) == [(0, 1, 3)]
    assert plan([256, 257, 256, 512, 513], 256) == [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 5, 3)]
    assert plan([3, 2, 300, 1, 1], 256) == [(0, 2, 1), (2, 3, 2), (3, 5, 1)]
    assert plan([], 256) == []


@pytest.mark.parametrize("name,fuse,launches", lm.ILU_CASES)
def test_ilu_cases_have_the_levels_their_plans_need(name, fuse, launches):
    for kind in ("ilu0", "ic0"):
        A, vals, wf, wb, x, z = lm.ilu_reference(name, kind)
        assert np.isfinite(vals).all() and np.isfinite(z).all()
        assert sum(wf) == sum(wb) == A.shape[0]
        f = lm.ILU_FUSE_DEFAULT if fuse is None else fuse
        for w in (wf, wb):
            assert len(ilu_ref.plan(w, f)) == launches, (name, fuse, kind)
            if name == "poisson1d_4500":
                assert list(w) == [1] * 4500 and len(w) > 2 * lm.ILU_RUN_MAX
            elif name == "poisson2d_17":
                assert list(w) == PROFILE_17
            else:
                assert list(w) == [600] and 600 % lm.ILU_BLOCK != 0 and 600 > 2 * lm.ILU_BLOCK
