"""The device loops and preconditioners AT the limits that include/mikrylov.h documents -- the values that size the LDS
arrays, the register accumulators and the launch plans -- and at the value below where that takes another path: GMRES(m) at a
restart of 127 and 128, IDR(s) at s = 31 and 32, the thick-restart Lanczos loops at a basis of 128, LOBPCG at a block of 15 and
16, the L-BFGS operators with 9, 63 and 64 pairs in a wrapped ring, the Chebyshev preconditioner applied at degree 63 and 64
and the filter at 127 and 128, AMG with a dense coarsest level of 289, 364 and 1024 rows, and ILU(0) / IC(0) with a run of
levels that is split, levels on either side of the fuse width, and a level wider than a workgroup inside a fused run.  Each
against its NumPy restatement in the device's summation order; floats are compared as bit patterns throughout.  The cases,
their restatements and what a case must reach before it ends are in tests/_limits.py, the latter asserted without a GPU by
tests/test_limits_cpu.py and again here.  No case hands a kernel a value beyond its limit."""
import numpy as np
import pytest

from oracle import gpu_order
from tests import _cheb_ref as cheb_ref, _ilu_ref as ilu_ref, _lbfgs_ref as lbfgs_ref, _limits as lm
import test_gpu_amg as amg
import test_gpu_cheb as cheb
import test_gpu_chebfilt as filt
import test_gpu_gmres as gm
import test_gpu_idr as idr
import test_gpu_lobpcg as lob
import test_gpu_trlan as tl
import test_gpu_trsvd as sv
from test_gpu_ilu import device_op, same
from test_gpu_lanczos import fmt_of, set_format
from test_gpu_lbfgs import ys_array

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1. GMRES(m)
@pytest.mark.parametrize("reorth", [True, False], ids=["cgs2", "cgs1"])
@pytest.mark.parametrize("restart", lm.GMRES_RESTARTS)
def test_gmres_at_the_restart_limit(restart, reorth):
    """A full first cycle -- 16 groups of 8 basis columns, or 15 and one of 7; the Givens arrays up to index 128; the back
    substitution from column 128 -- a restart, and a few steps of the second cycle."""
    want = lm.gmres_reference(restart, reorth)
    assert not want.converged and want.restarts == 1 and want.nIter == restart + want.last_steps
    A = gm.matrix(lm.GMRES_MATRIX)
    op = device_op(A, False)
    set_format(op, 0)
    s = gm.solve(op, gm.rhs_of(lm.GMRES_MATRIX), restart=restart, reorth=reorth, **lm.GMRES_ARGS)
    gm.check_bits(s, want, (restart, reorth))
    assert fmt_of(op) == 0 and s.basis_bytes >= 8 * (restart + 1) * A.shape[0]
    op.free()


# ---------------------------------------------------------------------------------------------- 2. IDR(s)
@pytest.mark.parametrize("s", lm.IDR_S)
def test_idr_at_the_shadow_limit(s):
    """The build-up and at least one full cycle of s + 1 steps behind it: the s x s matrix in LDS and its small solve at 31 and
    32 columns; on the plain CSR kernel and in the builder's format."""
    want = lm.idr_reference(s)
    assert want.nMatvec > 2 * s and want.s == s
    A = idr.matrix(lm.IDR_MATRIX)
    for fmt in (0, -1):
        op = device_op(A, False)
        if fmt >= 0:
            set_format(op, fmt)
        got = idr.solve(op, idr.rhs_of(lm.IDR_MATRIX), s=s, **lm.IDR_ARGS)
        idr.check_bits(got, want, (s, fmt))
        assert got.workspace_bytes >= 8 * 3 * s * A.shape[0]
        if fmt == 0:
            assert fmt_of(op) == 0
        op.free()


# ---------------------------------------------------------------------------------------------- 3. thick-restart Lanczos
@pytest.mark.parametrize("which", ["SA", "LA"])
def test_trlan_at_the_basis_limit(which):
    """One restart from a basis of 128: the 128 x 128 Jacobi, the rotation reading 128 columns in eight launches, the last
    of 9 columns, and a second cycle that orthogonalises against 122 .. 128 vectors."""
    want = lm.trlan_reference(which)
    assert want.cycles >= 2 and want.keep % tl.KT != 0
    A = tl.matrix(lm.TRLAN_MATRIX)
    op = device_op(A, True)
    s = tl.solve(op, lm.TRLAN_NEV, which=which, **lm.TRLAN_ARGS)
    tl.check_bits(s, want, which)
    assert s.ncv == lm.TRLAN_NCV and s.workspace_bytes == tl.workspace(A.shape[0], lm.TRLAN_NCV, s.keep)
    op.free()


# ---------------------------------------------------------------------------------------------- 4. thick-restart SVD
@pytest.mark.parametrize("reorth", sv.MODES)
def test_trsvd_at_the_basis_limit(reorth):
    """The same for both bases, on a 401 x 251 matrix from the small end of its spectrum."""
    R, C = lm.trsvd_matrix().shape
    op, tall = sv.operators(lm.TRSVD_MATRIX)
    want = lm.trsvd_reference(reorth, geometry=gpu_order.launch_geometry(tall))
    assert want.cycles >= 2 and want.keep % sv.KT != 0
    s = sv.solve(op, lm.TRSVD_NSV, reorth=reorth, **lm.TRSVD_ARGS)
    sv.check_bits(s, want, reorth)
    assert s.ncv == lm.TRSVD_NCV and s.workspace_bytes == sv.workspace(R, C, lm.TRSVD_NCV, s.keep)
    op.free()


# ---------------------------------------------------------------------------------------------- 5. LOBPCG
@pytest.mark.parametrize("block", lm.LOBPCG_BLOCKS)
def test_lobpcg_at_the_block_limit(block):
    """nev = block = 15 and 16: every accumulator of the Gram kernel in use, S = [X, W, P] of 45 and 48 columns from the
    second iteration on."""
    want = lm.lobpcg_reference(block)
    assert want.nIter >= 3 and list(want.actives[:3]) == [block] * 3
    op = device_op(lob.matrix(lm.LOBPCG_MATRIX), True)
    s = lob.solve(op, block, **lm.lobpcg_args(block))
    lob.check_bits(s, want, block)
    assert s.block == block and s.precon_route == "none"
    op.free()


# ---------------------------------------------------------------------------------------------- 6. L-BFGS
@pytest.mark.parametrize("scaling", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("npairs", lm.LBFGS_NPAIRS)
def test_lbfgs_at_the_pair_limit(npairs, scaling):
    """A full ring whose oldest pair is not in slot 0 (2 and 5 pairs stored beyond npairs): the two-loop recursion over
    2 npairs + 1 launches, out of place and in place, and the compact product -- 2 npairs columns in one multi-dot pass, 128
    of them in 16 groups at the limit -- of both forward operators."""
    import pykrylov_amd
    from pykrylov_amd import _lib
    n = lm.LBFGS_N
    S, Y, v = lm.lbfgs_pool()
    for wrap in lm.LBFGS_WRAPS:
        R, want_h, want_c, want_c1 = lm.lbfgs_reference(npairs, scaling, wrap)
        ops = lm.lbfgs_ops(npairs, wrap)
        tag = (npairs, scaling, wrap)
        assert sum(t is not None for t in R.ys) == npairs and R.insert != 0
        H = pykrylov_amd.InverseLBFGSOperator(n, npairs, scaling=scaling)
        lbfgs_ref.replay(H, ops, S, Y)
        assert H.insert == R.insert and H.info["stored"] == npairs and same(ys_array(H.ys), ys_array(R.ys)), tag
        assert same(H.s, R.s) and same(H.y, R.y), tag
        assert same(H * v, want_h), tag
        assert H.info["launches_last_apply"] == 2 * npairs + 1 and same(H.gamma, R.gamma), tag
        d_in, d_out = _lib.DeviceArray.from_numpy(v), _lib.DeviceArray(n)
        H.apply_device(d_in, d_out)
        assert same(d_out.to_numpy(), want_h) and same(d_in.to_numpy(), v), tag
        H.apply_device(d_in, d_in)
        assert same(d_in.to_numpy(), want_h), tag
        d_in.free()
        d_out.free()
        H.free()
        C = pykrylov_amd.CompactLBFGSOperator(n, npairs, scaling=scaling)
        lbfgs_ref.replay(C, ops, S, Y)
        assert same(C * v, want_c), tag
        assert C.insert == R.insert and same(C.gamma, R.gamma), tag
        C.free()
        B = pykrylov_amd.LBFGSOperator(n, npairs, scaling=scaling)
        lbfgs_ref.replay(B, ops, S, Y)
        assert same(B * v, want_c1) and B.gamma == 1.0, tag
        B.free()


# ---------------------------------------------------------------------------------------------- 7. Chebyshev
@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
def test_chebyshev_applied_at_the_degree_limit(scaled):
    """Degree 63 and 64 -- 64 and 65 launches, the last entries of the coefficient arrays -- out of place and in place."""
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    A = cheb.matrix(lm.CHEB_MATRIX)
    x = np.random.default_rng(11).standard_normal(A.shape[0])
    lmin, lmax = cheb_ref.interval(A, scale_diag=scaled)
    op = device_op(A, True)
    d_in, d_out = _lib.DeviceArray.from_numpy(x), _lib.DeviceArray(A.shape[0])
    for k in lm.CHEB_DEGREES:
        z = cheb_ref.apply(A, x, k, lmin, lmax, scaled)
        M = tools.chebyshev(op, degree=k, scale_diag=scaled)
        assert M.interval == (lmin, lmax) and M.info["launches"] == 1 + k
        assert same(M * x, z), (k, scaled)
        d_in.upload(x)
        _lib.check(lib.mk_cheb_apply(M.handle, d_in.ptr, d_out.ptr))
        assert same(d_out.to_numpy(), z) and same(d_in.to_numpy(), x), (k, scaled)
        M.apply_device(d_in, d_in)
        assert same(d_in.to_numpy(), z), (k, scaled)
        M.free()
    d_in.free()
    d_out.free()
    op.free()


@pytest.mark.parametrize("side", filt.SIDES)
def test_chebyshev_filter_applied_at_the_degree_limit(side):
    from pykrylov_amd import tools
    A = filt.matrix(lm.FILTER_MATRIX)
    op = device_op(A, True)
    iv, a0 = filt.plain_interval(A, side)
    for k in lm.FILTER_DEGREES:
        x, want = filt.applied(lm.FILTER_MATRIX, A, side, k)
        F = tools.cheb_filter(op, degree=k, interval=iv, ref=a0)
        assert F.degree == k and F.info["launches"] == k
        assert same(F * x, want), (side, k)
        F.free()
    op.free()


# ---------------------------------------------------------------------------------------------- 8. AMG
@pytest.mark.parametrize("name,rows", lm.AMG_CASES)
def test_amg_with_a_dense_level_of_several_rows_per_lane(name, rows):
    """coarse_max = 1024: the coarsest level's inverse is applied by one workgroup whose lanes take a second row (289 and 364
    rows) and four rows each with all of `sb[1024]` in use (1024 rows).  The two-level case passes max_levels = 16, the bound
    of that argument."""
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    kw = dict(max_levels=16) if len(rows) > 1 else {}
    A, H, x, z = lm.amg_reference(name, **kw)
    assert tuple(lv["A"].shape[0] for lv in H.levels) == rows and rows[-1] > 256 and H.inverse is not None
    op = device_op(A, True)
    M = tools.amg(op, coarse_max=lm.AMG_COARSE_MAX, **kw)
    amg.check_hierarchy(M, H, (name, lm.AMG_COARSE_MAX))
    assert M.info["coarse_solver"] == "inverse" and M.levels[-1]["rows"] == rows[-1]
    assert same(M * x, z), name
    d_in, d_out = _lib.DeviceArray.from_numpy(x), _lib.DeviceArray(A.shape[0])
    _lib.check(lib.mk_amg_apply(M.handle, d_in.ptr, d_out.ptr))
    assert same(d_out.to_numpy(), z) and same(d_in.to_numpy(), x), name
    _lib.check(lib.mk_amg_apply(M.handle, d_in.ptr, d_in.ptr))
    assert same(d_in.to_numpy(), z), name
    d_in.free()
    d_out.free()
    M.free()
    op.free()


# ---------------------------------------------------------------------------------------------- 9. ILU(0) / IC(0)
@pytest.mark.parametrize("name,fuse,launches", lm.ILU_CASES)
def test_ilu_launch_plans(name, fuse, launches, monkeypatch):
    """The launches of both sweeps against `_ilu_ref.plan`, the factor and the applies, out of place and in place: 4500 levels
    of one row in runs of 2048, 2048 and 404 (and one launch each); the widths 1 .. 17 .. 1 with the fuse width at 16 (the
    17-row level alone between two runs), 17 (one run) and 1 (only the first and the last level fuse); one level of 600 rows in
    ONE workgroup, which strides it three times, and in three workgroups, the last of 88 rows."""
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    if fuse is None:
        monkeypatch.delenv("MK_ILU_FUSE_ROWS", raising=False)
    else:
        monkeypatch.setenv("MK_ILU_FUSE_ROWS", str(fuse))
    f = lm.ILU_FUSE_DEFAULT if fuse is None else fuse
    for kind in ("ilu0", "ic0"):
        A, vals, wf, wb, x, want = lm.ilu_reference(name, kind)
        op = device_op(A, True)
        M = getattr(tools, kind)(op)
        what = (name, fuse, kind)
        info = M.info
        assert info["fuse_rows"] == f and M.levels == (len(wf), len(wb)) and info["widest_level"] == max(wf + wb), what
        assert M.launches == (len(ilu_ref.plan(wf, f)), len(ilu_ref.plan(wb, f))) == (launches, launches), what
        ip, ix, v, dg = M.factor_arrays()
        assert np.array_equal(ip, A.indptr) and np.array_equal(ix, A.indices)
        assert np.array_equal(dg, ilu_ref.diag_positions(A.indptr, A.indices))
        assert same(v, vals), what
        assert same(M * x, want), what
        d_in, d_out = _lib.DeviceArray.from_numpy(x), _lib.DeviceArray(A.shape[0])
        _lib.check(lib.mk_ilu_apply(M.handle, d_in.ptr, d_out.ptr))
        assert same(d_out.to_numpy(), want) and same(d_in.to_numpy(), x), what
        _lib.check(lib.mk_ilu_apply(M.handle, d_in.ptr, d_in.ptr))
        assert same(d_in.to_numpy(), want), what
        d_in.free()
        d_out.free()
        M.free()
        op.free()
