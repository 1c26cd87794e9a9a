"""z-uniform pattern bytes of the brick march (formats 9 / 10 / 11, csrc/mk_format.hip `pen_zuniform`, csrc/mk_spmv_fmt9.h): where
every interior plane of a matrix carries the pattern bytes of plane 1 -- decided on the bytes when the format is built, reported
in slot 12 of mk_csr_march_info -- the march reads the interior planes' bytes from plane 1.  The same bytes, so every product
and every CG run keeps its bits; a matrix whose planes differ keeps reading its own bytes."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref
from test_gpu_cg_xdefer import _run_pieces, _same, _set
from test_gpu_pencil import fmt_of, op9

pytestmark = pytest.mark.gpu

FUSED = {"MK_CG_FUSE": "1", "MK_CG_XDEFER": "3"}
UNFUSED = {"MK_CG_FUSE": "0", "MK_CG_XDEFER": "1"}


def zuniform(op):
    from pykrylov_amd import _lib
    info = (ctypes.c_int64 * 13)()
    _lib.check(_lib.init().mk_csr_march_info(op.handle, info, 13))
    return int(info[12])


def check_bits(A, fmt, flag, monkeypatch, seed=3):
    """format, flag, the plain product against format 0 (and the oracle) and CG's fused passes against the three-kernel pass"""
    from pykrylov_amd import CG
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    op, op0 = op9(A, symmetric=True, fmt=fmt), op9(A, symmetric=True, fmt=0)
    for trial in range(2):
        x = rng.standard_normal(n)
        if trial:
            x[::7] = 0.0
            x[5::11] *= 1e300
        y = op * x
        assert fmt_of(op) == fmt and fmt_of(op0) == 0
        assert np.array_equal(y, op0 * x) and np.array_equal(y, A.matvec(x))
    assert zuniform(op) == flag and zuniform(op0) == 0
    rhs = A.matvec(np.ones(n)) + 0.1 * rng.standard_normal(n)
    runs = []
    for env in (UNFUSED, FUSED):
        _set(monkeypatch, env)
        s = CG(op9(A, symmetric=True, fmt=fmt))
        s.solve(rhs, matvec_max=40)
        runs.append((s.nMatvec, np.array(s.residHistory), s.x.copy(), float(s.residNorm)))
    _same(runs[1], runs[0], "fused CG")
    op.free()
    op0.free()


def without_couplings(A, P, planes):
    """A with the couplings between the planes z and z + 1 removed, symmetrically, for every z of `planes`"""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    cols, vals = np.asarray(A.indices, dtype=np.int64), np.asarray(A.data)
    keep = np.ones(len(cols), dtype=bool)
    for z in planes:
        keep &= ~((rows // P == z) & (cols == rows + P))
        keep &= ~((rows // P == z + 1) & (cols == rows - P))
    return csr_ref.from_coo(rows[keep], cols[keep], vals[keep], A.shape)


@pytest.mark.parametrize("dims,fmt", [((128, 8, 26), 9), ((101, 9, 11), 11), ((255, 15, 8), 10)])
def test_flag_set_and_bits_equal(dims, fmt, monkeypatch):
    A = csr_ref.poisson3d(*dims) if fmt == 9 else csr_ref.poisson3d_varcoef(*dims, seed=5)
    check_bits(A, fmt, 1, monkeypatch)


@pytest.mark.parametrize("z", [5, 1, 24])
def test_flag_clear_where_an_interior_plane_or_an_end_differs(z, monkeypatch):
    """The couplings z <-> z + 1 of one pair of planes removed: in the interior (5 <-> 6), at plane 1 itself (1 <-> 2: the plane the
    others are compared with) and below the last plane (nz - 2 <-> nz - 1: the interior plane nz - 2 changes, the last plane may)."""
    A = without_couplings(csr_ref.poisson3d(128, 8, 26), 128 * 8, [z])
    check_bits(A, 9, 0, monkeypatch)


@pytest.mark.parametrize("nz,flag", [(3, 1), (2, 0)])
def test_three_planes_have_one_interior_plane_and_two_have_none(nz, flag, monkeypatch):
    check_bits(csr_ref.poisson3d(128, 8, nz), 9, flag, monkeypatch)


def test_a_last_plane_of_its_own_leaves_the_flag_set(monkeypatch):
    """z-uniform except in the last plane: its -1 / +1 couplings are gone for every fourth row pair -- the last plane is read at its
    own bytes, like the first."""
    A = csr_ref.poisson3d(128, 8, 26)
    P, n = 128 * 8, A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    cols, vals = np.asarray(A.indices, dtype=np.int64), np.asarray(A.data)
    lo = np.minimum(rows, cols)
    drop = (rows // P == 25) & (np.abs(cols - rows) == 1) & (lo % 4 == 0)
    assert drop.sum() > 100
    B = csr_ref.from_coo(rows[~drop], cols[~drop], vals[~drop], A.shape)
    check_bits(B, 9, 1, monkeypatch)
    # ... and the same change in the FIRST plane and in an interior one: set, clear
    for z, flag in ((0, 1), (7, 0)):
        drop = (rows // P == z) & (np.abs(cols - rows) == 1) & (lo % 4 == 0)
        check_bits(csr_ref.from_coo(rows[~drop], cols[~drop], vals[~drop], A.shape), 9, flag, monkeypatch)


@pytest.mark.parametrize("varcoef,fmt", [(False, 9), (True, 11)])
@pytest.mark.parametrize("nr,rank,planes", [(3, 1, 20), (3, 0, 7), (2, 1, 13)])
def test_a_slab_takes_the_flag_from_its_own_bytes(nr, rank, planes, varcoef, fmt, monkeypatch):
    """One rank's slab over the host-staged loopback transport of tests/test_gpu_slab_march.py: the slab's plan checks the slab's
    bytes (a middle rank's first and last planes are interior planes of the grid and carry the interior's bytes; rank 0's first
    plane does not, and is read at its own), interior + boundary launches and the whole-slab launch (7 planes)."""
    from pykrylov_amd import _lib
    from test_gpu_slab_march import build_slab, local_oracle
    want = None
    for env in (UNFUSED, FUSED):
        _set(monkeypatch, env)
        lib, world, op = build_slab(128, 8, planes * nr, nr, rank, varcoef, fmt)
        try:
            n_local, ncols = int(op.shape[0]), int(op.shape[1])
            A = local_oracle(op)
            rng = np.random.default_rng(11 + rank)
            x = rng.standard_normal(ncols)
            xd, yd = _lib.DeviceArray.from_numpy(x), _lib.DeviceArray(n_local)
            op.spmv_device(xd.ptr, yd.ptr)
            assert fmt_of(op) == fmt and zuniform(op) == 1
            assert np.array_equal(yd.to_numpy(), A.matvec(x))
            rhs = _lib.DeviceArray.from_numpy(rng.standard_normal(n_local))
            got = _run_pieces(op, rhs, [5, 16, 4], True, n_own=n_local, abstol=0.0, reltol=0.0, matvec_max=1 << 60, check_curvature=1)
        finally:
            op.free()
            lib.mk_comm_destroy()
        if want is None:
            want = got
        _same(got, want, env)
