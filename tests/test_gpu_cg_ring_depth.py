"""CG's ring of directions at the depths the automatic rule reaches at HBM sizes (csrc/mk_cg.hip, csrc/mk_ringdepth.h): m = 24
and m = 32 (the cap, MK_XD_MAX) against the three-kernel pass (MK_CG_FUSE=0), BIT for bit -- history, x, r, p, matvec count --
and the caller's bound on the depth (mk_params_ring): it caps the automatic rule and an explicit MK_CG_XDEFER alike, for every
set-up of the object or for its first k only (what a placement search probes with)."""
import ctypes

import numpy as np
import pytest

from test_gpu_cg_xdefer import _matrix, _run_pieces, _same, _set
from test_gpu_pencil import fmt_of, op9

pytestmark = pytest.mark.gpu

MS = (24, 32)
UNFUSED = {"MK_CG_FUSE": "0", "MK_CG_XDEFER": "1"}
SHAPES = [((128, 128, 64), 9), ((101, 9, 11), 11), ((250, 7, 13), 9)]
# matvec_max one below, at and one above the cap, more than two rings, one pass; 400: a halt by tolerance inside a ring
COUNTS = (1, 31, 32, 33, 70, 400)
PARAMS = dict(abstol=0.0, reltol=0.0, matvec_max=1 << 40, check_curvature=1)


def _deep(m):
    return {"MK_CG_FUSE": "1", "MK_CG_XDEFER": str(m)}


def _rhs(A, seed):
    n = A.shape[0]
    return A.matvec(np.ones(n)) + 0.1 * np.random.default_rng(seed).standard_normal(n)


def _solves(A, fmt, rhs, env, monkeypatch):
    from pykrylov_amd import CG
    _set(monkeypatch, env)
    op = op9(A, symmetric=True, fmt=fmt)
    out = []
    for k in COUNTS:
        s = CG(op)
        s.solve(rhs, matvec_max=k)
        out.append((s.nMatvec, np.array(s.residHistory), s.x.copy(), float(s.residNorm)))
    assert fmt_of(op) == fmt
    return out


@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("dims,fmt", SHAPES)
def test_deep_rings_change_no_bit(dims, fmt, nt, monkeypatch):
    monkeypatch.setenv("MK_SPMV_NT", nt)
    A = _matrix(dims, fmt)
    rhs = _rhs(A, 4)
    want = _solves(A, fmt, rhs, UNFUSED, monkeypatch)        # (the reference: once per shape, shared by both depths)
    assert want[-1][0] < 400                                 # stopped by tolerance (50 passes on the last shape: between two sweeps)
    for m in MS:
        got = _solves(A, fmt, rhs, _deep(m), monkeypatch)
        for k, (g, w) in enumerate(zip(got, want)):
            _same(g, w, (m, COUNTS[k]))


@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("dims,fmt", SHAPES)
def test_uneven_pieces_with_x_read_between(dims, fmt, nt, monkeypatch):
    """Pieces of 1, m - 1, m + 1, 40 (more than a ring), 1 and 2 passes, x and p read after every piece, r, the history and the
    counts at the end; after every piece nothing is left to apply (`_run_pieces` asserts it)."""
    monkeypatch.setenv("MK_SPMV_NT", nt)
    A = _matrix(dims, fmt)
    rhs = _rhs(A, 2)
    for m in MS:
        pieces = [1, m - 1, m + 1, 40, 1, 2]
        _set(monkeypatch, UNFUSED)
        want = _run_pieces(op9(A, symmetric=True, fmt=fmt), rhs, pieces, True, **PARAMS)
        assert want[-4] == 2 * m + 44
        _set(monkeypatch, _deep(m))
        got = _run_pieces(op9(A, symmetric=True, fmt=fmt), rhs, pieces, True, **PARAMS)
        _same(got, want, m)


def _depth_run(op, rhs, passes, ring_cap=None, setups=1):
    """(ring depth the last set-up chose, what a caller sees after `passes` passes) of a run through the C ABI."""
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    kw = dict(PARAMS) if ring_cap is None else dict(PARAMS, ring_cap=ring_cap)
    with DeviceRun(op, _lib.MK_CG, rhs, None, placement_draws=1, **kw) as run:
        depths = []
        for _ in range(setups):
            run.setup()
            run.iterate(passes)
            res = run.finish()
            depths.append(int(res.aux[1]))
        seen = [run.x(), run.vector(1), run.vector(0), run.history(), int(res.nMatvec), int(res.itn), float(res.residNorm)]
    return depths, seen


def test_the_bound_of_the_parameter_block(monkeypatch):
    """mk_params_ring.  With the bound at 8 and MK_CG_XDEFER unset a run is MK_CG_XDEFER=8's bit for bit (at this size the
    automatic rule gives 1: the bound only caps).  The bound BEATS an explicit MK_CG_XDEFER=32 -- the environment chooses below
    the caller's bound, never above it (include/mikrylov.h) -- for every set-up ({8, 0}) or for the first only ({8, 1}: a placement
    probe, whose second set-up grows the ring to what the environment asks for)."""
    A = _matrix((128, 8, 26), 9)
    rhs = _rhs(A, 9)
    _set(monkeypatch, {"MK_CG_FUSE": "1", "MK_CG_XDEFER": "8"})
    d8, want = _depth_run(op9(A, symmetric=True), rhs, 45)
    assert d8 == [8]
    monkeypatch.delenv("MK_CG_XDEFER")
    d, got = _depth_run(op9(A, symmetric=True), rhs, 45, ring_cap=(8, 0))
    assert d == [1]
    _same(got, want, "bound 8, MK_CG_XDEFER unset")
    monkeypatch.setenv("MK_CG_XDEFER", "32")
    d, got = _depth_run(op9(A, symmetric=True), rhs, 45)
    assert d == [32]
    _same(got, want, "no bound, MK_CG_XDEFER=32")
    d, got = _depth_run(op9(A, symmetric=True), rhs, 45, ring_cap=(8, 0), setups=2)
    assert d == [8, 8]
    _same(got, want, "bound 8 at every set-up, MK_CG_XDEFER=32")
    d, got = _depth_run(op9(A, symmetric=True), rhs, 45, ring_cap=(8, 1), setups=3)
    assert d == [8, 32, 32]
    _same(got, want, "bound 8 at the first set-up, MK_CG_XDEFER=32")
    monkeypatch.setenv("MK_CG_FUSE", "0")
    d, got = _depth_run(op9(A, symmetric=True), rhs, 45, ring_cap=(8, 0))
    assert d == [0]
    _same(got, want, "three-kernel passes")


def test_the_block_is_validated():
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    A = _matrix((128, 8, 26), 9)
    op = op9(A, symmetric=True)
    for bad in ((33, 0), (-1, 0), (8, -1)):
        with pytest.raises(_lib.MkError):
            DeviceRun(op, _lib.MK_CG, _rhs(A, 1), None, ring_cap=bad, **PARAMS)
    assert ctypes.sizeof(_lib.MkParamsRing) == ctypes.sizeof(_lib.MkParams) + 8


def test_a_placement_search_probes_at_one_depth_and_grows_the_kept_ring(monkeypatch):
    """The search of DeviceRun creates its objects with {8, 1}: every probe is timed at m <= 8, and the kept object's set-up
    afterwards takes what MK_CG_XDEFER (or, unset at an HBM size, the memory rule) gives; the run is the unsearched one's."""
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    A = _matrix((128, 8, 26), 9)
    rhs = _rhs(A, 9)
    _set(monkeypatch, {"MK_CG_FUSE": "1", "MK_CG_XDEFER": "32", "MK_PLACEMENT_MIN_MB": "0", "MK_PLACEMENT_SPACER_MB": "1"})
    _, want = _depth_run(op9(A, symmetric=True), rhs, 45)
    with DeviceRun(op9(A, symmetric=True), _lib.MK_CG, rhs, None, placement_draws=3, **PARAMS) as run:
        assert DeviceRun.PROBE_RING == (8, 1)
        run.setup()
        assert run.placement["count"] == 3
        run.iterate(45)
        res = run.finish()
        assert int(res.aux[1]) == 32
        got = [run.x(), run.vector(1), run.vector(0), run.history(), int(res.nMatvec), int(res.itn), float(res.residNorm)]
    _same(got, want, "searched")
