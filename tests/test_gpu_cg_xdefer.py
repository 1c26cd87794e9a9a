"""CG with a DEFERRED x update (csrc/mk_cg.hip, MK_CG_XDEFER = m): the fused product kernel leaves x alone, the last m
directions stay in a ring of m + 1 buffers and one sweep (`cg_xapply`) applies them -- each `x += alpha p` rounded on its own,
in order.  Everything here is compared BIT for bit with the three-kernel pass (MK_CG_FUSE=0) and with MK_CG_XDEFER=1 (the
x-carrying fused kernel): history, iterate, matvec count, residual norm, residual vector and search direction."""
import os

import numpy as np
import pytest

from oracle import csr_ref
from test_gpu_pencil import _solver_is_fused, fmt_of, op9, sym_banded

pytestmark = pytest.mark.gpu

MS = (2, 3, 8, 16)
# (knob settings, label): the three-kernel pass, the x-carrying fused pass, the deferred ones
VARIANTS = [({"MK_CG_FUSE": "0", "MK_CG_XDEFER": "1"}, "unfused"), ({"MK_CG_FUSE": "1", "MK_CG_XDEFER": "1"}, "m1")] + \
           [({"MK_CG_FUSE": "1", "MK_CG_XDEFER": str(m)}, "m%d" % m) for m in MS]


def _set(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _matrix(dims, fmt):
    return csr_ref.poisson3d(*dims) if fmt == 9 else csr_ref.poisson3d_varcoef(*dims, seed=5)


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (u, v) in enumerate(zip(a, b)):
        if isinstance(u, np.ndarray):
            assert u.shape == v.shape and np.array_equal(u, v), (what, i)
        else:
            assert u == v, (what, i, u, v)


def _solve_all(A, fmt, rhs, cases, monkeypatch, precon=None):
    """Every case under every variant; returns {label: [(nMatvec, history, x, residNorm), ...]}."""
    from pykrylov_amd import CG
    out = {}
    for env, label in VARIANTS:
        _set(monkeypatch, env)
        op = op9(A, symmetric=True, fmt=fmt)
        assert _solver_is_fused(op, rhs) == (env["MK_CG_FUSE"] == "1")
        res = []
        for kw in cases:
            s = CG(op) if precon is None else CG(op, precon=precon)
            s.solve(rhs, **kw)
            res.append((s.nMatvec, np.array(s.residHistory), s.x.copy(), float(s.residNorm)))
        assert fmt_of(op) == fmt
        out[label] = res
    return out


# aligned bricks (128 x 128 x 64 and a larger one), general geometry (odd L, odd P, P no multiple of 4 L), formats 9 / 10 / 11
SOLVE_CASES = [((128, 128, 64), 9), ((256, 128, 40), 11), ((128, 8, 26), 10), ((101, 9, 11), 11), ((250, 7, 13), 9), ((255, 15, 8), 10)]


@pytest.mark.parametrize("dims,fmt", SOLVE_CASES)
def test_deferred_x_changes_no_bit(dims, fmt, monkeypatch):
    """Default stopping (a halt by tolerance, wherever in the ring it falls), matvec_max at counts that are no multiples of
    m (and one that is), a nonzero initial guess."""
    A = _matrix(dims, fmt)
    n = A.shape[0]
    rng = np.random.default_rng(4)
    rhs = A.matvec(np.ones(n)) + 0.1 * rng.standard_normal(n)
    guess = rng.standard_normal(n)
    cases = [dict(matvec_max=400), dict(matvec_max=1), dict(matvec_max=7), dict(matvec_max=16), dict(matvec_max=37),
             dict(guess=guess, matvec_max=23)]
    out = _solve_all(A, fmt, rhs, cases, monkeypatch)
    for label in out:
        for k in range(len(cases)):
            _same(out[label][k], out["unfused"][k], (label, cases[k].get("matvec_max")))
    assert out["unfused"][0][0] < 400                        # (the first case stopped by tolerance)


@pytest.mark.parametrize("nt", ["1", "0"])
def test_deferred_x_nontemporal_and_five_point(nt, monkeypatch):
    """MK_SPMV_NT=1 (the instantiations the 512^3 headline runs: non-temporal p / Ap stores, non-temporal sweep of x) on a
    7-point matrix, on a 5-point one (marched line by line) and on a general geometry."""
    monkeypatch.setenv("MK_SPMV_NT", nt)
    rng = np.random.default_rng(6)
    for A, fmt in ((csr_ref.poisson3d(128, 8, 26), 9), (csr_ref.poisson2d(300), 9), (csr_ref.poisson3d_varcoef(100, 9, 7, seed=2), 11)):
        n = A.shape[0]
        rhs = A.matvec(np.ones(n)) + 0.1 * rng.standard_normal(n)
        cases = [dict(matvec_max=300), dict(matvec_max=13)]
        out = _solve_all(A, fmt, rhs, cases, monkeypatch)
        for label in out:
            for k in range(len(cases)):
                _same(out[label][k], out["unfused"][k], (nt, label, k))


def test_deferred_x_with_a_diagonal_preconditioner(monkeypatch):
    from pykrylov_amd.linop import DiagonalOperator
    A = csr_ref.poisson3d_varcoef(128, 8, 14, seed=5)
    n = A.shape[0]
    rng = np.random.default_rng(8)
    rhs = A.matvec(np.ones(n)) + 0.1 * rng.standard_normal(n)
    d = 1.0 / (1.0 + rng.random(n))
    out = _solve_all(A, 11, rhs, [dict(matvec_max=200), dict(matvec_max=11)], monkeypatch, precon=DiagonalOperator(d))
    for label in out:
        for k in range(2):
            _same(out[label][k], out["unfused"][k], (label, k))


def _deferring():
    return os.environ.get("MK_CG_FUSE") == "1" and int(os.environ.get("MK_CG_XDEFER", "1")) > 1


def _run_pieces(op, rhs, pieces, look, n_own=None, guess=None, **params):
    """A run through the C ABI in uneven pieces; `look`: read x (and p) after every piece.  Returns what a caller can see."""
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    seen = []
    with DeviceRun(op, _lib.MK_CG, rhs, guess, **params) as run:
        run.setup()
        for k in pieces:
            run.iterate(k)
            if _deferring():
                assert run.unapplied() == 0, ("unapplied directions after iterate(%d)" % k, run.unapplied())
            if look:
                seen.append(run.x())
                seen.append(run.vector(1)[:n_own])
        res = run.finish()
        seen += [run.x(), run.vector(1)[:n_own], run.vector(0)[:n_own], run.history(), int(res.nMatvec), int(res.itn),
                 float(res.residNorm)]
        seen.append(run.x())                                  # (asked twice: nothing may be applied twice)
    return seen


@pytest.mark.parametrize("dims,fmt", [((128, 128, 64), 9), ((101, 9, 11), 11), ((128, 8, 26), 10)])
@pytest.mark.parametrize("look", [False, True])
def test_uneven_pieces_and_looks_between_passes(dims, fmt, look, monkeypatch):
    """`iterate` called in pieces of 1, m - 1, m + 1 and the driver's 20 (enqueued as 16 + 4), x read between the pieces (or
    only at the end), no halt inside: after every call nothing is left to apply."""
    A = _matrix(dims, fmt)
    n = A.shape[0]
    rhs = A.matvec(np.ones(n)) + 0.1 * np.random.default_rng(2).standard_normal(n)
    params = dict(abstol=0.0, reltol=0.0, matvec_max=1 << 40, check_curvature=1)
    want = {}
    for env, label in VARIANTS:
        _set(monkeypatch, env)
        op = op9(A, symmetric=True, fmt=fmt)
        for mm in (MS if label in ("unfused", "m1") else (int(env["MK_CG_XDEFER"]),)):
            got = _run_pieces(op, rhs, [1, mm - 1, mm + 1, 20, 1, 2], look, **params)
            if label == "unfused":
                want[mm] = got
                assert got[-4] == 2 * mm + 24
            _same(got, want[mm], (label, mm))


@pytest.mark.parametrize("dims,fmt", [((128, 8, 26), 9), ((250, 7, 13), 11)])
def test_halts_in_mid_ring_and_passes_enqueued_behind_them(dims, fmt, monkeypatch):
    """A halt by tolerance and by matvec_max in the middle of a ring, with far more passes enqueued behind it than the ring
    holds (iterate(200) in one call: batches of 16, 32, ... are enqueued before the host learns of the halt), x read after
    the halt, twice."""
    A = _matrix(dims, fmt)
    n = A.shape[0]
    rhs = A.matvec(np.ones(n)) + 0.1 * np.random.default_rng(3).standard_normal(n)
    for params in (dict(abstol=0.0, reltol=1e-3, matvec_max=1 << 40), dict(abstol=0.0, reltol=0.0, matvec_max=5),
                   dict(abstol=0.0, reltol=0.0, matvec_max=21), dict(abstol=0.0, reltol=1e-2, matvec_max=1 << 40)):
        want = None
        for env, label in VARIANTS:
            _set(monkeypatch, env)
            op = op9(A, symmetric=True, fmt=fmt)
            got = _run_pieces(op, rhs, [3, 200, 7], True, check_curvature=1, **params)
            if want is None:
                want = got
                assert got[-4] < 150                          # (halted well inside the 200 passes of the second piece)
            _same(got, want, (label, params))


def test_curvature_halt_keeps_the_stopped_direction_out_of_x(monkeypatch):
    """An indefinite matrix of the class: the pass whose <p, Ap> <= 0 stops the loop before its x update (cg.py:119-124) --
    its direction is in the ring and must not reach x."""
    rng = np.random.default_rng(11)
    L, P = 128, 512
    n = P * 12
    A = sym_banded(n, L, P, rng, drop=0.2)
    rhs = rng.standard_normal(n)
    want = None
    for env, label in VARIANTS:
        _set(monkeypatch, env)
        op = op9(A, symmetric=True, fmt=11)
        got = _run_pieces(op, rhs, [60, 5], False, abstol=0.0, reltol=0.0, matvec_max=1 << 40, check_curvature=1)
        if want is None:
            want = got
            assert got[-3] == got[-4] - 1 and got[-4] < 60    # (itn = nMatvec - 1: the last product's pass was abandoned)
        _same(got, want, label)


@pytest.mark.parametrize("nx,ny", [(128, 8), (100, 9)])
@pytest.mark.parametrize("nr,rank,planes", [(2, 0, 20), (2, 1, 13), (3, 1, 20), (3, 0, 7), (3, 2, 23)])
def test_deferred_x_on_a_slab_over_the_host_transport(nr, rank, planes, nx, ny, monkeypatch):
    """One rank of 2 and of 3 on its slab over the host-staged transport (the loopback of tests/test_gpu_slab_march.py):
    interior + boundary launches and the whole-slab launch (7 planes), the neighbours' planes of p formed on the spot and kept
    behind the own rows of every ring slot."""
    from pykrylov_amd import _lib
    from test_gpu_slab_march import build_slab
    want = None
    for env, label in VARIANTS:
        _set(monkeypatch, env)
        lib, world, op = build_slab(nx, ny, planes * nr, nr, rank, True, 11)
        try:
            n_local = int(op.shape[0])
            rng = np.random.default_rng(5)
            rhs = _lib.DeviceArray.from_numpy(rng.standard_normal(n_local))
            guess = _lib.DeviceArray.from_numpy(rng.standard_normal(n_local))
            got = []
            for g in (None, guess):
                got += _run_pieces(op, rhs, [5, 16, 4], True, n_own=n_local, guess=g, abstol=0.0, reltol=0.0, matvec_max=1 << 60,
                                   check_curvature=1)
        finally:
            op.free()
            lib.mk_comm_destroy()
        if want is None:
            want = got
        _same(got, want, label)
