"""Device L-BFGS operators (pykrylov_amd/lbfgs.py, csrc/mk_lbfgs.hip): products and state bit for bit against the NumPy
restatement of the reference (tests/_lbfgs_ref.py) run with the device's summation order, solves preconditioned on the
device bit for bit against the same solves through the host callback, halting, lifetimes, launch counts and errors."""
import ctypes
import os

import numpy as np
import pytest

from oracle import csr_ref
from oracle.gpu_order import stream_dot
from tests import _lbfgs_ref as lr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (1, 2, 255, 1000, 1001, 2 ** 18 + 3, 2 ** 20 + 3)        # the last two: more than one pair per lane (512 workgroups)
NPAIRS = (1, 5, 8)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def ys_array(ys):
    return np.array([np.nan if t is None else t for t in ys])


_POOLS = {}


def pool(n):
    if n not in _POOLS:
        _POOLS.clear()                                           # (one size at a time: the large pools are 100 MB each)
        S, Y = lr.make_pairs(n, lr.POOL, 31 + n)
        _POOLS[n] = (S, Y, np.random.default_rng(77 + n).standard_normal(n))
    return _POOLS[n]


def cases(n):
    for npairs in NPAIRS:
        for scaling in (False, True):
            for name in lr.SCENARIOS:
                yield npairs, scaling, name


# ------------------------------------------------------------------ 1. apply
@pytest.mark.parametrize("n", SIZES)
def test_apply_bit_for_bit(n):
    import pykrylov_amd
    from pykrylov_amd import _lib
    S, Y, v = pool(n)
    for npairs, scaling, name in cases(n):
        ops = lr.scenario_ops(name, npairs)
        R = lr.RefLBFGS(n, npairs, scaling, dot=stream_dot)
        H = pykrylov_amd.InverseLBFGSOperator(n, npairs, scaling=scaling)
        lr.replay(R, ops, S, Y)
        lr.replay(H, ops, S, Y)
        want = R.inverse(v)
        got = H * v
        tag = (n, npairs, scaling, name)
        assert same(got, want), tag
        assert H.insert == R.insert and same(ys_array(H.ys), ys_array(R.ys)) and same(H.gamma, R.gamma), tag
        p = sum(t is not None for t in R.ys)
        assert H.info["launches_last_apply"] == 2 * p + 1 and H.info["stored"] == p, tag
        # in place and out of place on device vectors
        d_in, d_out = _lib.DeviceArray.from_numpy(v), _lib.DeviceArray(n)
        H.apply_device(d_in, d_out)
        assert same(d_out.to_numpy(), want) and same(d_in.to_numpy(), v), tag
        H.apply_device(d_in, d_in)
        assert same(d_in.to_numpy(), want), tag
        d_in.free()
        d_out.free()
        H.free()


# ------------------------------------------------------------------ 2. forward
@pytest.mark.parametrize("n", SIZES)
def test_forward_bit_for_bit(n):
    import pykrylov_amd
    S, Y, v = pool(n)
    for npairs, scaling, name in cases(n):
        ops = lr.scenario_ops(name, npairs)
        R = lr.RefLBFGS(n, npairs, scaling, dot=stream_dot)
        C = pykrylov_amd.CompactLBFGSOperator(n, npairs, scaling=scaling)
        lr.replay(R, ops, S, Y)
        lr.replay(C, ops, S, Y)
        tag = (n, npairs, scaling, name)
        assert same(C * v, R.compact(v)), tag
        assert C.insert == R.insert and same(ys_array(C.ys), ys_array(R.ys)) and same(C.gamma, R.gamma), tag
        B = pykrylov_amd.LBFGSOperator(n, npairs, scaling=scaling)
        lr.replay(B, ops, S, Y)
        got = B * v
        assert B.gamma == 1.0, tag                               # the outer-product form never reads gamma
        if scaling:
            C0 = pykrylov_amd.CompactLBFGSOperator(n, npairs, scaling=False)
            lr.replay(C0, ops, S, Y)
            assert same(got, C0 * v), tag
            C0.free()
        else:
            assert same(got, C * v), tag
        B.free()
        C.free()


def test_forward_against_the_reference_fixture():
    """n = 10: LBFGSOperator against the reference's outer-product B * v (relative 2-norm 1e-12, the project's parity
    bar), and the reference's own criterion np.allclose((B * H).full(), eye) (its tests/test_lbfgs.py:55-56)."""
    import pykrylov_amd
    g = np.load(os.path.join(GOLDEN, "lbfgs.npz"))
    n = 10
    S, Y, v = g["pool_s_10"], g["pool_y_10"], g["v_10"]
    for npairs in (1, 5):
        for scaling in (0, 1):
            for name in lr.SCENARIOS:
                key = "%d_%d_%d_%s_" % (n, npairs, scaling, name)
                ops = [tuple(o) for o in g[key + "ops"]]
                B = pykrylov_amd.LBFGSOperator(n, npairs, scaling=bool(scaling))
                H = pykrylov_amd.InverseLBFGSOperator(n, npairs, scaling=False)
                C = pykrylov_amd.CompactLBFGSOperator(n, npairs, scaling=bool(scaling))
                Hs = pykrylov_amd.InverseLBFGSOperator(n, npairs, scaling=bool(scaling))
                for op in (B, H, C, Hs):
                    lr.replay(op, ops, S, Y)
                want = g[key + "Bv"]
                err = np.linalg.norm(B * v - want) / np.linalg.norm(want)
                print("%s rel err of B*v against the reference: %.3e" % (key, err))
                assert err <= 1e-12, key
                for got, what in ((C * v, "Cv"), (Hs * v, "Hv")):
                    e = np.linalg.norm(got - g[key + what]) / np.linalg.norm(g[key + what])
                    assert e <= 1e-12, (key, what, e)
                assert np.allclose((B * H).full(), np.eye(n)), key
                assert np.allclose((C * Hs).full(), np.eye(n)), key
                for op in (B, H, C, Hs):
                    op.free()


# ------------------------------------------------------------------ 3. store
def test_store_from_device_arrays_and_download():
    import pykrylov_amd
    from pykrylov_amd import _lib
    n, npairs = 1001, 5
    S, Y, v = pool(n)
    A = pykrylov_amd.InverseLBFGSOperator(n, npairs, scaling=True)
    B = pykrylov_amd.InverseLBFGSOperator(n, npairs, scaling=True)
    R = lr.RefLBFGS(n, npairs, True, dot=stream_dot)
    for i in range(7):
        ds, dy = _lib.DeviceArray.from_numpy(S[i]), _lib.DeviceArray.from_numpy(Y[i])
        assert A.store(S[i], Y[i]) is True
        assert B.store(ds, dy) is True
        R.store(S[i], Y[i])
        assert same(ds.to_numpy(), S[i]) and same(dy.to_numpy(), Y[i])
        ds.free()
        dy.free()
        assert not A.store(S[i], -S[i]) and not B.store(S[i], np.zeros(n))       # rejected: nothing changes
        assert A.insert == B.insert == R.insert
        assert same(ys_array(A.ys), ys_array(B.ys)) and same(ys_array(A.ys), ys_array(R.ys))
        assert same(A.s, B.s) and same(A.y, B.y)
        assert A.s.shape == (n, npairs)
        assert same(A.s, R.s) and same(A.y, R.y)
        assert same(A * v, B * v)
    assert A.info["accepted"] == 7 and A.info["rejected"] == 7
    A.accept_threshold = 1e300                                   # settable, and read at the next store
    assert not A.store(S[0], Y[0]) and A.info["rejected"] == 8
    A.restart()
    assert A.insert == 0 and A.ys == [None] * npairs and A.info["stored"] == 0
    assert same(A * v, v)
    A.free()
    B.free()


# ------------------------------------------------------------------ 4. in the loops
def _matrix(name):
    if name == "poisson2d_64":
        return csr_ref.poisson2d(64)
    return csr_ref.read_matrix_market(os.path.join(GOLDEN, "1138bus.mtx"))


def _secant_operator(A, npairs=5, scaling=True):
    import pykrylov_amd
    n = A.shape[0]
    H = pykrylov_amd.InverseLBFGSOperator(n, npairs, scaling=scaling)
    rng = np.random.default_rng(8)
    for _ in range(npairs):
        s = rng.standard_normal(n)
        assert H.store(s, A.matvec(s))
    return H


class Shell(object):
    """A plain object whose product forwards to H: dispatch takes the host-callback route."""

    def __init__(self, H):
        self.H, self.calls = H, 0

    def __mul__(self, x):
        self.calls += 1
        return self.H * x


def _solve(cls_name, op, rhs, precon):
    import pykrylov_amd
    cls = dict(cg=pykrylov_amd.CG, bicgstab=pykrylov_amd.BiCGSTAB, cgs=pykrylov_amd.CGS, tfqmr=pykrylov_amd.TFQMR,
               minres=pykrylov_amd.Minres, symmlq=pykrylov_amd.Symmlq)[cls_name]
    if cls_name == "minres":
        s = cls(op)
        s.solve(rhs, precon=precon, show=False, check=False, etol=0.0, rtol=1e-10)
        return s.itn, np.array(s.residHistory), s.x
    if cls_name == "symmlq":
        s = cls(op, precon=precon)
        s.solve(rhs, rtol=1e-10)
        return s.nMatvec, np.array([s.residNorm]), s.x
    s = cls(op, precon=precon, reltol=1e-10)
    s.solve(rhs, matvec_max=400)
    return s.nMatvec, np.array(getattr(s, "residHistory", [s.residNorm])), s.x


@pytest.mark.parametrize("solver", ["cg", "bicgstab", "cgs", "tfqmr", "minres", "symmlq"])
@pytest.mark.parametrize("name", ["poisson2d_64", "1138bus"])
def test_solver_with_device_operator_matches_the_callback_path(solver, name):
    from pykrylov_amd import CsrOperator
    A = _matrix(name)
    op = CsrOperator(A.indptr, A.indices, A.data, A.shape, symmetric=True)
    rhs = A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))
    H = _secant_operator(A)
    applies0 = H.info["applies"]
    k0, h0, x0 = _solve(solver, op, rhs, H)
    on_device = H.info["applies"] - applies0
    shell = Shell(H)
    k1, h1, x1 = _solve(solver, op, rhs, shell)
    assert shell.calls > 1 and on_device >= shell.calls
    assert k0 == k1 and same(h0, h1) and same(x0, x1), (solver, name, k0, k1)
    H.free()
    op.free()


# ------------------------------------------------------------------ 5. halting and lifetime
def _has_vector(run, k):
    try:
        run.vector(k)
        return True
    except Exception:
        return False


def test_apply_after_halt_is_a_no_op_at_every_site():
    """A solve stopped by its iteration budget: the vectors after the stop equal those of the callback path, whose
    callback is not invoked once the loop has halted."""
    from pykrylov_amd import CsrOperator, _lib
    from pykrylov_amd.generic import DeviceRun, HostPrecon
    A = _matrix("poisson2d_64")
    op = CsrOperator(A.indptr, A.indices, A.data, A.shape, symmetric=True)
    rhs = A.matvec(np.ones(A.shape[0]))
    H = _secant_operator(A)
    for kind in (_lib.MK_BICGSTAB, _lib.MK_CG, _lib.MK_CGS, _lib.MK_TFQMR):
        out = []
        for p in (H, HostPrecon(Shell(H))):
            run = DeviceRun(op, kind, rhs, None, precon_diag=p, abstol=0.0, reltol=0.0, matvec_max=5)
            run.run()
            assert run.iterate(3) == 0
            out.append([run.x()] + [run.vector(k) for k in range(2) if _has_vector(run, k)])
            run.close()
        assert len(out[0]) == len(out[1]) and all(same(a, b) for a, b in zip(out[0], out[1])), kind
    H.free()
    op.free()


def test_solver_keeps_the_operator_alive_and_sees_a_store_between_solves():
    import pykrylov_amd
    from pykrylov_amd import CsrOperator, _lib
    from pykrylov_amd.generic import DeviceRun
    A = _matrix("poisson2d_64")
    n = A.shape[0]
    op = CsrOperator(A.indptr, A.indices, A.data, A.shape, symmetric=True)
    rhs = A.matvec(np.ones(n))
    H = _secant_operator(A, npairs=6)                            # (five pairs in six slots)
    G = _secant_operator(A, npairs=6)
    s_ref = pykrylov_amd.CG(op, precon=Shell(G), reltol=1e-10)
    s_ref.solve(rhs, matvec_max=400)
    first = (s_ref.nMatvec, s_ref.x.copy())
    extra = np.random.default_rng(99).standard_normal(n)
    assert G.store(extra, A.matvec(extra))
    s_ref.solve(rhs, matvec_max=400)
    second = (s_ref.nMatvec, s_ref.x.copy())
    assert not same(first[1], second[1])                         # the sixth pair changes the solve

    run = DeviceRun(op, _lib.MK_CG, rhs, None, precon_diag=H, abstol=1e-8, reltol=1e-10, matvec_max=400)
    res = run.run()
    assert res.nMatvec == first[0] and same(run.x(), first[1])
    assert H.store(extra, A.matvec(extra))                       # between two solves of the SAME solver object
    H.free()                                                     # ... which still holds the operator
    res = run.run()
    assert res.nMatvec == second[0] and same(run.x(), second[1])
    x = run.x()
    assert run.iterate(5) == 0 and same(run.x(), x)              # halted: every launch of the apply is a no-op
    run.close()
    G.free()
    op.free()


# ------------------------------------------------------------------ 6. launch count
def test_launch_count_is_2p_plus_1():
    import pykrylov_amd
    n = 1001
    S, Y, v = pool(n)
    H = pykrylov_amd.InverseLBFGSOperator(n, 8, scaling=True)
    for p in range(9):
        assert H.info["stored"] == p
        H * v
        assert H.info["launches_last_apply"] == 2 * p + 1, p
        if p < 8:
            assert H.store(S[p], Y[p])
    H.free()


# ------------------------------------------------------------------ 7. full size
def test_full_size_apply_and_compact_product():
    """n = 2^24, five pairs, full ring (10 columns x 128 MiB on the device): one apply and one compact product."""
    import pykrylov_amd
    n, npairs = 2 ** 24, 5
    rng = np.random.default_rng(5)
    R = lr.RefLBFGS(n, npairs, True, dot=stream_dot)
    H = pykrylov_amd.InverseLBFGSOperator(n, npairs, scaling=True)
    C = pykrylov_amd.CompactLBFGSOperator(n, npairs, scaling=True)
    for _ in range(npairs):
        s = rng.standard_normal(n)
        y = s * (1.0 + rng.random(n)) + 0.01 * rng.standard_normal(n)
        R.store(s, y)
        assert H.store(s, y) and C.store(s, y)
    v = rng.standard_normal(n)
    assert H.info["bytes"] >= 10 * 8 * n
    assert same(H * v, R.inverse(v))
    assert H.info["launches_last_apply"] == 11
    assert same(ys_array(H.ys), ys_array(R.ys)) and same(H.gamma, R.gamma)
    assert same(C * v, R.compact(v))
    H.free()
    C.free()


# ------------------------------------------------------------------ 8. errors
def test_errors():
    import pykrylov_amd
    from pykrylov_amd import CsrOperator, _lib
    A = _matrix("poisson2d_64")
    n = A.shape[0]
    op = CsrOperator(A.indptr, A.indices, A.data, A.shape, symmetric=True)
    rhs = np.ones(n)
    small = pykrylov_amd.InverseLBFGSOperator(n - 1)
    with pytest.raises(ValueError, match="shape"):
        pykrylov_amd.CG(op, precon=small).solve(rhs)
    lib = _lib.init()
    prm = _lib.MkParams()
    prm.struct_size = ctypes.sizeof(_lib.MkParams)
    prm.kind = _lib.MK_CG
    prm.matvec_max = 10
    h = ctypes.c_void_p()
    _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(prm), ctypes.byref(h)))
    assert lib.mk_solver_set_precon_lbfgs(h, small.handle) == -2             # MK_ERR_ARG: size mismatch
    H = pykrylov_amd.InverseLBFGSOperator(n)
    _lib.check(lib.mk_solver_set_precon_lbfgs(h, H.handle))
    _lib.check(lib.mk_solver_set_precon_lbfgs(h, None))                      # NULL removes it
    _lib.check(lib.mk_solver_set_precon_lbfgs(h, H.handle))
    _lib.check(lib.mk_solver_set_precon_diag(h, None))                       # the other setters replace it
    _lib.check(lib.mk_solver_destroy(h))

    class Part(object):                                                      # a row-partitioned operator
        shape, local_size = (n, n), n // 2

        def __mul__(self, x):
            return x

    with pytest.raises(NotImplementedError, match="single-GPU"):
        pykrylov_amd.generic.KrylovMethod(Part())._device_precon(H)
    with pytest.raises(TypeError):
        H * (rhs + 0j)
    with pytest.raises(TypeError):
        H.store(rhs + 0j, rhs)
    S = np.random.default_rng(3).standard_normal(n)
    assert H.store(S, 2 * S)
    before = (H.s, H.y, H.insert, H.ys)
    for bad in (np.ones(n - 1), np.ones(n + 1), np.ones((n, 1))):
        with pytest.raises(ValueError):
            H.store(S, bad)                                                  # the good half is not written either
        with pytest.raises(ValueError):
            H.store(bad, S)
    with pytest.raises(ValueError):
        H.store(_lib.DeviceArray(n - 1), _lib.DeviceArray(n))
    assert same(H.s, before[0]) and same(H.y, before[1]) and H.insert == before[2] and H.ys == before[3]
    H.free()
    with pytest.raises(ValueError, match="freed"):
        H * rhs
    with pytest.raises(ValueError, match="freed"):
        pykrylov_amd.CG(op, precon=H).solve(rhs)
    small.free()
    op.free()
