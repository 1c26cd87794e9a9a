"""Device ILU(0) / IC(0) (pykrylov_amd.tools.ilu0 / ic0, mk_ilu.hip): factors and applies bit for bit against the CPU
restatement (tests/_ilu_ref.py), solves with the factor on the device bit for bit against the same solves whose
preconditioner is the reference apply called back on the host, errors and lifetimes."""
import os

import numpy as np
import pytest

from oracle import csr_ref
from tests import _ilu_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def ref_matrix(name):
    if name == "jpwh_991":
        return csr_ref.read_matrix_market(os.path.join(GOLDEN, "jpwh_991.mtx"))
    if name == "1138bus":
        return csr_ref.read_matrix_market(os.path.join(GOLDEN, "1138bus.mtx"))       # expanded to full storage
    if name == "random_diagdom_1e4":
        return csr_ref.random_diagdom(10 ** 4)
    if name == "poisson2d_100":
        return csr_ref.poisson2d(100)
    if name == "varcoef_20_20_5":
        return csr_ref.poisson3d_varcoef(20, 20, 5)
    if name == "stored_zeros":                      # a 2-D Laplacian with explicit zeros in and beside the pattern
        A = csr_ref.poisson2d(12)
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        far = (rows + 7) % A.shape[0]
        keep = far != rows
        r = np.concatenate([rows, rows[keep]])
        c = np.concatenate([A.indices, far[keep]])
        v = np.concatenate([A.data, np.zeros(int(keep.sum()))])
        return csr_ref.from_coo(r, c, v, A.shape)
    if name == "diagonal":
        n = 300
        d = 1.0 + np.random.default_rng(5).random(n)
        return csr_ref.from_coo(np.arange(n), np.arange(n), d, (n, n))
    raise KeyError(name)


SYMMETRIC = ("1138bus", "poisson2d_100", "varcoef_20_20_5", "diagonal")
ALL = ("jpwh_991", "1138bus", "random_diagdom_1e4", "poisson2d_100", "varcoef_20_20_5", "stored_zeros", "diagonal")


def device_op(A, symmetric):
    from pykrylov_amd import CsrOperator
    return CsrOperator(A.indptr, A.indices, A.data, A.shape, symmetric=symmetric)


@pytest.fixture(params=["fused", "unfused"])
def fusion(request, monkeypatch):
    if request.param == "unfused":
        monkeypatch.setenv("MK_ILU_FUSE_ROWS", "0")
    else:
        monkeypatch.delenv("MK_ILU_FUSE_ROWS", raising=False)
    return request.param


_REF_CACHE = {}


def reference(name, kind):
    key = (name, kind)
    if key not in _REF_CACHE:
        A = ref_matrix(name)
        vals = (ref.ic0 if kind == "ic0" else ref.ilu0)(A.indptr, A.indices, A.data)
        _REF_CACHE[key] = (A, vals)
    return _REF_CACHE[key]


@pytest.mark.parametrize("name", ALL)
def test_factor_and_apply_bits(name, fusion):
    from pykrylov_amd import tools
    kinds = ("ilu0", "ic0") if name in SYMMETRIC else ("ilu0",)
    for kind in kinds:
        A, vals = reference(name, kind)
        op = device_op(A, symmetric=name in SYMMETRIC)
        M = getattr(tools, kind)(op)
        ip, ix, v, dg = M.factor_arrays()
        assert np.array_equal(ip, A.indptr) and np.array_equal(ix, A.indices)
        assert np.array_equal(dg, ref.diag_positions(A.indptr, A.indices))
        assert same(v, vals), (name, kind, fusion)
        fw, bw = ref.levels(A.indptr, A.indices, True), ref.levels(A.indptr, A.indices, False)
        info = M.info
        assert M.levels == (len(fw), len(bw))
        assert info["widest_level"] == max(len(r) for r in fw + bw)
        if fusion == "unfused":
            assert M.launches == M.levels and info["fuse_rows"] == 0
        assert info["bytes"] >= 8 * A.nnz
        x = np.random.default_rng(11).standard_normal(A.shape[0])
        want = ref.apply(A.indptr, A.indices, vals, x, kind)
        assert same(want, ref.apply_rows(A.indptr, A.indices, vals, x, kind))
        assert same(M * x, want), (name, kind, fusion)
        # in place and out of place on device pointers
        from pykrylov_amd import _lib
        lib = _lib.init()
        d_in, d_out = _lib.DeviceArray.from_numpy(x), _lib.DeviceArray(A.shape[0])
        _lib.check(lib.mk_ilu_apply(M.handle, d_in.ptr, d_out.ptr))
        assert same(d_out.to_numpy(), want) and same(d_in.to_numpy(), x)
        _lib.check(lib.mk_ilu_apply(M.handle, d_in.ptr, d_in.ptr))
        assert same(d_in.to_numpy(), want)
        d_in.free()
        d_out.free()
        M.free()
        op.free()


def test_jpwh991_takes_one_launch_per_sweep_under_default_fusion(monkeypatch):
    from pykrylov_amd import tools
    monkeypatch.delenv("MK_ILU_FUSE_ROWS", raising=False)
    A = ref_matrix("jpwh_991")
    op = device_op(A, False)
    M = tools.ilu0(op)
    assert M.levels == (37, 37) and M.launches == (1, 1)
    M.free()
    op.free()


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


@pytest.mark.parametrize("solver,name", [(s, m) for s in ("bicgstab", "cgs", "tfqmr") for m in ("jpwh_991", "random_diagdom_1e4")]
                         + [(s, m) for s in ("minres", "symmlq", "cg") for m in ("poisson2d_100", "1138bus")])
def test_solver_with_device_factor_matches_the_callback_path(solver, name):
    from pykrylov_amd import tools
    kind = "ic0" if name in SYMMETRIC else "ilu0"
    A, vals = reference(name, kind)
    op = device_op(A, symmetric=name in SYMMETRIC)
    rhs = A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))
    M = getattr(tools, kind)(op)
    host = ref.HostIlu(A.indptr, A.indices, vals, kind, vectorised=True)
    k0, h0, x0 = _solve(solver, op, rhs, M)
    k1, h1, x1 = _solve(solver, op, rhs, host)
    assert host.calls > 1
    assert k0 == k1 and same(h0, h1) and same(x0, x1), (solver, name, k0, k1)
    M.free()
    op.free()


@pytest.mark.slow
def test_full_size_bicgstab_random_diagdom_1e6():
    import pykrylov_amd
    from pykrylov_amd import gallery, tools
    op = gallery.random_diagdom(10 ** 6)
    ip, ix, data = op.to_csr_arrays()
    A = csr_ref.RefCsr(ip, ix, data, op.shape)
    rhs = A.matvec(np.ones(op.shape[0]))
    M = tools.ilu0(op)
    _, _, vals, _ = M.factor_arrays()
    runs = []
    for precon in (M, ref.HostIlu(ip, ix, vals, "ilu0", vectorised=True), None):
        s = pykrylov_amd.BiCGSTAB(op, precon=precon, reltol=1e-8, abstol=0.0)
        s.solve(rhs, matvec_max=2000)
        runs.append((s.nMatvec, s.converged, s.residNorm, s.x))
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2] and same(runs[0][3], runs[1][3])
    assert runs[0][1] and runs[2][1] and runs[0][0] < runs[2][0], (runs[0][:3], runs[2][:3])
    print("BiCGSTAB 1e-8 on random_diagdom(1e6): ilu0 %d matvecs, none %d (ratio %.2f)"
          % (runs[0][0], runs[2][0], runs[0][0] / runs[2][0]))
    M.free()
    op.free()


@pytest.mark.slow
def test_full_size_apply_poisson3d_128():
    from pykrylov_amd import gallery, tools
    op = gallery.poisson3d(128)
    for kind in ("ilu0", "ic0"):
        M = getattr(tools, kind)(op)
        ip, ix, vals, _ = M.factor_arrays()
        x = np.random.default_rng(9).standard_normal(op.shape[0])
        assert same(M * x, ref.apply(ip, ix, vals, x, kind)), kind
        assert M.levels == (382, 382)
        M.free()
    op.free()


def test_errors():
    from pykrylov_amd import _lib, tools
    from pykrylov_amd import CsrOperator
    Z = CsrOperator(np.array([0, 2, 4]), np.array([0, 1, 0, 1]), np.array([0.0, 1.0, 1.0, 0.0]), (2, 2))
    with pytest.raises(_lib.MkError, match="zero pivot in row 0"):
        tools.ilu0(Z)
    N = CsrOperator(np.array([0, 1, 2]), np.array([1, 0]), np.array([1.0, 1.0]), (2, 2), symmetric=True)
    with pytest.raises(_lib.MkError, match="row 0 stores no diagonal"):
        tools.ilu0(N)
    with pytest.raises(_lib.MkError, match="row 0 stores no diagonal"):
        tools.ic0(N)
    B = CsrOperator(np.array([0, 2, 4]), np.array([0, 1, 0, 1]), np.array([1.0, 2.0, 2.0, 1.0]), (2, 2), symmetric=True)
    with pytest.raises(_lib.MkError, match="breakdown in row 1"):
        tools.ic0(B)
    P = CsrOperator(np.array([0, 2, 3]), np.array([0, 1, 1]), np.array([1.0, 2.0, 1.0]), (2, 2), symmetric=True)
    with pytest.raises(_lib.MkError, match="not symmetric"):
        tools.ic0(P)
    A = device_op(csr_ref.poisson2d(6), True)
    S = A + A                                                   # a composite: no arrays of its own
    with pytest.raises(_lib.MkError, match="to_csr_arrays"):
        tools.ilu0(S)
    with pytest.raises(ValueError):
        tools.ilu0(device_op(csr_ref.from_coo(np.array([0]), np.array([0]), np.array([1.0]), (2, 3)), False))
    for o in (Z, N, B, P, S, A):
        o.free()


def test_solver_keeps_the_factor_alive_and_halted_applies_change_nothing():
    import pykrylov_amd
    from pykrylov_amd import _lib, tools
    from pykrylov_amd.generic import DeviceRun
    A = ref_matrix("jpwh_991")
    _, vals = reference("jpwh_991", "ilu0")
    op = device_op(A, False)
    rhs = A.matvec(np.ones(A.shape[0]))
    host = ref.HostIlu(A.indptr, A.indices, vals, "ilu0", vectorised=True)
    s_ref = pykrylov_amd.BiCGSTAB(op, precon=host, reltol=1e-10)
    s_ref.solve(rhs, matvec_max=400)
    M = tools.ilu0(op)
    run = DeviceRun(op, _lib.MK_BICGSTAB, rhs, None, precon_diag=M, abstol=1e-8, reltol=1e-10, matvec_max=400)
    M.free()                                                    # the solver still holds the factor ...
    op.free()                                                   # ... and the factor the matrix
    res = run.run()
    x = run.x()
    assert res.nMatvec == s_ref.nMatvec and same(x, s_ref.x)
    # the loop has halted: more passes change nothing (every launch of the apply is a no-op)
    assert run.iterate(5) == 0
    assert same(run.x(), x)
    run.close()


def test_apply_after_halt_is_a_no_op_at_every_site():
    """A solve stopped by its iteration budget: the vectors after the stop equal those of the callback path, whose
    callback is not invoked once the loop has halted."""
    from pykrylov_amd import _lib, tools
    from pykrylov_amd.generic import DeviceRun, HostPrecon
    A, vals = reference("random_diagdom_1e4", "ilu0")
    op = device_op(A, False)
    rhs = A.matvec(np.ones(A.shape[0]))
    M = tools.ilu0(op)
    host = ref.HostIlu(A.indptr, A.indices, vals, "ilu0", vectorised=True)
    out = []
    for p in (M, HostPrecon(host)):
        run = DeviceRun(op, _lib.MK_BICGSTAB, rhs, None, precon_diag=p, abstol=0.0, reltol=0.0, matvec_max=5)
        run.run()
        out.append([run.x()] + [run.vector(k) for k in range(2) if _has_vector(run, k)])
        run.close()
    assert len(out[0]) == len(out[1]) and all(same(a, b) for a, b in zip(out[0], out[1]))
    M.free()
    op.free()


def _has_vector(run, k):
    try:
        run.vector(k)
        return True
    except Exception:
        return False
