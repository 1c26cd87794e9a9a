"""Device FSAI preconditioner (pykrylov_amd.tools.fsai, csrc/mk_fsai.hip): the factor and the applies bit for bit against the
NumPy restatement (tests/_fsai_ref.py), solves with the object on the device bit for bit against the same solves whose
preconditioner is the object called back on the host, that it preconditions, lifetimes and errors.  Floats are compared as
bit patterns throughout.  No case provokes a fault: every refusal is made before a kernel could read out of range."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref, gpu_order, krylov_ref as kr
from tests import _fsai_ref as ref
from test_gpu_ilu import _solve, device_op, ref_matrix, same

pytestmark = pytest.mark.gpu

# (matrix, power): every row count is no multiple of the rows a workgroup handles (256, 32 or 8).  Longest rows: 3 / 7,
# 3 / 7, 11 / 30, 4 / 13, 4 / 13, 1, 1, 14 -- the register kernel (<= 4), the 8-lane kernel (<= 16) and the 32-lane kernel
CASES = (("poisson2d_12", 1), ("poisson2d_12", 2), ("poisson2d_100", 1), ("poisson2d_100", 2), ("1138bus", 1),
         ("1138bus", 2), ("varcoef_20_20_5", 1), ("varcoef_20_20_5", 2), ("stored_zeros", 1), ("stored_zeros", 2),
         ("diagonal", 1), ("diagonal", 2), ("one_by_one", 1), ("stencil27_6", 1))


def banded(hb, n=100):
    """SPD band matrix: a_ii = 8, a_ij = -1 / (1 + |i - j|) for 0 < |i - j| <= hb (diagonally dominant up to hb = 32:
    2 (H_33 - 1) = 6.2 < 8).  Rows from hb on hold hb + 1 entries on and below the diagonal."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = np.abs(i - j) <= hb
    v = np.where(i == j, 8.0, -1.0 / (1.0 + np.abs(i - j)))
    return csr_ref.from_coo(i[keep], j[keep], v[keep], (n, n))


_MAT = {}


def matrix(name):
    if name not in _MAT:
        if name == "poisson2d_12":
            _MAT[name] = csr_ref.poisson2d(12)
        elif name == "one_by_one":
            _MAT[name] = csr_ref.from_coo(np.array([0]), np.array([0]), np.array([2.5]), (1, 1))
        elif name == "stencil27_6":
            _MAT[name] = csr_ref.stencil27(6)
        elif name.startswith("banded_"):
            _MAT[name] = banded(int(name[7:]))
        else:
            _MAT[name] = ref_matrix(name)
    return _MAT[name]


_REF = {}


def reference(name, power):
    """Per (matrix, power), computed once: the matrix, the factor, an input vector and the apply."""
    if (name, power) not in _REF:
        A = matrix(name)
        G = ref.factor(A, power=power)
        x = np.random.default_rng(11).standard_normal(A.shape[0])
        _REF[name, power] = (A, G, x, ref.apply(G, x))
    return _REF[name, power]


def set_formats(M, fmt):
    from pykrylov_amd import _lib
    for h in M.factor_handles():
        _lib.check(_lib.init().mk_csr_set_format(h, fmt))


def check_factor(M, G, what):
    ip, ix, v = M.factor_arrays()
    assert np.array_equal(ip, G.indptr) and np.array_equal(ix, G.indices), what
    assert same(v, G.data), what
    info = M.info
    longest = int(np.diff(G.indptr).max())
    assert (info["rows"], info["nnz"], info["longest_row"], info["launches"]) == (G.shape[0], G.nnz, longest, 2), what
    assert info["bytes"] >= 2 * 12 * G.nnz + 8 * G.shape[0] and info["setup_us"] >= 0
    assert M.symmetric and M.shape == G.shape


@pytest.mark.parametrize("name,power", CASES)
def test_factor_bits(name, power):
    """`factor_arrays()` equals the restatement: the pattern exactly, the values bit for bit."""
    from pykrylov_amd import tools
    A, G, _, _ = reference(name, power)
    op = device_op(A, True)
    M = tools.fsai(op, power=power)
    assert M.power == power
    check_factor(M, G, (name, power))
    M.free()
    op.free()


@pytest.mark.parametrize("hb,longest", [(3, 4), (4, 5), (31, 32)])
def test_row_length_edges(hb, longest):
    """Rows of exactly 4, 5 and 32 entries: the last size of the register kernel, the first of the LDS kernel, and
    MK_FSAI_MAX_ROW."""
    from pykrylov_amd import tools
    A, G, x, z = reference("banded_%d" % hb, 1)
    assert int(np.diff(G.indptr).max()) == longest
    op = device_op(A, True)
    M = tools.fsai(op)
    check_factor(M, G, hb)
    assert same(M * x, z)
    M.free()
    op.free()


def test_rows_that_are_too_long_are_refused():
    from pykrylov_amd import tools
    op = device_op(matrix("banded_32"), True)
    with pytest.raises(ValueError, match=r"row 32 of the pattern has 33 entries.*power"):
        tools.fsai(op)
    op.free()
    op = device_op(matrix("stencil27_6"), True)
    with pytest.raises(ValueError, match=r"row \d+ of the pattern has \d+ entries.*lower `power`"):
        tools.fsai(op, power=2)
    op.free()


def test_explicit_pattern():
    """The pattern tril(A^2) of poisson2d(12), passed as `pattern=`, gives the bits of power = 2."""
    from pykrylov_amd import tools
    A, G, x, z = reference("poisson2d_12", 2)
    op = device_op(A, True)
    M = tools.fsai(op, pattern=ref.power_pattern(A.indptr, A.indices, 2))
    check_factor(M, G, "pattern")
    assert M.power == 1 and same(M * x, z)
    M.free()
    op.free()


@pytest.mark.parametrize("fmt", [0, -1], ids=["format0", "default_format"])
@pytest.mark.parametrize("name,power", CASES)
def test_apply_bits(name, power, fmt):
    """`M * x`, mk_fsai_apply out of place (the input unchanged) and `apply_device` in place equal the restatement byte for
    byte, with G and its transpose in the formats the builder chooses and with format 0 forced on both."""
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    A, G, x, z = reference(name, power)
    op = device_op(A, True)
    M = tools.fsai(op, power=power)
    if fmt >= 0:
        set_formats(M, fmt)
    assert same(M * x, z), (name, power, fmt)
    d_in, d_out = _lib.DeviceArray.from_numpy(x), _lib.DeviceArray(A.shape[0])
    _lib.check(lib.mk_fsai_apply(M.handle, d_in.ptr, d_out.ptr))
    assert same(d_out.to_numpy(), z) and same(d_in.to_numpy(), x), (name, power, fmt)
    M.apply_device(d_in, d_in)
    assert same(d_in.to_numpy(), z), (name, power, fmt)
    info = M.info
    print("%s power %d: formats of G / G' = %d / %d" % (name, power, info["format_g"], info["format_gt"]))
    if fmt == 0:
        assert info["format_g"] == info["format_gt"] == 0
    d_in.free()
    d_out.free()
    M.free()
    op.free()


def _host_twin(M):
    from pykrylov_amd import LinearOperator
    n = M.shape[0]
    calls = [0]

    def mv(v):
        calls[0] += 1
        return M * v
    return LinearOperator(n, n, matvec=mv, symmetric=True), calls


@pytest.mark.parametrize("name", ["poisson2d_100", "1138bus"])
@pytest.mark.parametrize("solver", ["cg", "bicgstab", "cgs", "tfqmr", "minres", "symmlq"])
def test_solver_with_the_device_object_matches_the_callback_path(solver, name):
    """precon=M on the device route against the same object called back on the host: counts, histories and x
    byte-identical.  The loops stop inside a batch of enqueued passes, so the applies enqueued after the stop are part of what
    is compared: they must change nothing."""
    from pykrylov_amd import tools
    A = matrix(name)
    op = device_op(A, True)
    rhs = A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))
    M = tools.fsai(op)
    host, calls = _host_twin(M)
    k0, h0, x0 = _solve(solver, op, rhs, M)
    k1, h1, x1 = _solve(solver, op, rhs, host)
    assert calls[0] > 1 and k0 > 1
    assert k0 == k1 and same(h0, h1) and same(x0, x1), (solver, name, k0, k1)
    M.free()
    op.free()


@pytest.mark.parametrize("name", ["poisson2d_100", "1138bus"])
def test_gmres_with_the_device_object_matches_the_callback_path(name):
    from pykrylov_amd import GMRES, tools
    A = matrix(name)
    op = device_op(A, True)
    rhs = A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))
    M = tools.fsai(op)
    host, calls = _host_twin(M)
    runs = []
    for p in (M, host):
        s = GMRES(op, reltol=1e-10, abstol=1e-8, precon=p)
        s.solve(rhs, restart=9, matvec_max=60)
        runs.append(s)
    s, t = runs
    assert s.precon_route == "fsai" and t.precon_route == "host" and calls[0] > 1 and s.nMatvec > 1
    assert s.nMatvec == t.nMatvec and same(s.residHistory, t.residHistory) and same(s.x, t.x), name
    M.free()
    op.free()


def test_solver_route_is_fsai_and_a_budget_stop_inside_a_batch_changes_nothing():
    """DeviceRun names the route; a solve stopped by its budget after 5 products (inside the first batch of 16 passes)
    leaves the vectors of the callback path, whose callback is not invoked once the loop has halted."""
    from pykrylov_amd import _lib, tools
    from pykrylov_amd.generic import DeviceRun, HostPrecon
    A = matrix("poisson2d_100")
    op = device_op(A, True)
    rhs = A.matvec(np.ones(A.shape[0]))
    M = tools.fsai(op, power=2)
    host, _ = _host_twin(M)
    out = []
    for p in (M, HostPrecon(host)):
        run = DeviceRun(op, _lib.MK_BICGSTAB, rhs, None, precon_diag=p, abstol=0.0, reltol=0.0, matvec_max=5)
        assert run.precon_kind == ("fsai" if p is M else "host")
        run.run()
        vecs = [run.x()]
        for k in range(2):
            try:
                vecs.append(run.vector(k))
            except Exception:
                break
        out.append(vecs)
        run.close()
    assert len(out[0]) == len(out[1]) and all(same(a, b) for a, b in zip(out[0], out[1]))
    M.free()
    op.free()


@pytest.mark.parametrize("side", ["M", "N"])
@pytest.mark.parametrize("tag", ["small", "odd"])
@pytest.mark.parametrize("solver", ["lsqr", "lsmr"])
def test_least_squares_with_the_device_object_matches_the_callback_path(solver, tag, side):
    """The object as M (nrows(A) entries) and as N (ncols(A) entries) of LSQR / LSMR on the tall matrices of
    tests/test_gpu_lls_device_precon.py: every result of the solve byte-identical to the same object behind a plain function
    (called back on the host), and `precon_route` reads 'fsai'."""
    from pykrylov_amd import tools
    from test_gpu_lls import op_from
    from test_gpu_lls_device_precon import problem, record, through_callbacks, tridiag
    A, b = problem(tag)
    k = A.shape[0] if side == "M" else A.shape[1]
    T = op_from(tridiag(k, 1 if side == "M" else 2), symmetric=True)
    P = tools.fsai(T)
    kw = {side: P}
    extra = {} if tag == "small" else {"itnlim": 25}
    dev, route, got = record(solver, A, b, kw, **extra)
    calls = {}
    host, route_h, _ = record(solver, A, b, through_callbacks(kw, calls), **extra)
    other = "N" if side == "M" else "M"
    assert route == {side: "fsai", other: "none"} and route_h == {side: "host", other: "none"}
    assert calls[side] > 1 and got["itn"] > 1
    assert dev == host, (solver, tag, side, [k for k in dev if dev[k] != host[k]])
    with pytest.raises(ValueError, match="shape"):
        record(solver, A, b, {other: P}, itnlim=2)               # the other side has another size
    P.free()
    T.free()


@pytest.mark.parametrize("power", [1, 2])
def test_minres_counts_on_poisson2d_100_equal_the_oracles(power, monkeypatch):
    """MINRES on poisson2d_100, rtol = 1e-10, b = A ones: as many iterations as the CPU restatement of MINRES preconditioned
    by the reference apply (with the device's summation order), and fewer than without a preconditioner."""
    from pykrylov_amd import Minres, tools
    A, G, _, _ = reference("poisson2d_100", power)
    n = A.shape[0]
    rhs = A.matvec(np.ones(n))
    op = device_op(A, True)
    M = tools.fsai(op, power=power)
    s = Minres(op)
    s.solve(rhs, precon=M, show=False, check=False, etol=0.0, rtol=1e-10)
    s0 = Minres(op)
    s0.solve(rhs, show=False, check=False, etol=0.0, rtol=1e-10)
    monkeypatch.setattr(kr, "_sq", lambda a: a * a)              # the reference's pow(x, 2) is not always x*x
    red = kr.Reductions(gpu_order.GpuDots(n, gpu_order.SPMV_SITES["minres"]))
    want = kr.minres(A, rhs, precon=ref.HostFsai(G), check=False, etol=0.0, rtol=1e-10, red=red)
    print("MINRES poisson2d_100: itn %d with fsai(power=%d), oracle %d, %d without" % (s.itn, power, want["itn"], s0.itn))
    assert s.itn == want["itn"] and s.istop == want["istop"] and s.istop in (1, 2)
    assert s.itn < s0.itn
    M.free()
    op.free()


def test_lifetimes():
    """free() while a solver holds the object, then solve again: same bits; free() twice; use after free(): ValueError; the
    matrix freed first: the object still applies (it keeps nothing of the matrix)."""
    import pykrylov_amd
    from pykrylov_amd import _lib, tools
    from pykrylov_amd.generic import DeviceRun
    A, G, x, z = reference("poisson2d_100", 1)
    op = device_op(A, True)
    rhs = A.matvec(np.ones(A.shape[0]))
    M = tools.fsai(op)
    s_ref = pykrylov_amd.BiCGSTAB(op, precon=M, reltol=1e-10)
    s_ref.solve(rhs, matvec_max=400)
    run = DeviceRun(op, _lib.MK_BICGSTAB, rhs, None, precon_diag=M, abstol=1e-8, reltol=1e-10, matvec_max=400)
    M.free()                                                    # the solver still holds the object ...
    M.free()                                                    # (twice: nothing happens)
    for use in (lambda: M * x, lambda: M.handle, lambda: M.info, lambda: M.factor_arrays(), lambda: M.factor_handles()):
        with pytest.raises(ValueError, match="freed"):
            use()
    d = _lib.DeviceArray.from_numpy(x)
    with pytest.raises(ValueError, match="freed"):
        M.apply_device(d, d)
    d.free()
    res = run.run()
    xs = run.x()
    assert res.nMatvec == s_ref.nMatvec and same(xs, s_ref.x)
    assert run.iterate(5) == 0 and same(run.x(), xs)            # halted: further passes change nothing
    run.close()
    # the matrix freed first: the object still applies
    M = tools.fsai(op)
    op.free()
    assert same(M * x, z)
    M.free()


def test_errors():
    from pykrylov_amd import CsrOperator, _lib, tools
    A = matrix("poisson2d_12")
    n = A.shape[0]
    with pytest.raises(ValueError, match="symmetric"):
        tools.fsai(device_op(A, False))
    R = device_op(csr_ref.from_coo(np.array([0, 1]), np.array([0, 1]), np.array([1.0, 1.0]), (2, 3)), True)
    with pytest.raises(ValueError, match="square"):
        tools.fsai(R)
    op = device_op(A, True)
    S = op + op                                                 # a composite: no arrays of its own
    with pytest.raises((TypeError, _lib.MkError), match="to_csr_arrays"):
        tools.fsai(S)
    op.local_size = n // 2                                      # what the package recognises a partitioned operator by
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        tools.fsai(op)
    del op.local_size
    for power in (0, 4, 1.5, True):
        with pytest.raises(ValueError, match="power"):
            tools.fsai(op, power=power)
    ip, ix = ref.power_pattern(A.indptr, A.indices, 1)
    with pytest.raises(ValueError, match="pattern"):
        tools.fsai(op, power=2, pattern=(ip, ix))
    # an upper entry in row 5, an unsorted row 9, a missing diagonal in row 20: the first bad row is named
    rows = np.repeat(np.arange(n), np.diff(ip))
    up = ix.copy()
    up[ip[6] - 1] = 6                                           # row 5 ends with column 6
    with pytest.raises(_lib.MkError, match="row 5 .*lower triangular"):
        tools.fsai(op, pattern=(ip, up))
    assert ip[10] - ip[9] >= 2
    uns = ix.copy()
    uns[ip[9]], uns[ip[9] + 1] = ix[ip[9] + 1], ix[ip[9]]
    bad_late = uns.copy()
    bad_late[ip[31] - 1] = 32                                   # (a later bad row does not change the message)
    for cand in (uns, bad_late):
        with pytest.raises(_lib.MkError, match="row 9 .*not sorted"):
            tools.fsai(op, pattern=(ip, cand))
    keep = ~((rows == 20) & (ix == 20))
    ip2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))])
    with pytest.raises(_lib.MkError, match="row 20 .*diagonal"):
        tools.fsai(op, pattern=(ip2, ix[keep]))
    with pytest.raises(ValueError, match="indptr"):
        tools.fsai(op, pattern=(ip[:-1], ix))
    # a_77,77 = -1: the dense solves of rows 77, 78 and 89 break down; the smallest is named
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    data = np.where((rows == 77) & (A.indices == 77), -1.0, A.data)
    B = CsrOperator(A.indptr, A.indices, data, A.shape, symmetric=True)
    with pytest.raises(_lib.MkError, match="breakdown in row 77"):
        tools.fsai(B)
    with pytest.raises(_lib.MkError, match="breakdown in row 77"):
        tools.fsai(B, power=2)                                  # (the LDS kernel)
    # a matrix that does not store the diagonal of row 3
    keep = ~((rows == 3) & (A.indices == 3))
    C = csr_ref.from_coo(rows[keep], A.indices[keep], A.data[keep], A.shape)
    Cop = device_op(C, True)
    with pytest.raises(_lib.MkError, match="row 3 stores no diagonal"):
        tools.fsai(Cop)
    lib = _lib.init()
    h = ctypes.c_void_p()
    ip32 = np.ascontiguousarray(ip, dtype=np.int32)
    assert lib.mk_fsai_create(op.handle, ip32.ctypes.data, None, ctypes.byref(h)) == -2        # MK_ERR_ARG: half a pattern
    for o in (R, S, op, B, Cop):
        o.free()
