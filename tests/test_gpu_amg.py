"""Device smoothed-aggregation AMG preconditioner (pykrylov_amd.tools.amg, csrc/mk_amg.hip): the hierarchy and the applies bit
for bit against the NumPy restatement (tests/_amg_ref.py), solves with the object on the device bit for bit against the same
solves whose preconditioner is the object called back on the host, lifetimes and errors.  Floats are compared as bit patterns
throughout.  No case provokes a fault: every refusal is made before a kernel could read out of range."""
import ctypes

import numpy as np
import pytest

from oracle import csr_ref
from tests import _amg_ref as ref
from test_amg_cpu import ISOLATED_ROW, matrix
from test_gpu_ilu import _solve, device_op, same

pytestmark = pytest.mark.gpu

# (matrix, coarse_max).  169, 400, 512, 1138 and 81 rows: no multiples of the 256 rows of a workgroup, several workgroups,
# several blocks of the device scan (1024 items) in 1138bus.  The first five have at least three rows on every level, so that
# every product of the chunked variant can take three chunks; the sixth ends in a level of ONE row.
CASES = (("poisson2d_20", 16), ("poisson2d_13", 16), ("poisson3d_8", 64), ("1138bus", 20), ("isolated", 16))
ONE_ROW = ("poisson3d_8", 16)
CAP = 40                                                       # entries of an expanded chunk in the chunked variant
VARIANTS = {"base": {}, "chunked": {"expand_cap": CAP}, "seed2": {"seed": 2}}

_REF = {}


def reference(name, **kw):
    """Per argument set, computed once and left unchanged: the matrix, the restated hierarchy, an input vector, the cycle."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _REF:
        A = matrix(name)
        H = ref.build(A, **kw)
        x = np.random.default_rng(11).standard_normal(A.shape[0])
        _REF[key] = (A, H, x, H * x)
    return _REF[key]


def row_counts(X, Y):
    """Entries of the expanded list of every row of X Y."""
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    return np.bincount(rows, weights=np.diff(Y.indptr)[X.indices], minlength=X.shape[0]).astype(np.int64)


def chunks_of(count, cap):
    """Chunks of whole rows of at most `cap` entries, a longer row alone (the rule of the header)."""
    k = r = 0
    while r < len(count):
        s = count[r]
        r += 1
        while r < len(count) and s + count[r] <= cap:
            s += count[r]
            r += 1
        k += 1
    return k


def same_csr(got, want, what):
    ip, ix, v, shape = got
    assert tuple(shape) == tuple(want.shape), what
    assert np.array_equal(ip, want.indptr) and np.array_equal(ix, want.indices), what
    assert same(v, want.data), what


def check_hierarchy(M, H, what, cap=0):
    info, levels = M.info, M.levels
    assert info["levels"] == len(H.levels) == len(levels), what
    assert info["coarse_solver"] == ("inverse" if H.inverse is not None else "smoother"), what
    deg = M.params["degree"]
    assert info["launches"] == (len(levels) - 1) * (7 + 2 * deg) + (1 if H.inverse is not None else 1 + deg)
    over = False
    for l, (lv, got) in enumerate(zip(H.levels, levels)):
        arrays = M.level_arrays(l)
        same_csr(arrays["A"], lv["A"], (what, l, "A"))
        assert same(arrays["lmax"], lv["lmax"]) and same(got["lmax"], lv["lmax"]), (what, l)
        assert (got["rows"], got["nnz"]) == (lv["A"].shape[0], lv["A"].nnz), (what, l)
        if lv["P"] is None:
            assert arrays["P"] is None and arrays["agg"] is None and got["nnz_p"] == 0
            continue
        assert np.array_equal(arrays["agg"], lv["agg"]), (what, l)
        assert (got["aggregates"], got["mis_rounds"], got["nnz_p"]) == (lv["nagg"], lv["rounds"], lv["P"].nnz), (what, l)
        same_csr(arrays["P"], lv["P"], (what, l, "P"))
        same_csr(arrays["R"], lv["R"], (what, l, "R"))
        assert (got["expanded_ap"], got["expanded_rap"]) == (lv["expanded_ap"], lv["expanded_rap"]), (what, l)
        if cap:
            c_ap = row_counts(lv["A"], lv["P"])
            c_rap = row_counts(lv["R"], ref.product(lv["A"], lv["P"])[0])
            c_p = 1 + np.diff(lv["A"].indptr)
            want = (chunks_of(c_ap, cap), chunks_of(c_rap, cap), chunks_of(c_p, cap))
            assert (got["chunks_ap"], got["chunks_rap"], got["chunks_p"]) == want, (what, l)
            if what[:2] != ONE_ROW:
                assert min(want) >= 3, (what, l, want)
            over = over or max(c_ap.max(), c_rap.max()) > cap
        else:
            assert (got["chunks_ap"], got["chunks_rap"], got["chunks_p"]) == (1, 1, 1)
    assert not cap or over, "no row of a product exceeds the cap"
    inv = M.coarse_inverse()
    if H.inverse is None:
        assert inv is None
    else:
        assert inv.shape == H.inverse.shape and same(inv, H.inverse), what
    assert same(M.operator_complexity, H.operator_complexity) and same(M.grid_complexity, H.grid_complexity)
    assert info["operator_complexity_x1000"] == int(np.floor(1000 * H.operator_complexity + 0.5))
    assert info["bytes"] > 0 and info["setup_us"] >= 0 and M.symmetric and M.shape == H.shape


# ------------------------------------------------------------------ hierarchy
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name,coarse_max", CASES + (ONE_ROW,))
def test_hierarchy_bits(name, coarse_max, variant):
    """agg, the MIS round count, the arrays of P, R and A_l, lmax on every level and the coarse inverse equal the restatement;
    with chunks of at most 40 expanded entries (every product in three chunks or more, rows longer than the cap) the same bits
    as with one chunk; with another seed another hierarchy, again the restatement's."""
    from pykrylov_amd import tools
    kw = dict(VARIANTS[variant])
    A, H, x, z = reference(name, coarse_max=coarse_max, **{k: v for k, v in kw.items() if k != "expand_cap"})
    assert len(H.levels) >= (3 if name == "poisson2d_20" else 2)
    op = device_op(A, True)
    M = tools.amg(op, coarse_max=coarse_max, **kw)
    check_hierarchy(M, H, (name, coarse_max, variant), cap=kw.get("expand_cap", 0))
    assert same(M * x, z)
    if name == "isolated":
        agg = M.level_arrays(0)["agg"]
        assert int((agg == agg[ISOLATED_ROW]).sum()) == 1
    M.free()
    op.free()


def test_default_arguments_and_a_single_level():
    """The defaults (coarse_max = 256): poisson2d(13) is one level, its dense inverse; 1138bus three levels."""
    from pykrylov_amd import tools
    for name in ("poisson2d_13", "1138bus"):
        A, H, x, z = reference(name)
        op = device_op(A, True)
        M = tools.amg(op)
        check_hierarchy(M, H, (name, "defaults"))
        assert M.info["levels"] == (1 if name == "poisson2d_13" else 3)
        assert same(M * x, z)
        M.free()
        op.free()


# ------------------------------------------------------------------ apply
APPLY = (("poisson2d_20", dict(coarse_max=16)),                # the dense inverse on the coarsest level
         ("poisson2d_20", dict(coarse_max=16, max_levels=2)),  # the smoother alone
         ("poisson2d_20", dict(coarse_max=16, degree=3)),
         ("1138bus", dict(coarse_max=20)))


FORCED = (0, 1, 2, 3, 4)
IN_USE = {}                                                    # requested storage -> storages the level matrices ended in


@pytest.mark.parametrize("fmt", FORCED + (-1,), ids=["format%d" % f for f in FORCED] + ["default_format"])
@pytest.mark.parametrize("name,kw", APPLY, ids=["inverse", "smoother", "degree3", "1138bus"])
def test_apply_bits(name, kw, fmt):
    """`M * x`, mk_amg_apply out of place (the input unchanged), with in == out and through `apply_device` equal the restated
    cycle byte for byte, with A and every P and R forced into storage formats 0 .. 4 (a request a matrix cannot take degrades;
    which storage every level matrix ended in is recorded for test_apply_bits_ran_in_the_forced_storages) and in the formats
    the builder chooses."""
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    A, H, x, z = reference(name, **kw)
    assert (H.inverse is None) == ("max_levels" in kw)
    op = device_op(A, True)
    if fmt >= 0:
        _lib.check(lib.mk_csr_set_format(op.handle, fmt))
    M = tools.amg(op, **kw)
    if fmt >= 0:
        for l in range(M.info["levels"]):
            for h in M.level_handles(l):
                if h is not None:
                    _lib.check(lib.mk_csr_set_format(h, fmt))
    assert same(M * x, z), (name, kw, fmt)
    d_in, d_out = _lib.DeviceArray.from_numpy(x), _lib.DeviceArray(A.shape[0])
    _lib.check(lib.mk_amg_apply(M.handle, d_in.ptr, d_out.ptr))
    assert same(d_out.to_numpy(), z) and same(d_in.to_numpy(), x), (name, kw, fmt)
    _lib.check(lib.mk_amg_apply(M.handle, d_in.ptr, d_in.ptr))
    assert same(d_in.to_numpy(), z), (name, kw, fmt)
    d_in.upload(x)
    M.apply_device(d_in, d_out)
    M.apply_device(d_out, d_out)
    assert same(d_out.to_numpy(), H * z), (name, kw, fmt)
    got = ctypes.c_int32()
    for l in range(M.info["levels"]):                          # (after the applies: what the residual and correction ran in)
        for h in M.level_handles(l):
            if h is not None:
                _lib.check(lib.mk_csr_format_info(h, ctypes.byref(got), None, None, None, None))
                IN_USE.setdefault(fmt, set()).add(got.value)
    print("%s %s: request %d, storages of the level matrices %s" % (name, kw, fmt, sorted(IN_USE[fmt])))
    _lib.check(lib.mk_csr_format_info(op.handle, ctypes.byref(got), None, None, None, None))
    print("%s %s: format of A in use %d" % (name, kw, got.value))
    if fmt == 0:
        assert got.value == 0
    d_in.free()
    d_out.free()
    M.free()
    op.free()


def test_apply_bits_ran_in_the_forced_storages():
    """MkAmgEpi (residual and correction of the V-cycle) met every storage 0 .. 4: each was in use by at least one level
    matrix of the case that asked for it."""
    for fmt in FORCED:
        assert fmt in IN_USE.get(fmt, ()), (fmt, IN_USE)


# ------------------------------------------------------------------ routes
def _host_twin(M):
    from pykrylov_amd import LinearOperator
    n = M.shape[0]
    calls = [0]

    def mv(v):
        calls[0] += 1
        return M * v
    return LinearOperator(n, n, matvec=mv, symmetric=True), calls


def _amg_for(name, op):
    from pykrylov_amd import tools
    return tools.amg(op) if name == "1138bus" else tools.amg(op, coarse_max=16)


@pytest.mark.parametrize("solver,name", [(s, "poisson2d_20") for s in ("cg", "bicgstab", "cgs", "tfqmr", "symmlq")]
                         + [("minres", "1138bus"), ("cg", "1138bus")])
def test_solver_with_the_device_object_matches_the_callback_path(solver, name):
    """precon=M on the device route against the same object called back on the host: counts, histories and x
    byte-identical.  The loops stop inside a batch of enqueued passes, so the cycles enqueued after the stop are part of what
    is compared: they must change nothing."""
    from pykrylov_amd.generic import resolve_precon
    A = matrix(name)
    op = device_op(A, True)
    rhs = A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))
    M = _amg_for(name, op)
    assert resolve_precon(M, A.shape[0], "precon", solver)[0] == "amg"
    host, calls = _host_twin(M)
    assert resolve_precon(host, A.shape[0], "precon", solver)[0] == "host"
    k0, h0, x0 = _solve(solver, op, rhs, M)
    k1, h1, x1 = _solve(solver, op, rhs, host)
    k2, _, _ = _solve(solver, op, rhs, None)
    print("%s on %s: %d with AMG, %d without" % (solver, name, k0, k2))
    # (fewer passes with the cycle than without is asked of MINRES only: the reference's CG builds its search direction from
    #  r, not from precon * r -- cg.py:104,150-151, kept bit for bit -- and gains nothing from any preconditioner)
    assert calls[0] > 1 and k0 > 1 and (k0 < k2 or solver != "minres")
    assert k0 == k1 and same(h0, h1) and same(x0, x1), (solver, name, k0, k1)
    M.free()
    op.free()


@pytest.mark.parametrize("cls", ["GMRES", "IDR"])
def test_gmres_and_idr_with_the_device_object_match_the_callback_path(cls):
    import pykrylov_amd
    A = matrix("poisson2d_20")
    op = device_op(A, True)
    rhs = A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))
    M = _amg_for("poisson2d_20", op)
    host, calls = _host_twin(M)
    runs = []
    for p in (M, host):
        s = getattr(pykrylov_amd, cls)(op, reltol=1e-10, abstol=1e-8, precon=p)
        s.solve(rhs, matvec_max=60, **({"restart": 9} if cls == "GMRES" else {"s": 4}))
        runs.append(s)
    s, t = runs
    assert s.precon_route == "amg" and t.precon_route == "host" and calls[0] > 1 and s.nMatvec > 1
    assert s.nMatvec == t.nMatvec and same(s.residHistory, t.residHistory) and same(s.x, t.x), cls
    M.free()
    op.free()


def test_solver_route_is_amg_and_a_budget_stop_inside_a_batch_changes_nothing():
    """DeviceRun names the route; a solve stopped by `matvec_max` after 5 products (inside the first batch of passes) leaves
    the vectors of the callback path, whose callback is not invoked once the loop has halted."""
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun, HostPrecon
    A = matrix("poisson2d_20")
    op = device_op(A, True)
    rhs = A.matvec(np.ones(A.shape[0]))
    M = _amg_for("poisson2d_20", op)
    host, _ = _host_twin(M)
    out = []
    for p in (M, HostPrecon(host)):
        run = DeviceRun(op, _lib.MK_BICGSTAB, rhs, None, precon_diag=p, abstol=0.0, reltol=0.0, matvec_max=5)
        assert run.precon_kind == ("amg" if p is M else "host")
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
@pytest.mark.parametrize("solver", ["lsqr", "craigmr"])
def test_least_squares_with_the_device_object_matches_the_callback_path(solver, tag, side):
    """The object as M (nrows(A) entries) and as N (ncols(A) entries) of LSQR / CRAIG-MR on the tall matrices of
    tests/test_gpu_lls_device_precon.py: every result of the solve byte-identical to the same object behind a plain function
    (called back on the host), and `precon_route` reads 'amg'."""
    from pykrylov_amd import tools
    from test_gpu_lls import op_from
    from test_gpu_lls_device_precon import problem, record, through_callbacks, tridiag
    A, b = problem(tag)
    k = A.shape[0] if side == "M" else A.shape[1]
    T = op_from(tridiag(k, 1 if side == "M" else 2), symmetric=True)
    P = tools.amg(T, coarse_max=8)
    assert P.info["levels"] >= 2
    kw = {side: P}
    extra = {} if tag == "small" else {"itnlim": 25}
    dev, route, got = record(solver, A, b, kw, **extra)
    calls = {}
    host, route_h, _ = record(solver, A, b, through_callbacks(kw, calls), **extra)
    other = "N" if side == "M" else "M"
    assert route == {side: "amg", other: "none"} and route_h == {side: "host", other: "none"}
    assert calls[side] > 1 and got["itn"] > 1
    assert dev == host, (solver, tag, side, [k for k in dev if dev[k] != host[k]])
    with pytest.raises(ValueError, match="shape"):
        record(solver, A, b, {other: P}, itnlim=2)               # the other side has another size
    P.free()
    T.free()


# ------------------------------------------------------------------ errors and lifetime
def test_lifetimes():
    """free() while a solver holds the object, then solve: the bits of a solve with a live object; free() twice; use after
    free(): ValueError; the matrix freed first: the object still applies (the library keeps the matrix until the object
    goes)."""
    import pykrylov_amd
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    A, H, x, z = reference("poisson2d_20", coarse_max=16)
    op = device_op(A, True)
    rhs = A.matvec(np.ones(A.shape[0]))
    M = _amg_for("poisson2d_20", op)
    s_ref = pykrylov_amd.BiCGSTAB(op, precon=M, reltol=1e-10)
    s_ref.solve(rhs, matvec_max=400)
    run = DeviceRun(op, _lib.MK_BICGSTAB, rhs, None, precon_diag=M, abstol=1e-8, reltol=1e-10, matvec_max=400)
    M.free()                                                    # the solver still holds the object ...
    M.free()                                                    # (twice: nothing happens)
    for use in (lambda: M * x, lambda: M.handle, lambda: M.info, lambda: M.levels, lambda: M.level_arrays(0),
                lambda: M.coarse_inverse(), lambda: M.operator_complexity):
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
    # the matrix destroyed first: the object still applies
    M = _amg_for("poisson2d_20", op)
    op.free()
    assert same(M * x, z)
    M.free()


def test_errors():
    from pykrylov_amd import CsrOperator, LinearOperator, _lib, tools
    A = matrix("poisson2d_13")
    n = A.shape[0]
    with pytest.raises(ValueError, match="symmetric"):
        tools.amg(device_op(A, False))
    R = device_op(csr_ref.from_coo(np.array([0, 1]), np.array([0, 1]), np.array([1.0, 1.0]), (2, 3)), True)
    with pytest.raises(ValueError, match="square"):
        tools.amg(R)
    lib = _lib.init()
    h = ctypes.c_void_p()
    assert lib.mk_amg_create(R.handle, 0.0, 1, 4.0, 4.0 / 3.0, 256, 10, 1, 0, ctypes.byref(h)) == -2       # MK_ERR_ARG
    assert b"square" in lib.mk_last_error()
    with pytest.raises(TypeError, match="CSR"):
        tools.amg(LinearOperator(n, n, matvec=lambda v: A.matvec(v), symmetric=True))      # a callback operator
    op = device_op(A, True)
    S = op + op                                                 # a composite: no arrays of its own
    with pytest.raises((TypeError, _lib.MkError), match="to_csr_arrays"):
        tools.amg(S)
    op.local_size = n // 2                                      # what the package recognises a partitioned operator by
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        tools.amg(op)
    del op.local_size
    for bad in (dict(degree=0), dict(ratio=1.0), dict(omega=0.0), dict(theta=-1.0), dict(coarse_max=0), dict(coarse_max=1025),
                dict(max_levels=17), dict(seed=-1), dict(expand_cap=-1)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            tools.amg(op, **bad)
    # ... and by the library, for a caller of the C entry point
    for args in ((-1.0, 1, 4.0, 1.0, 256, 10), (0.0, 0, 4.0, 1.0, 256, 10), (0.0, 1, 1.0, 1.0, 256, 10), (0.0, 1, 4.0, 0.0, 256, 10),
                 (0.0, 1, 4.0, 1.0, 1025, 10), (0.0, 1, 4.0, 1.0, 256, 17)):
        assert lib.mk_amg_create(op.handle, *args, 1, 0, ctypes.byref(h)) == -2, args
    # a negative and a zero diagonal entry in rows 77 and 90, a missing one in row 5: the smallest row is named
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    for value in (-4.0, 0.0):
        data = np.where((rows == A.indices) & ((rows == 77) | (rows == 90)), value, A.data)
        B = CsrOperator(A.indptr, A.indices, data, A.shape, symmetric=True)
        with pytest.raises(ValueError, match="row 77 of level 0"):
            tools.amg(B, coarse_max=16)
        B.free()
    keep = ~((rows == A.indices) & (rows == 5))
    C = device_op(csr_ref.from_coo(rows[keep], A.indices[keep], A.data[keep], A.shape), True)
    with pytest.raises(ValueError, match="row 5 of level 0"):
        tools.amg(C, coarse_max=16)
    M = tools.amg(op, coarse_max=16, max_levels=2)
    assert M.coarse_inverse() is None
    assert lib.mk_amg_coarse(M.handle, np.empty(4).ctypes.data) == -3                      # MK_ERR_STATE: no inverse
    assert lib.mk_amg_level(M.handle, 1, 1, ctypes.byref(h)) == -2                          # the last level has no P
    assert lib.mk_amg_level(M.handle, 2, 0, ctypes.byref(h)) == -2
    M.free()
    for o in (R, S, op, C):
        o.free()
