"""Device-resident preconditioners M and N in LSQR / LSMR / CRAIG / CRAIG-MR (csrc/mk_lls.hip, the two MkPrecon slots):
a device matrix, a block-Jacobi composite, an IC(0) factor and an inverse L-BFGS operator are applied at the
`u = M(Mu)` / `v = N(Nv)` sites without leaving HBM, and give the bits of the same object called back on the host --
through the whole solve, after the loop has halted, and when beta = 0 keeps N from being applied (lsqr.py:258).
Floats are compared as bit patterns throughout."""
import ctypes
import os

import numpy as np
import pytest

from oracle import csr_ref, gpu_order, krylov_ref as kr, lls_ref
from test_gpu_lls import golden_csr, op_from, run_device, run_oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOLVERS = ("lsqr", "lsmr", "craig", "craigmr")
KINDS = ("csr", "ic0", "lbfgs", "bj")
ROUTE = {"csr": "device", "bj": "device", "ic0": "ilu", "lbfgs": "lbfgs"}
# (kind of M, kind of N): every kind on M, on N, and one mixed pair
CASES = [(k, None) for k in KINDS] + [(None, k) for k in KINDS] + [("ic0", "lbfgs")]
CASE_IDS = ["M=%s,N=%s" % c for c in CASES]


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).tobytes()


def tridiag(k, seed, first=None):
    """SPD tridiagonal matrix like `spd()` of test_gpu_lls.py, as an oracle CSR; `first` cuts row / column 0 loose and puts
    that value on its diagonal."""
    rng = np.random.default_rng(seed)
    d = 2.0 + rng.random(k)
    rows, cols, vals = [], [], []
    for i in range(k):
        for j, v in ((i - 1, -0.5), (i, d[i]), (i + 1, -0.5)):
            if 0 <= j < k:
                rows.append(i), cols.append(j), vals.append(v)
    rows, cols, vals = np.array(rows), np.array(cols), np.array(vals)
    if first is not None:
        keep = ((rows == 0) == (cols == 0))
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
        vals[(rows == 0) & (cols == 0)] = first
    return csr_ref.from_coo(rows, cols, vals, (k, k))


_PROBLEMS = {}


def problem(tag):
    """`small`: the 60 x 40 matrix of lls_precon.npz (one workgroup per vector).  `odd`: a seeded sparse 1537 x 1025 matrix
    with a strong identity block like that fixture's generator (odd lengths, several 256-row tiles, several partial sums
    per dot).  Consistent right-hand sides (CRAIG needs one)."""
    if tag not in _PROBLEMS:
        if tag == "small":
            d = np.load(os.path.join(GOLDEN, "lls_precon.npz"), allow_pickle=False)
            A, b = golden_csr(d, "A_"), d["b_cons"]
        else:
            m, n, per_row = 1537, 1025, 5
            rng = np.random.default_rng(7)
            rows = np.concatenate([np.repeat(np.arange(m), per_row), np.arange(n)])
            cols = np.concatenate([rng.integers(0, n, m * per_row), np.arange(n)])
            vals = np.concatenate([0.2 * rng.standard_normal(m * per_row), np.ones(n)])
            A = csr_ref.from_coo(rows, cols, vals, (m, n))
            b = A.matvec(np.ones(n))
        _PROBLEMS[tag] = (A, b)
    return _PROBLEMS[tag]


def lbfgs_pairs(k, seed, npairs=3):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((npairs, k))
    Y = S * (1.0 + rng.random((npairs, k))) + 0.01 * rng.standard_normal((npairs, k))
    assert all(float(s @ y) > 0 for s, y in zip(S, Y))
    return S, Y


def make_precon(kind, k, seed):
    """The preconditioner of `kind` for vectors of k entries, and what has to be freed with it."""
    import pykrylov_amd
    from pykrylov_amd import tools
    if kind == "lbfgs":
        H = pykrylov_amd.InverseLBFGSOperator(k, 3)
        for s, y in zip(*lbfgs_pairs(k, seed)):
            assert H.store(s, y)
        return H, [H]
    T = op_from(tridiag(k, seed), symmetric=True)
    if kind == "csr":
        return T, [T]
    P = tools.ic0(T) if kind == "ic0" else tools.block_jacobi(T, 4)
    return P, [P, T]


def precons(case, m, n):
    kw, owned = {}, []
    for side, kind, k, seed in (("M", case[0], m, 1), ("N", case[1], n, 2)):
        if kind is not None:
            kw[side], own = make_precon(kind, k, seed)
            owned += own
    return kw, owned


def through_callbacks(kw, calls=None):
    """The same objects behind plain functions: nothing `resolve_precon` recognises, so they are called back on the host."""
    def wrap(side, P):
        def call(v):
            if calls is not None:
                calls[side] = calls.get(side, 0) + 1
            return P * v
        return call
    return {side: wrap(side, P) for side, P in kw.items()}


def record(solver, A, b, kw, **extra):
    """Everything the comparison covers: x, istop, itn, every scalar result attribute, resids, dir_errors_window."""
    op = op_from(A)
    got, s = run_device(solver, op, b, 0.0, 0.0, store_resids=True, **dict(kw, **extra))
    rec = {k: (v if k in ("istop", "itn") else bits(v)) for k, v in got.items()}
    rec["resids"] = bits(s.resids)
    rec["dir_errors_window"] = bits(s.dir_errors_window)
    route = dict(s.precon_route)
    op.free()
    return rec, route, got


def free_all(owned):
    for o in owned:
        o.free()


def both_routes(solver, tag, case, **extra):
    A, b = problem(tag)
    kw, owned = precons(case, *A.shape)
    dev, route, got = record(solver, A, b, kw, **extra)
    host, route_h, _ = record(solver, A, b, through_callbacks(kw), **extra)
    free_all(owned)
    want = {"M": ROUTE.get(case[0], "none"), "N": ROUTE.get(case[1], "none")}
    assert route == want, (route, want)
    assert route_h == {s: ("host" if v != "none" else "none") for s, v in want.items()}
    return dev, host, got


# ------------------------------------------------------------------ 1. route
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_route_is_recorded_and_the_host_entries_are_never_called(case, monkeypatch):
    """`precon_route` names the device route of each side, and the solve never enters the objects' host products (which
    upload, apply and download): they are replaced by functions that raise before the objects are built."""
    import pykrylov_amd
    from pykrylov_amd import CsrOperator, tools
    A, b = problem("small")

    def boom(*a, **k):
        raise AssertionError("the host entry of a device preconditioner was called")
    kw, owned = precons(case, *A.shape)
    for P in kw.values():
        assert np.isfinite(P * np.ones(P.shape[1])).all()     # (they work before ...)
    free_all(owned)
    monkeypatch.setattr(tools.IluPreconditioner, "_apply", boom)
    monkeypatch.setattr(pykrylov_amd.InverseLBFGSOperator, "lbfgs_matvec", boom)
    kw, owned = precons(case, *A.shape)                       # (the operators bind their products when they are built)
    monkeypatch.setattr(CsrOperator, "_times_vector", boom)
    for P in kw.values():
        with pytest.raises(AssertionError):
            P * np.ones(P.shape[1])
    rec, route, got = record("lsqr", A, b, kw)
    assert route == {"M": ROUTE.get(case[0], "none"), "N": ROUTE.get(case[1], "none")}
    assert got["itn"] > 5 and np.isfinite(got["x"]).all()
    free_all(owned)


# ------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("tag", ["small", "odd"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_bits_of_the_callback_route(solver, tag, case):
    # (the 1537 x 1025 solves are cut at 25 passes: every path has been through all its launches many times by then, and
    #  the host twin pays two round trips per pass)
    extra = {} if tag == "small" else {"itnlim": 25}
    dev, host, got = both_routes(solver, tag, case, **extra)
    print(solver, tag, case, "istop", got["istop"], "itn", got["itn"])
    assert got["itn"] > 5
    for k in host:
        assert dev[k] == host[k], k


@pytest.mark.parametrize("solver", SOLVERS)
def test_bits_of_the_oracle(solver, monkeypatch):
    """M and N device matrices: the oracle with the matrices' left-to-right products as M and N and, both sides being
    preconditioned, every inner product in the stream-dot order (as in test_lls_general_preconditioners_through_callbacks)."""
    A, b = problem("small")
    m, n = A.shape
    Tm, Tn = tridiag(m, 1), tridiag(n, 2)
    Pm, Pn = op_from(Tm, symmetric=True), op_from(Tn, symmetric=True)
    op = op_from(A)
    got, s = run_device(solver, op, b, 0.0, 0.0, M=Pm, N=Pn)
    assert s.precon_route == {"M": "device", "N": "device"}
    monkeypatch.setattr(lls_ref, "_sq", lambda a: a * a)

    class Dots(gpu_order.GpuDots):
        def __call__(self, a, bb, site):
            return gpu_order.stream_dot(a, bb)
    ref = run_oracle(solver, A, b, 0.0, 0.0, red=kr.Reductions(Dots(0, [])), M=Tm.matvec, N=Tn.matvec)
    assert (got["istop"], got["itn"]) == (ref["istop"], ref["itn"]) and got["itn"] > 5
    assert bits(got["x"]) == bits(ref["x"])
    for k, v in got.items():
        if k not in ("x", "istop", "itn"):                   # (every scalar, and CRAIG's residual vector r)
            assert bits(v) == bits(ref[k]), k
    for o in (Pm, Pn, op):
        o.free()


# ------------------------------------------------------------------ 3. halt
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("case", [("csr", "ic0"), ("lbfgs", "bj"), ("ic0", "lbfgs")], ids=lambda c: "M=%s,N=%s" % c)
def test_nothing_changes_after_the_loop_has_halted(solver, case):
    """Stopped by the iteration budget in the middle of a batch of enqueued passes: every launch after the gate that ends
    the loop is a no-op, as the callback is not invoked then."""
    dev, host, got = both_routes(solver, "odd", case, itnlim=3)          # (etol = 0.0 in every run of this file)
    assert (got["istop"], got["itn"]) == (7, 3)
    for k in host:
        assert dev[k] == host[k], k


# ------------------------------------------------------------------ 4. beta = 0
# A = diag(a), b = 3 e1 and N e1 = c e1: u = e1, Nv = a1 e1, v = c a1 e1, alpha = sqrt(v1 Nv1), and the first pass forms
# u <- a1 (v1 / alpha) - alpha = 0 EXACTLY for the constants below (found by search in IEEE double arithmetic: they also make
# N(Nv / alpha) differ from N(Nv) / alpha in the last bit, so a re-application of N in that pass would show -- for all three
# kinds: the L-BFGS operator scales by gamma = 1.6, so H e1 is no copy of e1).
BETA0 = {"csr": (1.67, 2.025),       # N = device matrix, N[0, 0] = 2.025
         "ic0": (1.943, 0.726),      # N = IC(0) of T with T[0, 0] = 0.726: N e1 = (e1 / sqrt(T00)) / sqrt(T00)
         "lbfgs": (1.673, 0.625)}    # N = H with scaling, whose pairs vanish in entry 0 and whose newest pair is y = 0.625 s
                                     # with small whole numbers in s (s.y and y.y are exact in any order): H e1 = gamma e1,
                                     # gamma = s.y / y.y = 1.6 rounded


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("kind", ["csr", "ic0", "lbfgs"])
def test_n_is_not_applied_when_beta_is_zero(solver, kind):
    import pykrylov_amd
    from pykrylov_amd import tools
    n = 40
    a1, first = BETA0[kind]
    d = 1.0 + np.arange(n) / 8.0
    d[0] = a1
    A = csr_ref.RefCsr(np.arange(n + 1), np.arange(n), d, (n, n))
    b = np.zeros(n)
    b[0] = 3.0
    owned = []
    if kind == "lbfgs":
        N = pykrylov_amd.InverseLBFGSOperator(n, 3, scaling=True)
        S, Y = lbfgs_pairs(n, 5)
        S[2] = np.random.default_rng(6).integers(1, 4, n)
        Y[2] = first * S[2]
        for s, y in zip(S, Y):
            s[0] = y[0] = 0.0
            assert N.store(s, y)
        e1 = np.zeros(n)
        e1[0] = 1.0
        assert np.array_equal(N * e1, 1.6 * e1)
    else:
        T = op_from(tridiag(n, 2, first=first), symmetric=True)
        owned.append(T)
        N = T if kind == "csr" else tools.ic0(T)
    owned.append(N)
    calls = {}
    dev, route, got = record(solver, A, b, {"N": N}, itnlim=5)
    host, _, got_h = record(solver, A, b, through_callbacks({"N": N}, calls), itnlim=5)
    free_all(owned)
    print(solver, kind, "istop", got["istop"], "itn", got["itn"], "N calls", calls)
    assert route["N"] == ROUTE[kind]
    # the set-up applies N once; a pass with beta = 0 does not: at least the first pass is such a pass
    assert 1 <= calls["N"] <= max(got_h["itn"], 1)
    if solver == "lsqr":                                     # (rnorm = 0 after that pass: 'Ax - b is small enough')
        assert (got["istop"], got["itn"], calls["N"]) == (1, 1, 1)
    for k in host:
        assert dev[k] == host[k], k                          # (bit patterns: NaNs included)


# ------------------------------------------------------------------ 5. lifetime, replacement, errors (C ABI)
def _solve_handle(lib, _lib, h, b, n):
    d_rhs = _lib.DeviceArray.from_numpy(np.ascontiguousarray(b, dtype=np.float64))
    try:
        _lib.check(lib.mk_solver_setup(h, d_rhs.ptr, None))
        res = _lib.MkResult()
        _lib.check(lib.mk_solver_finish(h, ctypes.byref(res)))
        while not res.halted:
            done = ctypes.c_int64()
            _lib.check(lib.mk_solver_iterate(h, 1 << 20, ctypes.byref(done)))
            _lib.check(lib.mk_solver_finish(h, ctypes.byref(res)))
        px = ctypes.c_void_p()
        _lib.check(lib.mk_solver_x(h, ctypes.byref(px)))
        return int(res.itn), _lib.download(px.value, n)
    finally:
        d_rhs.free()


def test_sides_hold_their_objects_and_are_replaced_one_at_a_time():
    from pykrylov_amd import _lib, lls
    A, b = problem("small")
    m, n = A.shape
    op = op_from(A)
    lib = _lib.init()
    M_SIDE, N_SIDE, ERR_ARG, ERR_UNSUPPORTED = 0, 1, -2, -5

    def expect(kw):
        s = lls.LSQRFramework(op)
        s.solve(b, etol=0.0, **kw)
        return s.itn, s.x

    # what the three stages below must give, from twins of the objects the handle will hold
    kw1, own1 = precons(("lbfgs", "ic0"), m, n)
    kw2, own2 = precons(("lbfgs", "lbfgs"), m, n)
    kw3, own3 = precons((None, "lbfgs"), m, n)
    want = [expect(kw1), expect(kw2), expect(kw3)]
    free_all(own1 + own2 + own3)
    assert len({bits(x) for _, x in want}) == 3

    prm = _lib.MkParams()
    prm.struct_size = ctypes.sizeof(_lib.MkParams)
    prm.kind = _lib.MK_LSQR
    prm.itnlim = 3 * n
    prm.atol = prm.btol = 1.0e-9
    prm.conlim = 1.0e8
    prm.etol = 0.0
    prm.window = 5
    h = ctypes.c_void_p()
    _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(prm), ctypes.byref(h)))
    _lib.check(lib.mk_solver_set_transpose(h, op.T.handle))
    (Hm, _), (F, ownF) = make_precon("lbfgs", m, 1), make_precon("ic0", n, 2)
    _lib.check(lib.mk_solver_set_lls_precon_bfgs(h, M_SIDE, Hm.handle))
    _lib.check(lib.mk_solver_set_lls_precon_ilu(h, N_SIDE, F.handle))
    free_all([Hm] + ownF)                                     # destroyed while the sides hold them: deferred
    got = _solve_handle(lib, _lib, h, b, n)
    assert got[0] == want[0][0] and bits(got[1]) == bits(want[0][1])

    Hn, _ = make_precon("lbfgs", n, 2)
    _lib.check(lib.mk_solver_set_lls_precon_bfgs(h, N_SIDE, Hn.handle))      # releases the factor; M is untouched
    got = _solve_handle(lib, _lib, h, b, n)
    assert got[0] == want[1][0] and bits(got[1]) == bits(want[1][1])
    _lib.check(lib.mk_solver_set_lls_precon_bfgs(h, M_SIDE, None))           # NULL removes M; N is untouched
    got = _solve_handle(lib, _lib, h, b, n)
    assert got[0] == want[2][0] and bits(got[1]) == bits(want[2][1])

    # error codes
    Tn = op_from(tridiag(n, 2), symmetric=True)
    Fm, ownFm = make_precon("ic0", m, 1)
    assert lib.mk_solver_set_lls_precon_csr(h, N_SIDE, op.handle) == ERR_ARG          # 60 x 40: not square
    assert lib.mk_solver_set_lls_precon_csr(h, M_SIDE, Tn.handle) == ERR_ARG          # 40 x 40 on the m = 60 side
    assert lib.mk_solver_set_lls_precon_ilu(h, N_SIDE, Fm.handle) == ERR_ARG
    assert lib.mk_solver_set_lls_precon_bfgs(h, M_SIDE, Hn.handle) == ERR_ARG
    assert lib.mk_solver_set_lls_precon_csr(h, 2, Tn.handle) == ERR_ARG               # no such side
    got = _solve_handle(lib, _lib, h, b, n)                                          # a refused setter changes nothing
    assert got[0] == want[2][0] and bits(got[1]) == bits(want[2][1])
    _lib.check(lib.mk_solver_set_lls_precon_csr(h, N_SIDE, Tn.handle))               # replaces the L-BFGS operator
    _lib.check(lib.mk_solver_set_lls_precon_callback(h, ctypes.cast(None, _lib.PRECON_FN), None,
                                                     ctypes.cast(None, _lib.PRECON_FN), None))   # (no callback to remove)
    Hn.free()
    # the handle goes while both sides hold something whose owner is gone already (the references are dropped by the
    # solver's destructor: test_destroying_the_solver_releases_what_its_sides_hold looks at the memory)
    (Hd, _), (Fd, ownFd) = make_precon("lbfgs", m, 3), make_precon("ic0", n, 4)
    _lib.check(lib.mk_solver_set_lls_precon_bfgs(h, M_SIDE, Hd.handle))
    _lib.check(lib.mk_solver_set_lls_precon_ilu(h, N_SIDE, Fd.handle))          # releases the matrix Tn
    free_all([Hd] + ownFd)
    _lib.check(lib.mk_solver_destroy(h))

    sq = op_from(tridiag(n, 2), symmetric=True)
    prm.kind = _lib.MK_CG
    prm.matvec_max = 10
    hc = ctypes.c_void_p()
    _lib.check(lib.mk_solver_create(sq.handle, ctypes.byref(prm), ctypes.byref(hc)))
    Hs, _ = make_precon("lbfgs", n, 2)
    Fs, ownFs = make_precon("ic0", n, 2)
    assert lib.mk_solver_set_lls_precon_csr(hc, N_SIDE, Tn.handle) == ERR_UNSUPPORTED
    assert lib.mk_solver_set_lls_precon_ilu(hc, N_SIDE, Fs.handle) == ERR_UNSUPPORTED
    assert lib.mk_solver_set_lls_precon_bfgs(hc, M_SIDE, Hs.handle) == ERR_UNSUPPORTED
    _lib.check(lib.mk_solver_destroy(hc))

    # every reference is back: the objects go at once, and fresh ones work
    free_all([Hs, Tn, sq] + ownFs + ownFm)
    v = np.random.default_rng(3).standard_normal(n)
    for kind in ("ic0", "lbfgs"):
        P, own = make_precon(kind, n, 2)
        assert np.isfinite(P * v).all()
        free_all(own)
    op.free()


def test_destroying_the_solver_releases_what_its_sides_hold():
    """M an L-BFGS operator and N a device matrix of 2^20 rows (48 MiB of rings, 40 MiB of matrix), both freed by their owners
    while the sides hold them -- which is deferred, the memory stays -- and the handle destroyed with both still attached:
    the destructor drops the two references, so the objects go with it and their memory is back."""
    import gc
    import pykrylov_amd
    from pykrylov_amd import CsrOperator, _lib
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value

    n = 1 << 20
    lib = _lib.init()
    op = CsrOperator(np.arange(n + 1), np.arange(n), np.ones(n), (n, n))
    prm = _lib.MkParams()
    prm.struct_size = ctypes.sizeof(_lib.MkParams)
    prm.kind = _lib.MK_LSQR
    prm.itnlim = 1
    prm.window = 5
    h = ctypes.c_void_p()
    _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(prm), ctypes.byref(h)))
    gc.collect()
    before = free_bytes()

    rng = np.random.default_rng(8)
    H = pykrylov_amd.InverseLBFGSOperator(n, 3)
    for _ in range(3):
        s = rng.standard_normal(n)
        assert H.store(s, s * (1.0 + rng.random(n)))
    cols = np.stack([np.arange(n) - 1, np.arange(n), np.arange(n) + 1], axis=1).reshape(-1)
    vals = np.tile([-0.5, 2.5, -0.5], n)
    keep = (cols >= 0) & (cols < n)
    indptr = np.concatenate([[0], np.cumsum(keep.reshape(n, 3).sum(axis=1))])
    T = CsrOperator(indptr, cols[keep], vals[keep], (n, n), symmetric=True)
    _lib.check(lib.mk_solver_set_lls_precon_bfgs(h, 0, H.handle))
    _lib.check(lib.mk_solver_set_lls_precon_csr(h, 1, T.handle))
    H.free()
    T.free()
    held = before - free_bytes()
    print("held by the sides: %.1f MiB" % (held / 2.0**20))
    assert held > 64 << 20                                   # (both are still there: the solver could go on applying them)
    _lib.check(lib.mk_solver_destroy(h))
    left = before - free_bytes()
    print("left after the solver went: %.1f MiB" % (left / 2.0**20))
    assert left < 8 << 20                                    # (the solver's own vectors went too: `left` may be negative)
    op.free()


# ------------------------------------------------------------------ 6. one handle, every kind in turn
KIND_ORDER = ("diag", "csr", "ilu", "lbfgs", "cheb", "callback", "none")


def test_a_replaced_kind_leaves_nothing_behind():
    """One BiCGSTAB handle (A = the 33-row tridiagonal matrix) and one LSQR handle (its first 17 columns; M and N both of the
    kind) take every kind of preconditioner in turn and solve again after each replacement: x, both history channels and
    itn are, byte for byte, those of a fresh handle that only ever held that kind.  Whatever a slot keeps across a
    replacement -- its ones, the pointer the kernels multiply by, the pinned buffers, d_ptmp -- must not show.  The
    lengths are odd, so the stream kernels' tail lane runs."""
    from pykrylov_amd import _lib, tools
    from pykrylov_amd.generic import HostPrecon
    lib = _lib.init()
    m, n = 33, 17
    T = tridiag(m, 11)
    rows = np.repeat(np.arange(m), np.diff(T.indptr))
    keep = T.indices < n
    A_sq, A_ls = op_from(T), op_from(csr_ref.from_coo(rows[keep], T.indices[keep], T.data[keep], (m, n)))
    d_rhs = _lib.DeviceArray.from_numpy(T.matvec(np.ones(m)))
    owned = [A_sq, A_ls, d_rhs]

    def kit(k, seed, call_first):
        """One preconditioner of every kind for vectors of k entries, as the C setters take them."""
        P = op_from(tridiag(k, seed), symmetric=True)
        d = _lib.DeviceArray.from_numpy(1.0 + np.random.default_rng(seed).random(k))
        F, H, C = tools.ic0(P), make_precon("lbfgs", k, seed)[0], tools.chebyshev(P, degree=3)
        host = HostPrecon(P, call_first)                     # (the callback: the same matrix, multiplied on the host)
        owned.extend([C, F, H, d, P])
        return {"diag": d.ptr, "csr": P.handle, "ilu": F._live(), "lbfgs": H._live(), "cheb": C._live(),
                "callback": host.thunk(k), "none": None}
    sq, pm, pn = kit(m, 1, False), kit(m, 2, True), kit(n, 3, True)

    def attach_square(h, kind):
        if kind == "callback":
            return lib.mk_solver_set_precon_callback(h, sq[kind], None)
        name = {"none": "csr"}.get(kind, kind)
        return getattr(lib, "mk_solver_set_precon_" + name)(h, sq[kind])

    def attach_sides(h, kind):
        if kind == "diag":
            return lib.mk_solver_set_lls_precon(h, pm[kind], pn[kind])
        if kind == "callback":
            return lib.mk_solver_set_lls_precon_callback(h, pm[kind], None, pn[kind], None)
        setter = getattr(lib, "mk_solver_set_lls_precon_" + {"none": "csr", "lbfgs": "bfgs"}.get(kind, kind))
        return setter(h, 0, pm[kind]) or setter(h, 1, pn[kind])

    def create(op, transpose, **params):
        prm = _lib.MkParams()
        prm.struct_size = ctypes.sizeof(_lib.MkParams)
        for k, v in params.items():
            setattr(prm, k, v)
        h = ctypes.c_void_p()
        _lib.check(lib.mk_solver_create(op.handle, ctypes.byref(prm), ctypes.byref(h)))
        if transpose:
            _lib.check(lib.mk_solver_set_transpose(h, op.T.handle))
        return h

    def solve(h, nx):
        _lib.check(lib.mk_solver_setup(h, d_rhs.ptr, None))
        res = _lib.MkResult()
        _lib.check(lib.mk_solver_finish(h, ctypes.byref(res)))
        while not res.halted:
            _lib.check(lib.mk_solver_iterate(h, 1 << 20, None))
            _lib.check(lib.mk_solver_finish(h, ctypes.byref(res)))
        px = ctypes.c_void_p()
        _lib.check(lib.mk_solver_x(h, ctypes.byref(px)))
        hist = np.zeros((2, int(res.hist_len)))
        _lib.check(lib.mk_solver_history(h, hist[0].ctypes.data, hist.shape[1]))
        _lib.check(lib.mk_solver_history2(h, hist[1].ctypes.data, hist.shape[1]))
        return int(res.itn), int(res.nMatvec), bits(_lib.download(px.value, nx)), bits(hist)

    families = (("bicgstab", attach_square, m, lambda: create(A_sq, False, kind=_lib.MK_BICGSTAB, abstol=1.0e-12,
                                                                    reltol=1.0e-12, matvec_max=4 * m)),
                ("lsqr", attach_sides, n, lambda: create(A_ls, True, kind=_lib.MK_LSQR, itnlim=3 * n, atol=1.0e-12,
                                                         btol=1.0e-12, conlim=1.0e8, etol=0.0, window=5)))
    for family, attach, nx, new_handle in families:
        want = {}
        for kind in KIND_ORDER:                              # fresh handles: each only ever holds its kind
            h = new_handle()
            _lib.check(attach(h, kind))
            want[kind] = solve(h, nx)
            _lib.check(lib.mk_solver_destroy(h))
        # (the kinds do differ -- but for the callback, which applies the matrix of "csr")
        assert len(set(want.values())) >= 6, family
        h = new_handle()
        for kind in KIND_ORDER:                              # one handle: every kind replaces the one before
            _lib.check(attach(h, kind))
            got = solve(h, nx)
            print(family, kind, "itn", got[0], "nMatvec", got[1])
            assert got[0] > 0 and got == want[kind], (family, kind)
        _lib.check(lib.mk_solver_destroy(h))
    free_all(owned)
