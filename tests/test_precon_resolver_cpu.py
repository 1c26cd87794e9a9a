"""`generic.resolve_precon` and `HostPrecon.thunk`: the one resolver and the one host callback behind ``precon`` of the
square solvers and M / N of the least-squares solvers, driven over one preconditioner per kind without a device."""
import ctypes

import numpy as np
import pytest

from tests.test_host import header_functions

N = 10
NAMES = ("precon", "M", "N")
KINDS = ("none", "diag", "host", "device", "ilu", "lbfgs", "cheb", "fsai", "amg")
SINGLE_GPU = ("host", "ilu", "lbfgs", "cheb", "fsai", "amg")
OBJECT_CLASSES = ("IluPreconditioner", "ChebyshevPreconditioner", "FsaiPreconditioner", "AmgPreconditioner")

# the functions include/mikrylov.h declares, as of the commit before the device objects got their common base
ABI = """
    mk_amg_apply mk_amg_coarse mk_amg_create mk_amg_destroy mk_amg_download mk_amg_info mk_amg_level
    mk_arena_reserve mk_axpby mk_axpy mk_build_info mk_calib_stream mk_cheb_apply mk_cheb_coefficients
    mk_cheb_create mk_cheb_destroy mk_cheb_info mk_comm_allreduce_host mk_comm_destroy mk_comm_info mk_comm_init
    mk_comm_init_host mk_comm_time_allreduce mk_comm_time_exchange mk_comm_transport mk_comm_unique_id
    mk_csr_col_range mk_csr_colblocks mk_csr_comm_last_us mk_csr_compose mk_csr_create mk_csr_create_block
    mk_csr_create_callback mk_csr_create_product mk_csr_create_reduced mk_csr_create_sum mk_csr_destroy
    mk_csr_download mk_csr_download_rows mk_csr_format_info mk_csr_from_coo mk_csr_lanczos mk_csr_launch_info
    mk_csr_localize mk_csr_march_info mk_csr_overlap_info mk_csr_pencil_info mk_csr_poisson2d mk_csr_poisson3d
    mk_csr_poisson3d_varcoef mk_csr_set_colblocks mk_csr_set_exchange mk_csr_set_format mk_csr_set_row_block
    mk_csr_set_tile_order mk_csr_shape mk_csr_stencil27 mk_csr_tile_order mk_csr_transpose mk_device_info mk_dot
    mk_exchange mk_free mk_fsai_apply mk_fsai_create mk_fsai_destroy mk_fsai_download mk_fsai_factors mk_fsai_info
    mk_ic0_create mk_ilu0_create mk_ilu_apply mk_ilu_destroy mk_ilu_download mk_ilu_info mk_init mk_last_error
    mk_lbfgs_apply mk_lbfgs_create mk_lbfgs_destroy mk_lbfgs_download mk_lbfgs_forward_combine mk_lbfgs_forward_dots
    mk_lbfgs_gram mk_lbfgs_info mk_lbfgs_restart mk_lbfgs_store mk_malloc mk_memcpy_d2d mk_memcpy_d2h mk_memcpy_h2d
    mk_memset mk_nrm2 mk_scal mk_shutdown mk_solver_create mk_solver_destroy mk_solver_finish mk_solver_fused
    mk_solver_history mk_solver_history2 mk_solver_iterate mk_solver_set_idr mk_solver_set_lls_precon
    mk_solver_set_lls_precon_amg mk_solver_set_lls_precon_bfgs mk_solver_set_lls_precon_callback
    mk_solver_set_lls_precon_cheb mk_solver_set_lls_precon_csr mk_solver_set_lls_precon_fsai
    mk_solver_set_lls_precon_ilu mk_solver_set_pcg mk_solver_set_precon_amg mk_solver_set_precon_callback
    mk_solver_set_precon_cheb mk_solver_set_precon_csr mk_solver_set_precon_diag mk_solver_set_precon_fsai
    mk_solver_set_precon_ilu mk_solver_set_precon_lbfgs mk_solver_set_transpose mk_solver_setup mk_solver_solve
    mk_solver_time_product mk_solver_time_spmv mk_solver_timing mk_solver_unapplied mk_solver_vector mk_solver_x
    mk_spmv mk_sync mk_version
""".split()


def _fake(cls, n):
    """An operator object of class `cls` with shape (n, n) that never saw the device."""
    op = object.__new__(cls)
    op.__dict__.update(_shape=(n, n), _symmetric=True, _nargout=n, _nargin=n)
    return op


class Diag(object):
    def __init__(self, n):
        self.diag = np.arange(1.0, n + 1)


class Host(object):
    """Something `resolve_precon` knows nothing about: it is applied on the host.  Returns n entries."""

    def __init__(self, n):
        self.n = n

    def __mul__(self, v):
        return np.resize(v, self.n)

    __call__ = __mul__


class Composite(object):
    """Like `tools.block_jacobi`: not a matrix itself, but it has a device view."""

    def __init__(self, n):
        from pykrylov_amd.linop import CsrOperator
        self.dev = _fake(CsrOperator, n)

    def _device_view(self):
        return self.dev


def make(kind, n=N):
    import pykrylov_amd
    from pykrylov_amd import tools
    return {"none": lambda: None, "diag": lambda: Diag(n), "host": lambda: Host(n), "device": lambda: Composite(n),
            "ilu": lambda: _fake(tools.IluPreconditioner, n), "lbfgs": lambda: pykrylov_amd.InverseLBFGSOperator(n),
            "cheb": lambda: _fake(tools.ChebyshevPreconditioner, n), "fsai": lambda: _fake(tools.FsaiPreconditioner, n),
            "amg": lambda: _fake(tools.AmgPreconditioner, n)}[kind]()


class Op(object):
    shape = (N, N)

    def __mul__(self, x):
        return x


class Part(Op):
    shape = (2 * N, 2 * N)
    local_size = N


def call_thunk(hp, v):
    """Invoke the C callback of `hp` on `v` as the library does; returns (its return code, the output buffer)."""
    vin = np.ascontiguousarray(v, dtype=np.float64)
    out = np.full(len(vin), np.nan)
    cb = hp.thunk(len(vin))
    return cb(None, vin.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)), out


@pytest.mark.parametrize("kind", KINDS)
def test_the_three_routes_read_the_same_word(kind):
    from pykrylov_amd.generic import DevicePrecon, HostPrecon, KrylovMethod, resolve_precon
    P = make(kind)
    got = [resolve_precon(P, N, name, "Solver") for name in NAMES]
    assert [route for route, _ in got] == [kind] * 3
    # what `_device_precon` hands to DeviceRun: the payload of the square route
    payload = KrylovMethod(Op())._device_precon(P)
    if kind == "none":
        assert payload is None
    elif kind == "diag":
        assert payload.dtype == np.float64 and np.array_equal(payload, P.diag)
    elif kind == "device":
        assert isinstance(payload, DevicePrecon) and payload.precon is P and payload.dev is P.dev
    elif kind == "host":
        assert isinstance(payload, HostPrecon) and payload.precon is P
    else:
        assert payload is P
    for _, side in got:
        assert type(side) is type(payload)


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "none"])
def test_a_wrong_shape_is_a_value_error_naming_shape(kind):
    from pykrylov_amd.generic import KrylovMethod, resolve_precon
    P = make(kind, N - 1)
    for name in NAMES:
        if kind == "host":
            # a host callable has no shape to look at before it is called: its callback refuses what it returns
            hp = resolve_precon(P, N, name, "Solver")[1]
            rc, _ = call_thunk(hp, np.ones(N))
            assert rc == 1 and isinstance(hp.error, ValueError) and "shape" in str(hp.error) and hp.calls == 0
            continue
        with pytest.raises(ValueError, match="shape"):
            resolve_precon(P, N, name, "Solver")
    if kind != "host":
        with pytest.raises(ValueError, match="shape"):
            KrylovMethod(Op())._device_precon(P)


def test_something_that_cannot_be_applied_is_a_type_error():
    from pykrylov_amd.generic import KrylovMethod, resolve_precon
    for name in NAMES:
        with pytest.raises(TypeError, match=name):
            resolve_precon(object(), N, name, "Solver")
    with pytest.raises(TypeError):
        KrylovMethod(Op())._device_precon(object())


@pytest.mark.parametrize("kind", KINDS)
def test_a_partitioned_square_operator_refuses_the_single_gpu_kinds(kind):
    """The size rule is `local_size or shape[0]`: everything here has the local size N of an operator of 2 N rows."""
    from pykrylov_amd.generic import KrylovMethod, resolve_precon
    P = make(kind)
    s = KrylovMethod(Part())
    if kind in SINGLE_GPU:
        word = "row-partitioned" if kind == "host" else "single-GPU"
        with pytest.raises(NotImplementedError, match=word):
            s._device_precon(P)
        with pytest.raises(NotImplementedError, match="row-partitioned"):
            resolve_precon(P, N, "precon", "Solver", partitioned=True)
    else:
        assert resolve_precon(P, N, "precon", "Solver", partitioned=True)[0] == kind
        s._device_precon(P)
        if kind != "none":
            with pytest.raises(ValueError, match="shape"):   # (not the global size)
                s._device_precon(make(kind, 2 * N))


def test_call_convention_of_the_host_thunk():
    """An object with both `__call__` and `__mul__`: a square solver evaluates ``precon * r``, M and N are called."""
    from pykrylov_amd.generic import resolve_precon

    class Both(object):
        def __call__(self, v):
            return 2.0 * v

        def __mul__(self, v):
            return 3.0 * v

    class OnlyCall(object):
        def __call__(self, v):
            return 5.0 * v

    class OnlyMul(object):
        def __mul__(self, v):
            return 7.0 * v

    v = np.arange(1.0, N + 1)
    for name in NAMES:
        for P, factor in ((Both(), 3.0 if name == "precon" else 2.0), (OnlyCall(), 5.0), (OnlyMul(), 7.0)):
            route, hp = resolve_precon(P, N, name, "Solver")
            assert route == "host" and hp.calls == 0
            rc, out = call_thunk(hp, v)
            assert rc == 0 and np.array_equal(out, factor * v) and hp.calls == 1 and hp.error is None
            assert np.array_equal(hp.apply(v), factor * v)


def test_the_first_error_of_a_host_thunk_is_kept():
    from pykrylov_amd.generic import resolve_precon
    raised = []

    def P(v):
        raised.append(RuntimeError("failure %d" % len(raised)))
        raise raised[-1]
    for name in NAMES:
        del raised[:]
        hp = resolve_precon(P, N, name, "Solver")[1]
        assert call_thunk(hp, np.ones(N))[0] == 1 and call_thunk(hp, np.ones(N))[0] == 1
        assert len(raised) == 2 and hp.error is raised[0] and hp.calls == 0


@pytest.mark.parametrize("name", OBJECT_CLASSES)
def test_a_freed_device_object_says_so_without_touching_the_device(name, monkeypatch):
    from pykrylov_amd import _lib, tools

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "init", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    P = _fake(getattr(tools, name), N)
    P._handle = None
    for use in (lambda: P.handle, P._live, lambda: P * np.ones(N), lambda: P.apply_device(None, None), lambda: P.info):
        with pytest.raises(ValueError, match="freed"):
            use()
    P.free()
    P.free()
    assert P._handle is None


def test_the_route_table_names_the_setters_of_every_route():
    """`generic.PRECON_SETTERS` has exactly the route words `resolve_precon` can return (`make` builds one preconditioner
    per word) except 'none', and every setter name it forms is declared in include/mikrylov.h and in `_lib.PROTOTYPES`."""
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import PRECON_SETTERS, precon_setter, resolve_precon
    routes = {resolve_precon(make(kind), N, "precon", "Solver")[0] for kind in KINDS}
    assert routes == set(KINDS) and set(PRECON_SETTERS) == routes - {"none"}
    declared = header_functions()
    formed = [precon_setter(route, lls) for route in PRECON_SETTERS for lls in (False, True)]
    for fn in formed:
        assert fn in declared and fn in _lib.PROTOTYPES, fn
    assert len(set(formed)) == len(formed)
    # ... and they are all the preconditioner setters there are
    assert sorted(formed) == sorted(fn for fn in declared if "_precon" in fn)
    assert precon_setter("lbfgs") == "mk_solver_set_precon_lbfgs" and precon_setter("lbfgs", True) == "mk_solver_set_lls_precon_bfgs"
    assert precon_setter("diag", True) == "mk_solver_set_lls_precon" and precon_setter("device") == "mk_solver_set_precon_csr"


def test_the_c_abi_declares_the_functions_it_declared_before():
    assert header_functions() == sorted(ABI)
