"""`generic.resolve_precon` and `HostPrecon.thunk`: the one resolver and the one host callback behind ``precon`` of the
square solvers and M / N of the least-squares solvers, driven over one preconditioner per kind without a device."""
import ctypes

import numpy as np
import pytest

N = 10
NAMES = ("precon", "M", "N")
KINDS = ("none", "diag", "host", "device", "ilu", "lbfgs", "cheb")
SINGLE_GPU = ("host", "ilu", "lbfgs", "cheb")


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
            "cheb": lambda: _fake(tools.ChebyshevPreconditioner, n)}[kind]()


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
