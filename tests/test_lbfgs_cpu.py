"""CPU-only checks of the L-BFGS operators: the NumPy restatement (tests/_lbfgs_ref.py) reproduces the fixture written by
the reference (tests/golden/lbfgs.npz) bit for bit, the C entry points and the ctypes table agree, and every argument error
is raised before a device is touched (these run on a machine without a GPU)."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from tests import _lbfgs_ref as lr

ENTRY_POINTS = ("mk_lbfgs_create", "mk_lbfgs_destroy", "mk_lbfgs_store", "mk_lbfgs_restart", "mk_lbfgs_apply",
                "mk_lbfgs_forward_dots", "mk_lbfgs_forward_combine", "mk_lbfgs_gram", "mk_lbfgs_info", "mk_lbfgs_download",
                "mk_solver_set_precon_lbfgs")


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def fixture_cases(g):
    for n in (10, 1001):
        for npairs in (1, 5):
            for scaling in (0, 1):
                for name in lr.SCENARIOS:
                    yield n, npairs, scaling, name, "%d_%d_%d_%s_" % (n, npairs, scaling, name)


def test_fixture_covers_the_cases_of_the_scenarios():
    g = np.load(os.path.join(GOLDEN, "lbfgs.npz"))
    cases = list(fixture_cases(g))
    assert len(cases) == 48
    for n, npairs, scaling, name, key in cases:
        ops = [tuple(o) for o in g[key + "ops"]]
        assert ops == lr.scenario_ops(name, npairs), key
        assert (key + "Bv" in g.files) == (n == 10)
    stored = {(npairs, name): sum(1 for c, _ in lr.scenario_ops(name, npairs) if c == lr.STORE)
              for npairs in (1, 5) for name in lr.SCENARIOS}
    assert stored[(5, "none")] == 0 and 0 < stored[(5, "few")] < 5 and stored[(5, "full")] == 5 and stored[(5, "wrap")] == 7
    assert {c for c, _ in lr.scenario_ops("reject", 5)} == {lr.STORE, lr.STORE_NEG, lr.STORE_ZERO}
    assert [c for c, _ in lr.scenario_ops("restart", 5)][-3:] == [lr.RESTART, lr.STORE, lr.STORE]


def test_restatement_reproduces_the_reference_bit_for_bit():
    g = np.load(os.path.join(GOLDEN, "lbfgs.npz"))
    for n, npairs, scaling, name, key in fixture_cases(g):
        S, Y, v = g["pool_s_%d" % n], g["pool_y_%d" % n], g["v_%d" % n]
        ops = [tuple(o) for o in g[key + "ops"]]
        H = lr.RefLBFGS(n, npairs, bool(scaling), dot=np.dot)
        C = lr.RefLBFGS(n, npairs, bool(scaling), dot=np.dot)
        lr.replay(H, ops, S, Y)
        lr.replay(C, ops, S, Y)
        assert same(H.inverse(v), g[key + "Hv"]), key
        assert same(C.compact(v), g[key + "Cv"]), key
        assert H.insert == g[key + "insert"][0] and C.insert == g[key + "insert"][1], key
        assert same([np.nan if t is None else t for t in H.ys], g[key + "ys"]), key
        assert same(H.gamma, g[key + "gammaH"]) and same(C.gamma, g[key + "gammaC"]), key
        if n == 10:
            # the outer-product form never reads gamma: it is the compact product with gamma = 1, to rounding
            B = lr.RefLBFGS(n, npairs, bool(scaling), dot=np.dot)
            lr.replay(B, ops, S, Y)
            want = g[key + "Bv"]
            assert np.linalg.norm(B.compact(v, use_gamma=False) - want) <= 1e-12 * np.linalg.norm(want), key


def header_functions():
    text = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", text))


def test_entry_points_are_declared_and_bound():
    from pykrylov_amd import _lib
    lib = _lib.load()                                            # loading needs no GPU
    names = {f for f in header_functions() if "lbfgs" in f}
    assert names == set(ENTRY_POINTS)
    assert {f for f in _lib.PROTOTYPES if "lbfgs" in f} == names
    for f in names:
        assert hasattr(lib, f), f
    text = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    for f in names:
        assert re.search(r"MK_API\s+int\s+%s\s*\(" % f, text), f


def test_argument_errors_need_no_device():
    import pykrylov_amd
    from pykrylov_amd import lbfgs
    for cls in (pykrylov_amd.InverseLBFGSOperator, pykrylov_amd.LBFGSOperator, pykrylov_amd.CompactLBFGSOperator):
        for n in (0, -3, 2.5):
            with pytest.raises(ValueError):
                cls(n)
        for npairs in (0, -1, lbfgs.MAX_PAIRS + 1, 1.5):
            with pytest.raises(ValueError):
                cls(10, npairs)
        op = cls(10, npairs=lbfgs.MAX_PAIRS, scaling=True)
        assert op.shape == (10, 10) and op.symmetric and op.T is op
        assert op.npairs == lbfgs.MAX_PAIRS and op.insert == 0 and op.ys == [None] * lbfgs.MAX_PAIRS
        assert op.gamma == 1.0 and op.accept_threshold == 1.0e-20 and op.scaling is True
        op.accept_threshold = 1e-8
        assert op.accept_threshold == 1e-8
        with pytest.raises(TypeError):
            op * (np.ones(10) + 1j)
        with pytest.raises(ValueError):
            op * np.ones(9)
        with pytest.raises(ValueError):
            op * np.ones((10, 1))
        with pytest.raises(ValueError):
            op.store(np.ones(9), np.ones(10))
        with pytest.raises(ValueError):
            op.store(np.ones(10), np.ones(11))
        with pytest.raises(TypeError):
            op.store(np.ones(10), np.ones(10) * 1j)
        assert op._handle is None                                # nothing above created the device object
        op.free()
        with pytest.raises(ValueError, match="freed"):
            op * np.ones(10)
        with pytest.raises(ValueError, match="freed"):
            op.store(np.ones(10), np.ones(10))
        with pytest.raises(ValueError, match="freed"):
            op.handle
    assert not hasattr(pykrylov_amd, "StructuredLBFGSOperator")


def test_dispatch_checks_need_no_device():
    """KrylovMethod._device_precon: the inverse operator goes to the device loop as it is; shape and partitioning are
    checked there; the forward operators are not preconditioners and take the host-callback route."""
    import pykrylov_amd
    from pykrylov_amd.generic import HostPrecon, KrylovMethod

    class Op(object):
        shape = (10, 10)

        def __mul__(self, x):
            return x

    class Part(Op):
        local_size = 5

    H = pykrylov_amd.InverseLBFGSOperator(10)
    assert KrylovMethod(Op())._device_precon(H) is H
    with pytest.raises(ValueError, match="shape"):
        KrylovMethod(Op())._device_precon(pykrylov_amd.InverseLBFGSOperator(9))
    with pytest.raises(NotImplementedError, match="single-GPU"):
        KrylovMethod(Part())._device_precon(H)
    for cls in (pykrylov_amd.LBFGSOperator, pykrylov_amd.CompactLBFGSOperator):
        assert isinstance(KrylovMethod(Op())._device_precon(cls(10)), HostPrecon)
    assert H._handle is None
