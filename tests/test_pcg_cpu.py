"""PCG without a device: the NumPy restatement of the device loop (tests/_pcg_ref.py) gives the bits of the oracle's CG when
there is no preconditioner, agrees with the textbook helper of the AMG tests, needs the flexible beta for a preconditioner
that changes at every call, halts and breaks down where the contract says; the constants and the new entry point are in the
header, the ctypes table and the library; the host-side checks of `pykrylov_amd.PCG` run before any device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import csr_ref, krylov_ref
from tests import _amg_ref
from tests import _pcg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MAT = {}


def poisson2d(m):
    if m not in _MAT:
        _MAT[m] = csr_ref.poisson2d(m)
    return _MAT[m]


def rhs_of(A):
    return A.matvec(1.0 + np.random.default_rng(4).random(A.shape[0]))


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class Diagonal(object):
    def __init__(self, d):
        self.d = d

    def __mul__(self, v):
        return self.d * v


class Changing(object):
    """Call k = 1, 2, ... multiplies by the diagonal 0.25 (1 + 3 cell_field(arange(n), k)): positive, another one every time."""

    def __init__(self, n):
        self.n, self.k = n, 0

    def __mul__(self, v):
        self.k += 1
        return (0.25 * (1.0 + 3.0 * csr_ref.cell_field(np.arange(self.n), self.k))) * v


@pytest.mark.parametrize("m,products", [(12, 44), (31, 106)])
def test_without_a_preconditioner_it_is_the_oracles_cg_bit_for_bit(m, products):
    A = poisson2d(m)
    b = rhs_of(A)
    got = ref.pcg(A, b, abstol=0.0, reltol=1e-10)
    want = krylov_ref.cg(A, b, abstol=0.0, reltol=1e-10)
    assert got.nMatvec == want["nMatvec"] == products and got.converged and want["converged"]
    assert same(got.x, want["x"]) and same(got.history, want["residHistory"])
    assert got.nIter == got.nMatvec and got.precon_calls == 0 and got.breakdown == 0 and got.definite
    # ... and with the flexible beta the same solution to rounding, in about as many products
    flex = ref.pcg(A, b, abstol=0.0, reltol=1e-10, flexible=True)
    assert flex.converged and abs(flex.nMatvec - products) <= 1


def test_agrees_with_the_textbook_helper():
    """The helper forms its norms with other calls (np.linalg.norm of r and of b): counts within one."""
    A = poisson2d(100)
    b = A.matvec(np.ones(A.shape[0]))
    _, it0 = _amg_ref.pcg(A, b, None, rtol=1e-10)
    M = _amg_ref.build(A)
    _, it1 = _amg_ref.pcg(A, b, M, rtol=1e-10)
    assert (it0, it1) == (211, 16)
    plain = ref.pcg(A, b, abstol=0.0, reltol=1e-10)
    amg = ref.pcg(A, b, abstol=0.0, reltol=1e-10, precon=M)
    flex = ref.pcg(A, b, abstol=0.0, reltol=1e-10, precon=M, flexible=True)
    print("poisson2d(100): %d plain, %d with AMG, %d flexible with AMG" % (plain.nIter, amg.nIter, flex.nIter))
    assert plain.converged and amg.converged and flex.converged
    assert abs(plain.nIter - 211) <= 1 and abs(amg.nIter - 16) <= 1
    assert flex.nIter == 16
    assert amg.precon_calls == amg.nIter and flex.precon_calls == flex.nIter
    assert np.linalg.norm(b - A.matvec(amg.x)) <= 1.01e-10 * np.linalg.norm(b)


def test_a_fixed_diagonal_flexible_and_standard_take_the_same_count():
    A = poisson2d(30)
    n = A.shape[0]
    M = Diagonal(1.0 / (4.0 + (csr_ref.cell_field(np.arange(n), 1) - 0.5)))
    b = rhs_of(A)
    std = ref.pcg(A, b, reltol=1e-10, precon=M)
    flex = ref.pcg(A, b, reltol=1e-10, precon=M, flexible=True)
    print("poisson2d(30), fixed diagonal: %d standard, %d flexible" % (std.nMatvec, flex.nMatvec))
    assert std.converged and flex.converged and std.nMatvec == flex.nMatvec
    assert np.allclose(std.x, flex.x, rtol=0, atol=1e-8)


def test_a_changing_preconditioner_needs_the_flexible_beta():
    A = poisson2d(30)
    n = A.shape[0]
    b = rhs_of(A)
    flex = ref.pcg(A, b, reltol=1e-10, precon=Changing(n), flexible=True)
    assert flex.converged and flex.breakdown == 0
    std = ref.pcg(A, b, reltol=1e-10, precon=Changing(n), matvec_max=2 * flex.nMatvec)
    print("poisson2d(30), a preconditioner that changes: flexible %d products, standard %d (converged %s)"
          % (flex.nMatvec, std.nMatvec, std.converged))
    assert not std.converged and std.nMatvec == 2 * flex.nMatvec
    assert np.linalg.norm(b - A.matvec(flex.x)) <= 1.01 * max(1e-8, 1e-10 * flex.residNorm0)      # (the default abstol)


def test_halts():
    A = poisson2d(12)
    n = A.shape[0]
    b = rhs_of(A)
    M = Diagonal(np.full(n, 0.25))
    z = ref.pcg(A, np.zeros(n), precon=M)
    assert z.nMatvec == 0 and z.nIter == 0 and z.precon_calls == 0 and list(z.history) == [0.0] and z.converged and not z.x.any()
    xs = 1.0 + np.arange(n) / n
    I = csr_ref.from_coo(np.arange(5), np.arange(5), np.full(5, 2.5), (5, 5))
    g = ref.pcg(I, np.arange(1.0, 6.0), guess=np.arange(1.0, 6.0) / 2.5, precon=Diagonal(np.ones(5)))
    assert g.nMatvec == 1 and g.nIter == 0 and g.converged and g.precon_calls == 0 and same(g.x, np.arange(1.0, 6.0) / 2.5)
    for flexible in (False, True):
        for mm in (1, 2, 3):
            for guess in (None, xs):
                got = ref.pcg(A, b, reltol=1e-14, matvec_max=mm, precon=M, flexible=flexible, guess=guess)
                assert got.nMatvec == mm and not got.converged
                assert len(got.history) == mm + (1 if guess is None else 0)
    # a budget the guess's product uses up: no pass, no application
    got = ref.pcg(A, b, matvec_max=1, precon=M, guess=xs)
    assert got.nMatvec == 1 and got.nIter == 0 and got.precon_calls == 0 and same(got.x, xs)
    # a run of at least one pass ended by the stop test: one application per pass (the halting pass applies nothing, the
    # set-up one)
    for flexible in (False, True):
        got = ref.pcg(A, b, reltol=1e-10, precon=M, flexible=flexible)
        assert got.converged and got.nIter >= 1 and got.precon_calls == got.nIter
        got = ref.pcg(A, b, reltol=1e-14, precon=M, flexible=flexible, matvec_max=7)
        assert not got.converged and got.nIter == 7 and got.precon_calls == 7


def test_breakdowns():
    A = poisson2d(12)
    n = A.shape[0]
    b = rhs_of(A)
    xs = 1.0 + np.arange(n) / n
    # a negative definite preconditioner: <r, M r> < 0 at the set-up
    for guess in (None, xs):
        got = ref.pcg(A, b, precon=Diagonal(np.full(n, -0.25)), guess=guess)
        assert got.breakdown == 2 and not got.converged and got.definite and got.nIter == 0 and got.precon_calls == 1
        assert same(got.x, np.zeros(n) if guess is None else guess) and len(got.history) == 1
    # -A: the curvature test stops the first pass; x untouched, no history entry, p is the direction
    neg = csr_ref.RefCsr(A.indptr, A.indices, -A.data, A.shape)
    got = ref.pcg(neg, b, guess=xs)
    assert not got.definite and got.breakdown == 1 and not got.converged
    assert got.nMatvec == 2 and got.nIter == 0 and len(got.history) == 1 and same(got.x, xs)
    assert same(got.p, b - neg.matvec(xs))
    # ... and without the test the run goes on
    on = ref.pcg(neg, b, guess=xs, check_curvature=False, matvec_max=20)
    assert on.definite and on.breakdown == 0 and on.nIter > 1


def test_constants_and_the_setter():
    from pykrylov_amd import _lib
    assert _lib.MK_PCG == 13
    hdr = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    assert "MK_PCG = 13" in hdr and "MK_IDR = 12" in hdr
    res, args = _lib.PROTOTYPES["mk_solver_set_pcg"]
    assert res is ctypes.c_int and len(args) == 2
    so = os.path.join(ROOT, "pykrylov_amd", "libmikrylov.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert any(ln.split()[-1] == "mk_solver_set_pcg" and ln.split()[1] == "T" for ln in out.splitlines())
    assert ctypes.sizeof(_lib.MkParams) == _lib.MkParams.restart.offset + 8          # mk_params did not change


def test_host_checks_come_before_the_device():
    from pykrylov_amd import PCG, LinearOperator

    class Partitioned(object):
        shape = (8, 8)
        local_size = 4

        @property
        def handle(self):
            raise AssertionError("the library was touched")

    with pytest.raises(NotImplementedError, match="row-partitioned"):
        PCG(Partitioned()).solve(np.ones(4))
    op = LinearOperator(6, 6, matvec=lambda v: 1 / 0)
    for bad in (0, 1, None, "yes", 2.0):
        with pytest.raises(ValueError, match="flexible must be True or False"):
            PCG(op).solve(np.ones(6), flexible=bad)
    with pytest.raises(ValueError, match="square"):
        PCG(LinearOperator(6, 5, matvec=lambda v: v)).solve(np.ones(5))
    s = PCG(op, abstol=1e-9, reltol=1e-7)
    assert (s.abstol, s.reltol, s.precon, s.breakdown, s.definite, s.flexible, s.precon_route, s.acronym) == \
        (1e-9, 1e-7, None, 0, True, False, "none", "PCG")
    assert s.infiniteDescent is None and s.residHistory == []
