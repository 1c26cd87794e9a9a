"""The Chebyshev filter and the filtered thick-restart Lanczos cycle without a device: the restatement of the filter
(tests/_chebfilt_ref.py) against the closed form on diagonal matrices; the automatic cut of `tools.cheb_filter_for` against
dense eigenvalues; the restatement of the filtered cycle on the CPU list of tests/test_trlan_cpu.py, held to that file's
bounds; the step counts the filter is there for; the host-side checks of the new keywords, which run before any device is
touched; the new entry points in the header."""
import os
import re

import numpy as np
import pytest

from oracle import csr_ref
from tests import _chebfilt_ref as ref
from tests import _trlan_ref as plain
from test_trlan_cpu import CASES, Op, dense_eigs, matrix as _trlan_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MAT, _EIG, _PLAIN = {}, {}, {}


def matrix(name):
    if name.startswith("poisson2d_"):
        if name not in _MAT:
            _MAT[name] = csr_ref.poisson2d(int(name.split("_")[1]))
        return _MAT[name]
    return _trlan_matrix(name)


def eigs(name):
    if name.startswith("poisson2d_"):
        if name not in _EIG:
            _EIG[name] = np.linalg.eigvalsh(matrix(name).to_dense())
        return _EIG[name]
    return dense_eigs(name)


# ---------------------------------------------------------------------------------------------- the filter
def test_coefficients_are_the_scaled_three_term_recurrence():
    """sigma_j = T_{j-1}(z0) / T_j(z0), z0 = (a0 - c) / e: the scaling that keeps y_j = T_j((A - c)/e) x / T_j(z0)."""
    a, b, a0, d = 1.0, 4.0, 0.25, 12
    c, e, p, q = ref.coefficients(a, b, a0, d)
    assert (c, e) == (2.5, 1.5) and q[0] == 0.0 and len(p) == len(q) == d
    z0 = (a0 - c) / e
    T = [1.0, z0]
    for j in range(2, d + 1):
        T.append(2.0 * z0 * T[-1] - T[-2])
    sigma = np.array([T[j - 1] / T[j] for j in range(1, d + 1)])
    assert np.allclose(p[0], sigma[0] / e, rtol=1e-14) and np.allclose(p[1:], 2.0 * sigma[1:] / e, rtol=1e-12)
    assert np.allclose(q[1:], sigma[:-1] * sigma[1:], rtol=1e-12)


@pytest.mark.parametrize("side", ["SA", "LA"])
@pytest.mark.parametrize("degree", [1, 2, 3, 8, 32])
def test_apply_on_a_diagonal_matrix_is_the_closed_form(degree, side):
    """On diag(lambda) the filter is rho(lambda_i) entry by entry; 1e-12 of the largest entry of the result (an entry at a zero
    of T_d has no relative accuracy of its own)."""
    n = 61
    lam = np.linspace(-0.5, 4.5, n)                              # some beyond a0, some between a0 and the interval, most inside
    A = csr_ref.from_coo(np.arange(n), np.arange(n), lam, (n, n))
    a, b, a0 = (1.0, 4.5, -0.25) if side == "SA" else (-0.5, 3.0, 4.25)
    x = 1.0 + np.random.default_rng(5).random(n)
    got = ref.apply(A, x, degree, a, b, a0)
    want = ref.rho(lam, degree, a, b, a0) * x
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(degree, side, "relative error", err)
    assert err <= 1e-12
    inside = (lam >= a) & (lam <= b)
    bound = 1.0 / np.cosh(degree * np.arccosh(abs((a0 - 0.5 * (a + b)) / (0.5 * (b - a)))))     # 1 / |T_d(z0)|
    assert np.all(np.abs(got[inside]) <= (1.0 + 1e-9) * bound * np.abs(x[inside]))      # damped to 1 / T_d(z0) inside
    wanted_end = lam < a0 if side == "SA" else lam > a0
    assert np.all(got[wanted_end] / x[wanted_end] > 1.0)                               # ... and growing beyond a0


def test_gershgorin_interval():
    A = matrix("poisson2d_12")
    assert ref.gershgorin(A) == (0.0, 8.0)
    V = matrix("varcoef_7_5_3")
    D = V.to_dense()
    off = np.sum(np.abs(D), axis=1) - np.abs(np.diag(D))
    lo, hi = ref.gershgorin(V)
    assert abs(lo - np.min(np.diag(D) - off)) <= 1e-13 * hi and abs(hi - np.max(np.diag(D) + off)) <= 1e-13 * hi
    ev = eigs("varcoef_7_5_3")
    assert lo <= ev[0] and ev[-1] <= hi
    assert ref.interval(V, 0.5, None) == (0.5, hi) and ref.interval(V, None, 3.0) == (lo, 3.0) and ref.interval(V, 1.0, 2.0) == (1.0, 2.0)


CUTS = sorted({(nm, w, nev) for nm, w, nev, _ in CASES})


@pytest.mark.parametrize("name,which,nev", CUTS, ids=["%s-%s-%d" % c for c in CUTS])
def test_the_automatic_cut_never_covers_a_wanted_eigenvalue(name, which, nev):
    """Cauchy interlacing: Ritz value i from an end is no more extreme than eigenvalue i, so the cut at Ritz value nev lies at
    or beyond the (nev+1)-th eigenvalue from the wanted end, and the reference point outside the interval."""
    A = matrix(name)
    ev = eigs(name)
    a, b, a0, pilot, d = ref.filter_for(A, nev, which)
    lo, hi = ref.gershgorin(A)
    assert pilot.steps == plain.default_ncv(A.shape[0], nev)
    if which == "SA":
        assert a >= ev[nev] and b == hi and a0 < a and a0 <= pilot.ritz[0]
    else:
        assert b <= ev[-1 - nev] and a == lo and a0 > b and a0 >= pilot.ritz[-1]
    # the degree: 16 unless the wanted end is so well separated that rho would fall below 2^-16 at the cut
    z0 = abs(a0 - 0.5 * (a + b)) / (0.5 * (b - a))
    assert 1 <= d <= 16 and np.cosh(d * np.arccosh(z0)) <= 2.0 ** 16 * (1 + 1e-12)
    assert d == 16 or np.cosh((d + 1) * np.arccosh(z0)) > 2.0 ** 16 * (1 - 1e-12)


# ---------------------------------------------------------------------------------------------- the filtered cycle
def plain_run(name, which, nev, ncv):
    key = (name, which, nev, ncv)
    if key not in _PLAIN:
        _PLAIN[key] = plain.trlan(matrix(name), nev, which, ncv=ncv, reltol=1e-10, abstol=0.0, matvec_max=2000)
    return _PLAIN[key]


def check_filtered(name, r, which, nev, reltol, distinct=False):
    """tests/test_trlan_cpu.py's bounds: eigenvalue error 1e-12 lambda_max, true residual 2 reltol lambda_max.  `distinct`: the
    matrix has multiple eigenvalues, of which a single-vector method returns one copy each."""
    A = matrix(name)
    ev = eigs(name)
    lam = ev[-1]
    if distinct:
        ev = ev[np.concatenate(([True], np.diff(ev) > 1e-9 * lam))]
    want = ev[:nev] if which == "SA" else ev[-nev:]
    # (a strong filter on a small matrix leaves B = rho(A) a numerical rank below ncv: the cycle then ends in a breakdown of
    #  B's recurrence, and the verification on A decides like after any other cycle)
    assert r.converged and r.nconv == nev
    assert r.w.shape == (nev,) and r.X.shape == (nev, A.shape[0]) and np.all(np.diff(r.w) >= 0)
    assert np.max(np.abs(r.w - want)) <= 1e-12 * lam, np.max(np.abs(r.w - want)) / lam
    true = np.array([np.linalg.norm(A.matvec(r.X[i]) - r.w[i] * r.X[i]) for i in range(nev)])
    assert np.max(true) <= 2.0 * reltol * lam, np.max(true) / lam
    assert np.max(np.abs(r.residNorms - true)) <= 1e-12 * lam
    assert np.max(np.abs(r.X @ r.X.T - np.eye(nev))) <= 1e-12
    assert np.all(r.residNorms <= r.threshold) and np.all(r.pairIters >= 1) and np.all(r.pairIters <= r.cycles)
    assert len(r.history) == r.cycles and r.history[-1] == r.residNorm == np.max(r.residNorms)
    assert r.verified and r.verified[-1] == r.cycles and r.verified == list(range(r.verified[0], r.cycles + 1))


@pytest.mark.parametrize("name,which,nev,ncv", CASES, ids=["%s-%s-%d-%d" % c for c in CASES])
def test_the_filtered_restatement_finds_the_extreme_pairs(name, which, nev, ncv):
    """The automatic interval and degree (16, or what `degree_cap` leaves of it), wherever the plain restatement converges; the
    budget is the plain test's 2000 products for the Lanczos steps times the degree."""
    base = plain_run(name, which, nev, ncv)
    assert base.converged
    A = matrix(name)
    a, b, a0, pilot, d = ref.filter_for(A, nev, which)
    r = ref.trlan_filtered(A, nev, which, d, a, b, a0, ncv=ncv, reltol=1e-10, abstol=0.0, matvec_max=16 * 2000)
    print(name, which, nev, ncv, "degree", d, "plain steps", base.nIter, "filtered steps", r.nIter, "products", r.nMatvec,
          "pilot", pilot.steps, "cycles", r.cycles, "breakdown", r.breakdown)
    assert r.nMatvec <= 16 * 2000 and r.nMatvec == d * r.nIter + nev * len(r.verified)
    assert r.anorm == max(abs(a), abs(b), abs(a0)) and r.threshold == 1e-10 * r.anorm
    check_filtered(name, r, which, nev, 1e-10)


@pytest.mark.parametrize("name", ["poisson1d_300", "poisson2d_48"])
def test_the_filter_halves_the_lanczos_steps_at_a_clustered_end(name):
    A = matrix(name)
    base = plain.trlan(A, 4, "SA", ncv=20, reltol=1e-10, abstol=0.0, matvec_max=4000)
    a, b, a0, pilot, d = ref.filter_for(A, 4, "SA")
    r = ref.trlan_filtered(A, 4, "SA", 16, a, b, a0, ncv=20, reltol=1e-10, abstol=0.0, matvec_max=64000)
    print(name, "plain steps", base.nIter, "filtered steps", r.nIter, "products", r.nMatvec, "pilot", pilot.steps)
    assert base.converged
    check_filtered(name, r, "SA", 4, 1e-10, distinct=name.startswith("poisson2d"))
    assert 2 * r.nIter <= base.nIter, (r.nIter, base.nIter)


def test_the_budget_is_never_exceeded_and_the_last_cycle_is_verified():
    name = "1138bus"
    A = matrix(name)
    a, b, a0, _, _ = ref.filter_for(A, 4, "SA")
    for mm in (16 * 4 + 4, 16 * 4 + 4 + 6 * 4 + 4, 200):
        r = ref.trlan_filtered(A, 4, "SA", 4, a, b, a0, ncv=16, reltol=1e-10, matvec_max=mm)
        assert not r.converged and r.nMatvec <= mm and r.verified == [r.cycles] and r.nMatvec == 4 * r.nIter + 4
        assert r.nMatvec + (16 - r.keep) * 4 + 4 > mm
        true = np.array([np.linalg.norm(A.matvec(r.X[i]) - r.w[i] * r.X[i]) for i in range(4)])
        assert np.max(np.abs(r.residNorms - true)) <= 1e-12 * eigs(name)[-1] and r.residNorm == np.max(r.residNorms) > r.threshold
    assert ref.trlan_filtered(A, 4, "SA", 4, a, b, a0, ncv=16, matvec_max=68).cycles == 1


def test_breakdown_on_a_multiple_of_the_identity():
    A = matrix("2.5I_5")
    r = ref.trlan_filtered(A, 1, "SA", 3, 3.0, 5.0, 2.0, ncv=3)
    assert r.breakdown and r.converged and r.nIter == 1 and r.nMatvec == 3 + 1 and r.cycles == 1 and r.verified == [1]
    assert abs(r.w[0] - 2.5) <= 4 * 2.5 * 2.0 ** -52 and r.residNorms[0] <= 1e-15
    two = ref.trlan_filtered(A, 2, "SA", 3, 3.0, 5.0, 2.0, ncv=3)
    assert two.breakdown and not two.converged and two.w.shape == (1,) and two.X.shape == (1, 5)


def test_argument_errors_of_the_restatement():
    A = matrix("varcoef_7_5_3")
    good = dict(nev=2, which="SA", degree=4, a=1.0, b=8.0, a0=0.1, ncv=9)
    ref.trlan_filtered(A, **good)
    for kw in (dict(which="LA"), dict(a0=1.0), dict(a0=4.0), dict(degree=0), dict(degree=129), dict(matvec_max=37), dict(ncv=2),
               dict(which="SM")):
        with pytest.raises(ValueError):
            ref.trlan_filtered(A, **dict(good, **kw))


# ---------------------------------------------------------------------------------------------- host logic
def test_host_side_checks_run_before_any_device_is_touched(monkeypatch):
    from pykrylov_amd import ThickRestartLanczos, _lib, eigsh, tools

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "init", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    for f in (5, 2.5, "x"):                                       # a matrix-free operator takes no filter, whatever it is
        with pytest.raises(ValueError, match="matrix-free or composed"):
            ThickRestartLanczos(Op()).solve(2, filter=f)
    with pytest.raises(ValueError, match="matrix-free or composed"):
        eigsh(Op(), k=2, which="SA", filter=8)
    with pytest.raises(TypeError):
        tools.cheb_filter(Op(), 4, (1.0, 2.0), 0.0)               # (no CSR arrays on the device)
    with pytest.raises(TypeError):
        tools.cheb_filter_for(Op(), 2)


def test_the_filter_enters_through_a_third_long_block_and_no_function_was_added(tmp_path):
    import ctypes
    import subprocess
    from pykrylov_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mikrylov.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.PROTOTYPES) and not [f for f in declared if "filt" in f]
    assert _lib.MK_FILTER_MAX_DEGREE == 128 and re.search(r"#define MK_FILTER_MAX_DEGREE 128\b", hdr)
    assert re.search(r"\}\s*mk_params_filter;", hdr)
    T = _lib.MkParamsFilter
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mikrylov.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mk_params_filter), offsetof(mk_params_filter, eig),'
                   'offsetof(mk_params_filter, degree), offsetof(mk_params_filter, a), offsetof(mk_params_filter, b),'
                   'offsetof(mk_params_filter, a0));return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(T), T.eig.offset, T.degree.offset, T.a.offset, T.b.offset, T.a0.offset]
    assert len({ctypes.sizeof(T), ctypes.sizeof(_lib.MkParamsEig), ctypes.sizeof(_lib.MkParamsShifts),
                ctypes.sizeof(_lib.MkParams)}) == 4                   # struct_size tells the blocks apart
