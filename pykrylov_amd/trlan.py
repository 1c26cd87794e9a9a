"""Thick-restart Lanczos for a few extreme eigenpairs of a symmetric operator, the whole cycle on the device
(``csrc/mk_trlan.hip``).

Wu and Simon's method: Lanczos with full orthogonalisation against a basis of `ncv` vectors; when the basis is full the
eigenproblem of the small projected matrix is solved on the host, `keep` Ritz vectors are kept by one rotation of the basis
on the device, and the process goes on behind them.  With ``filter=`` the process runs on a Chebyshev-filtered operator
``rho(A)`` (`tools.cheb_filter`, ``csrc/mk_chebfilt.hip``), which spreads a clustered end of the spectrum, and
the pairs are verified on `A` itself.  The class follows the reference's `KrylovMethod` protocol like the
solvers here, although its result is not a solution of ``A x = b``.  The NumPy restatement the device loop is tested against
is ``tests/_trlan_ref.py`` (``tests/_chebfilt_ref.py`` for the filtered cycle)."""
import numpy as np

from . import _lib
from .generic import DeviceRun, KrylovMethod, as_f64_vector

__docformat__ = 'restructuredtext'

MAX_NCV = _lib.MK_TRLAN_MAX_NCV


def default_ncv(n, nev):
    "The basis size `solve` takes when none is given."
    return min(n, MAX_NCV, max(2 * nev + 1, 20))


def default_keep(nev, ncv):
    "The number of Ritz vectors `solve` keeps at a restart when none is given."
    return min(nev + (ncv - nev) // 2, ncv - 1)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class ThickRestartLanczos(KrylovMethod):
    """The `nev` smallest (``'SA'``) or largest (``'LA'``) eigenvalues of a symmetric operator `A`, with eigenvectors.

    ``est_i = |beta S[last, i]|`` estimates the residual norm of Ritz pair i; a pair has converged when its estimate is at
    most ``threshold = max(abstol, reltol * anorm)``, `anorm` being the largest Ritz value in modulus seen so far (defaults:
    ``abstol = 0``, ``reltol = 1e-10``).  The run ends when the `nev` wanted pairs have all converged, at a breakdown (the
    basis spans an invariant subspace: every pair is exact) or when the next cycle's ``ncv - keep`` products would exceed
    `matvec_max`, which is never exceeded.  There is no preconditioner; the one spectral transformation is the Chebyshev
    filter of `solve`'s ``filter=`` (no shift-invert, no interior eigenvalues).

    A single-vector Lanczos method finds ONE copy of a multiple eigenvalue: on such a matrix the pairs returned are
    eigenpairs, but not the `nev` extreme ones counted with multiplicity.

    After `solve`: `w` (ascending), `X` (``nev x n``, row i the eigenvector of ``w[i]``), `residNorms` (the estimates),
    `pairIters` (the cycle, from 1, at which the pair in that place first converged; -1: never), `nconv`, `converged`,
    `breakdown`, `nMatvec`, `nIter` (Lanczos steps), `cycles`, `residHistory` (per cycle the largest estimate among the
    wanted pairs), `residNorm` (its last entry), `residNorm0` (the norm of the start vector), `anorm`, `threshold`, `ncv`,
    `keep`, `workspace_bytes` (the basis allocation), `sweeps` (Jacobi sweeps of the last small eigenproblem).  After a
    breakdown with fewer than `nev` basis vectors `w` and `X` hold only the pairs that exist.
    """

    def __init__(self, op, **kwargs):
        kwargs.setdefault('abstol', 0.0)
        kwargs.setdefault('reltol', 1.0e-10)
        KrylovMethod.__init__(self, op, **kwargs)
        self.name = 'Thick-Restart Lanczos'
        self.acronym = 'TRLAN'
        self.prefix = self.acronym + ': '
        self.w = self.X = self.residNorms = self.pairIters = None
        self.nconv = self.cycles = self.ncv = self.keep = self.workspace_bytes = self.sweeps = 0
        self.breakdown = False
        self.anorm = self.threshold = None
        self.filter_degree = self.filter_interval = None
        self.pilotMatvec = self.outside = 0

    def solve(self, nev, which='SA', ncv=None, keep=None, matvec_max=None, start=None, seed=1, filter=None, **kwargs):
        """Compute `nev` eigenpairs.

        :keywords:
            :which:      ``'SA'`` the smallest, ``'LA'`` the largest eigenvalues
            :ncv:        basis vectors per cycle, ``nev < ncv <= min(n, 128)`` (default ``min(n, 128, max(2 nev + 1, 20))``)
            :keep:       Ritz vectors kept at a restart, ``nev <= keep < ncv`` (default
                         ``min(nev + (ncv - nev) // 2, ncv - 1)``)
            :matvec_max: max. number of operator-vector products, at least `ncv` (default ``max(2 n, ncv)``); never exceeded
            :start:      the start vector, a host array or a `DeviceArray` (default: a hashed vector chosen by `seed`)
            :filter:     None: plain Lanczos on `A`.  A `tools.ChebyshevFilter` F of this operator whose `side` is `which`, or
                         an int d (``tools.cheb_filter_for(A, nev, which, degree=d)``, freed afterwards): Lanczos runs on
                         ``B = rho(A)`` -- every step costs `degree` products of `A` -- and B's estimates only open a
                         gate.  Once they have met ``max(abstol, reltol * anorm_B)``, and in the last cycle the budget
                         allows, the wanted Ritz vectors are verified on `A` after the restart rotation: ``theta = <x, A x>``
                         and ``||A x - theta x||``, one product each.  The run has converged when every such residual is at
                         most ``max(abstol, reltol * max(|a|, |b|, |a0|))`` and goes on from the restart otherwise.  `w` is
                         then ``theta`` ascending, `residNorms` the true residuals, `residHistory` per cycle the largest of
                         them where the cycle was verified (B's largest estimate otherwise), `threshold` and `anorm` those of
                         `A`, `pairIters` the cycle at which B's estimate first met the gate, `nMatvec` every product of `A`
                         (filter steps and verification; a pilot run's are in `pilotMatvec`), and a cycle starts only if its
                         ``(ncv - l) * degree + nev`` products fit into `matvec_max` (default ``max(2 n, ncv * degree + nev)``).
                         New attributes: `filter_degree`, `filter_interval`, `pilotMatvec`, and `outside`, the number of
                         returned `w` that do not lie on the wanted side of the cut -- the sign of a hand-given interval
                         that covers wanted eigenvalues (they are damped, not found); `converged` is then False.
        """
        if self.precon is not None:
            raise ValueError('ThickRestartLanczos takes no preconditioner (a spectral transformation is out of its scope)')
        if getattr(self.op, 'local_size', None) is not None:
            raise NotImplementedError('ThickRestartLanczos: the operator is row-partitioned; the eigensolver is single-GPU')
        shape = getattr(self.op, 'shape', None)
        if shape is None or len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError('ThickRestartLanczos needs a square operator, got shape %s' % (shape if shape is None else tuple(shape),))
        if getattr(self.op, 'symmetric', None) is False:
            raise ValueError('ThickRestartLanczos needs a symmetric operator; this one declares symmetric=False')
        n = int(shape[0])
        if which not in ('SA', 'LA'):
            raise ValueError("ThickRestartLanczos: which must be 'SA' or 'LA', got %r" % (which,))
        if not _is_int(nev) or nev < 1:
            raise ValueError('ThickRestartLanczos: nev must be a positive integer, got %r' % (nev,))
        nev = int(nev)
        if ncv is None:
            ncv = default_ncv(n, nev)
        if not _is_int(ncv) or not nev < ncv <= min(n, MAX_NCV):
            raise ValueError('ThickRestartLanczos: ncv must be an integer with nev = %d < ncv <= min(n, %d) = %d, got %r'
                             % (nev, MAX_NCV, min(n, MAX_NCV), ncv))
        ncv = int(ncv)
        if keep is None:
            keep = default_keep(nev, ncv)
        if not _is_int(keep) or not nev <= keep < ncv:
            raise ValueError('ThickRestartLanczos: keep must be an integer with nev = %d <= keep < ncv = %d, got %r'
                             % (nev, ncv, keep))
        keep = int(keep)
        filt, own = self._filter(filter, nev, which), _is_int(filter)
        try:
            first = ncv if filt is None else ncv * filt.degree + nev
            if matvec_max is None:
                matvec_max = max(2 * n, first)
            if not _is_int(matvec_max) or matvec_max < first:
                raise ValueError('ThickRestartLanczos: matvec_max must be an integer of at least %s = %d (the first cycle must '
                                 'fit), got %r' % ('ncv' if filt is None else 'ncv * degree + nev', first, matvec_max))
            if start is not None and not isinstance(start, _lib.DeviceArray):
                start = as_f64_vector(start, n, 'start')
            op = self._device_operator()
            with DeviceRun(op, _lib.MK_TRLAN, start, None, abstol=float(self.abstol), reltol=float(self.reltol),
                           matvec_max=int(matvec_max), eig=(nev, ncv, 0 if which == 'SA' else 1, keep, int(seed)),
                           filter=None if filt is None else (filt.degree,) + filt.interval + (filt.ref,)) as run:
                res = run.run()
                record = run.vector(nev).reshape(nev, 3)
                have = int(np.sum(~np.isnan(record[:, 0])))
                X = np.stack([run.vector(i) for i in range(have)]) if have else np.zeros((0, n))
                hist = run.history()
            self.filter_degree = None if filt is None else filt.degree
            self.filter_interval = None if filt is None else filt.interval
            self.pilotMatvec = 0 if filt is None else int(filt.pilotMatvec)
        finally:
            if own and filt is not None:
                filt.free()
        op._nMatvec += int(res.nMatvec)
        self.w = record[:have, 0].copy()
        self.X = X
        self.residNorms = record[:have, 1].copy()
        self.pairIters = record[:have, 2].astype(np.int64)
        self.residHistory = list(hist)
        self.residNorm0 = np.float64(res.residNorm0)
        self.residNorm = np.float64(res.residNorm)
        self.anorm = np.float64(res.Anorm)
        self.threshold = np.float64(res.threshold)
        self.nMatvec = int(res.nMatvec)
        self.nIter = int(res.itn)
        self.cycles = int(res.aux[0])
        self.ncv = int(res.aux[1])
        self.keep = int(res.aux[2])
        self.workspace_bytes = int(res.aux[3])
        self.nconv = int(res.aux[4])
        self.breakdown = bool(res.aux[5])
        self.sweeps = int(res.aux[6])
        self.rotation_ms = float(res.aux[7])
        self.outside = 0
        if self.filter_interval is not None:
            a, b = self.filter_interval
            self.outside = int(np.sum(self.w >= a)) if which == 'SA' else int(np.sum(self.w <= b))
        self.converged = bool(res.converged) and self.outside == 0
        self.bestSolution = self.x = X[0] if have else None
        if self._logging():
            self.logger.info('Threshold = %8.2e' % res.threshold)
            self.logger.info('%6d  %8.2e  (%d cycles, %d of %d pairs converged)' % (self.nMatvec, self.residNorm, self.cycles,
                                                                                    self.nconv, nev))
        return res

    def _filter(self, filter, nev, which):
        "The `tools.ChebyshevFilter` behind ``filter=`` (an int: a new one from a pilot run, the caller frees it), or None."
        if filter is None:
            return None
        from . import tools
        from .linop import CsrOperator
        if not isinstance(self.op, CsrOperator):
            raise ValueError('ThickRestartLanczos: filter= needs a device matrix (a CsrOperator); %r is matrix-free or composed'
                             % type(self.op).__name__)
        if _is_int(filter):
            return tools.cheb_filter_for(self.op, nev, which, degree=int(filter))
        if not isinstance(filter, tools.ChebyshevFilter):
            raise ValueError('ThickRestartLanczos: filter must be None, a degree or a tools.ChebyshevFilter, got %r' % (filter,))
        if filter._live() and filter._op is not self.op:
            raise ValueError('ThickRestartLanczos: the filter was made from another matrix than this operator')
        if filter.side != which:
            raise ValueError("ThickRestartLanczos: the filter wants the %s end of the spectrum (its ref lies %s its interval), "
                             "which = %r the other" % (filter.side, 'below' if filter.side == 'SA' else 'above', which))
        return filter


def eigsh(A, k=6, which='LA', ncv=None, tol=1e-10, maxiter=None, v0=None, filter=None):
    """`k` extreme eigenpairs of the symmetric operator `A` in the calling convention of ``scipy.sparse.linalg.eigsh``:
    returns ``(w, X)`` with the eigenvalues ascending and the eigenvectors in the COLUMNS of `X`.  `tol` is the relative
    tolerance (``reltol``; 0 means 1e-15), `maxiter` the largest number of products, `v0` the start vector, `filter` the
    Chebyshev filter of `ThickRestartLanczos.solve` (a degree or a `tools.ChebyshevFilter`).  Raises RuntimeError when the pairs
    have not converged."""
    s = ThickRestartLanczos(A, abstol=0.0, reltol=float(tol) if tol else 1e-15)
    s.solve(k, which=which, ncv=ncv, matvec_max=maxiter, start=v0, filter=filter)
    if not s.converged:
        raise RuntimeError('eigsh: %d of %d eigenpairs converged in %d products' % (s.nconv, k, s.nMatvec))
    return s.w, s.X.T
