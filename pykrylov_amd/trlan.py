"""Thick-restart Lanczos for a few extreme eigenpairs of a symmetric operator, the whole cycle on the device
(``csrc/mk_trlan.hip``).

Wu and Simon's method: Lanczos with full orthogonalisation against a basis of `ncv` vectors; when the basis is full the
eigenproblem of the small projected matrix is solved on the host, `keep` Ritz vectors are kept by one rotation of the basis
on the device, and the process goes on behind them.  The class follows the reference's `KrylovMethod` protocol like the
solvers here, although its result is not a solution of ``A x = b``.  The NumPy restatement the device loop is tested against
is ``tests/_trlan_ref.py``."""
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
    `matvec_max`, which is never exceeded.  There is no preconditioner and no spectral transformation.

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

    def solve(self, nev, which='SA', ncv=None, keep=None, matvec_max=None, start=None, seed=1, **kwargs):
        """Compute `nev` eigenpairs.

        :keywords:
            :which:      ``'SA'`` the smallest, ``'LA'`` the largest eigenvalues
            :ncv:        basis vectors per cycle, ``nev < ncv <= min(n, 128)`` (default ``min(n, 128, max(2 nev + 1, 20))``)
            :keep:       Ritz vectors kept at a restart, ``nev <= keep < ncv`` (default
                         ``min(nev + (ncv - nev) // 2, ncv - 1)``)
            :matvec_max: max. number of operator-vector products, at least `ncv` (default ``max(2 n, ncv)``); never exceeded
            :start:      the start vector, a host array or a `DeviceArray` (default: a hashed vector chosen by `seed`)
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
        if matvec_max is None:
            matvec_max = max(2 * n, ncv)
        if not _is_int(matvec_max) or matvec_max < ncv:
            raise ValueError('ThickRestartLanczos: matvec_max must be an integer of at least ncv = %d (the first cycle must '
                             'fit), got %r' % (ncv, matvec_max))
        if start is not None and not isinstance(start, _lib.DeviceArray):
            start = as_f64_vector(start, n, 'start')
        op = self._device_operator()
        with DeviceRun(op, _lib.MK_TRLAN, start, None, abstol=float(self.abstol), reltol=float(self.reltol),
                       matvec_max=int(matvec_max), eig=(nev, ncv, 0 if which == 'SA' else 1, keep, int(seed))) as run:
            res = run.run()
            record = run.vector(nev).reshape(nev, 3)
            have = int(np.sum(~np.isnan(record[:, 0])))
            X = np.stack([run.vector(i) for i in range(have)]) if have else np.zeros((0, n))
            hist = run.history()
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
        self.converged = bool(res.converged)
        self.bestSolution = self.x = X[0] if have else None
        if self._logging():
            self.logger.info('Threshold = %8.2e' % res.threshold)
            self.logger.info('%6d  %8.2e  (%d cycles, %d of %d pairs converged)' % (self.nMatvec, self.residNorm, self.cycles,
                                                                                    self.nconv, nev))
        return res


def eigsh(A, k=6, which='LA', ncv=None, tol=1e-10, maxiter=None, v0=None):
    """`k` extreme eigenpairs of the symmetric operator `A` in the calling convention of ``scipy.sparse.linalg.eigsh``:
    returns ``(w, X)`` with the eigenvalues ascending and the eigenvectors in the COLUMNS of `X`.  `tol` is the relative
    tolerance (``reltol``; 0 means 1e-15), `maxiter` the largest number of products, `v0` the start vector.  Raises
    RuntimeError when the pairs have not converged."""
    s = ThickRestartLanczos(A, abstol=0.0, reltol=float(tol) if tol else 1e-15)
    s.solve(k, which=which, ncv=ncv, matvec_max=maxiter, start=v0)
    if not s.converged:
        raise RuntimeError('eigsh: %d of %d eigenpairs converged in %d products' % (s.nconv, k, s.nMatvec))
    return s.w, s.X.T
