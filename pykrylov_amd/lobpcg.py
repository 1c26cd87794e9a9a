"""LOBPCG: a block, preconditioned eigensolver for a few extreme eigenpairs of a symmetric operator, the whole loop on the
device (``csrc/mk_lobpcg.hip``).

Knyazev's locally optimal block preconditioned conjugate gradient method: a block `X` of `block` vectors, the preconditioned
residuals `W` and the previous directions `P`; each iteration solves the Rayleigh-Ritz problem on ``span[X, W, P]`` (at most
48 vectors) on the host and rotates the block on the device.  It needs no inner solves, it consumes a preconditioner, and as a
block method it finds a multiple eigenvalue with its multiplicity -- the three things `ThickRestartLanczos` cannot do.  The
class follows the reference's `KrylovMethod` protocol like the solvers here, although its result is not a solution of
``A x = b``.  The NumPy restatement the device loop is tested against is ``tests/_lobpcg_ref.py``."""
import numpy as np

from . import _lib
from .generic import DeviceRun, KrylovMethod, resolve_precon

__docformat__ = 'restructuredtext'

MAX_BLOCK = _lib.MK_LOBPCG_MAX_BLOCK


def default_block(n, nev):
    "The block size `solve` takes when none is given."
    return min(MAX_BLOCK, n // 3, max(nev + 2, (3 * nev + 1) // 2))


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class LOBPCG(KrylovMethod):
    """The `nev` smallest (``'SA'``) or largest (``'LA'``) eigenvalues of a symmetric operator `A`, counted with their
    multiplicity, with eigenvectors.  `precon` is a symmetric positive definite approximation of the inverse of `A`, as the
    square solvers take it (``None``, a `DiagonalOperator`, a device matrix, `tools.ic0`, `tools.chebyshev`, `tools.fsai`,
    `tools.amg`, an `InverseLBFGSOperator`, or anything with ``precon * r``, called back on the host); it steers towards the
    smallest eigenvalues, so ``'LA'`` with a preconditioner is a ValueError.

    A pair has converged when its residual norm ``||A x - theta x||``, formed from the loop's own ``A X``, is at most
    ``threshold = max(abstol, reltol * anorm)`` (defaults: ``abstol = 0``, ``reltol = 1e-10``).  `anorm` is a LOWER estimate
    of the norm of `A`: the largest Ritz value in modulus of every projected problem seen so far (0.55 to 1.0 of the largest
    eigenvalue on the stencil matrices, 0.04 to 0.08 on ``1138bus`` with `tools.amg`), so the test is never looser than
    `ThickRestartLanczos`'s.  Soft locking is part of the method: a column whose residual norm has met the threshold --
    any of the `block` columns, not only the first `nev` -- takes no further preconditioner application and product and
    stays locked, while the Rayleigh-Ritz step goes on rotating it.  The run ends when the first `nev` pairs have all
    converged, at a breakdown (the projected Gram matrix fails its Cholesky pivot test twice in one iteration: `X` is the
    last iterate) or when the next iteration's products would exceed `matvec_max`, which is never exceeded.

    Choose ``block > nev``: the guard columns speed up the last wanted pairs (``1138bus`` ``'LA'`` with
    ``nev = block = 16`` stalls at a residual of 4e-5 after 400 iterations).

    After `solve`: `w` (ascending), `X` (``nev x n``, row i the eigenvector of ``w[i]``), `residNorms`, `residNorm` (the
    largest of them), `residHistory` (the largest of the first `nev` norms: of the start block's Ritz pairs, then one per
    iteration), `threshold`, `pairIters` (the iteration, 0 for the start block's own pairs, at which the pair first met the
    threshold; -1: never), `nconv`, `converged`, `breakdown`, `restarts` (projected problems solved again without `P`, and
    re-activations of a fully locked block), `anorm`, `nMatvec`, `nIter`, `block`, `active` (active columns of the last
    iteration), `precon_route`, `workspace_bytes`, `sweeps` (Jacobi sweeps of the last projected problem).
    """

    def __init__(self, op, **kwargs):
        kwargs.setdefault('abstol', 0.0)
        kwargs.setdefault('reltol', 1.0e-10)
        KrylovMethod.__init__(self, op, **kwargs)
        self.name = 'Locally Optimal Block Preconditioned Conjugate Gradient'
        self.acronym = 'LOBPCG'
        self.prefix = self.acronym + ': '
        self.w = self.X = self.residNorms = self.pairIters = None
        self.nconv = self.block = self.active = self.workspace_bytes = self.sweeps = self.restarts = 0
        self.breakdown = False
        self.anorm = self.threshold = None
        self.precon_route = 'none'

    def solve(self, nev, which='SA', block=None, matvec_max=None, start=None, seed=1, **kwargs):
        """Compute `nev` eigenpairs.

        :keywords:
            :which:      ``'SA'`` the smallest, ``'LA'`` the largest eigenvalues
            :block:      vectors in the block, ``nev <= block <= min(16, n // 3)`` (default
                         ``min(16, n // 3, max(nev + 2, (3 nev + 1) // 2))``)
            :matvec_max: max. number of operator-vector products, at least `block` (default ``max(2 n, block)``); never
                         exceeded
            :start:      the start block: a ``block x n`` host array or a `DeviceArray` of ``block * n`` doubles, vector
                         after vector (default: hashed vectors chosen by ``seed + j``)
        """
        if 'guess' in kwargs:
            raise ValueError('LOBPCG takes a start block (start=), not an initial guess')
        if getattr(self.op, 'local_size', None) is not None:
            raise NotImplementedError('LOBPCG: the operator is row-partitioned; the eigensolver is single-GPU')
        shape = getattr(self.op, 'shape', None)
        if shape is None or len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError('LOBPCG needs a square operator, got shape %s' % (shape if shape is None else tuple(shape),))
        if getattr(self.op, 'symmetric', None) is False:
            raise ValueError('LOBPCG needs a symmetric operator; this one declares symmetric=False')
        n = int(shape[0])
        if which not in ('SA', 'LA'):
            raise ValueError("LOBPCG: which must be 'SA' or 'LA', got %r" % (which,))
        if which == 'LA' and self.precon is not None:
            raise ValueError("LOBPCG: a preconditioner approximates the inverse of A, which steers towards the smallest "
                             "eigenvalues; which='LA' takes none")
        if not _is_int(nev) or nev < 1:
            raise ValueError('LOBPCG: nev must be a positive integer, got %r' % (nev,))
        nev = int(nev)
        top = min(MAX_BLOCK, n // 3)
        if block is None:
            block = default_block(n, nev)
        if not _is_int(block) or not nev <= block <= top:
            raise ValueError('LOBPCG: block must be an integer with nev = %d <= block <= min(%d, n // 3) = %d, got %r'
                             % (nev, MAX_BLOCK, top, block))
        block = int(block)
        if matvec_max is None:
            matvec_max = max(2 * n, block)
        if not _is_int(matvec_max) or matvec_max < block:
            raise ValueError('LOBPCG: matvec_max must be an integer of at least block = %d (the products of the start block '
                             'must fit), got %r' % (block, matvec_max))
        if start is not None and not isinstance(start, _lib.DeviceArray):
            a = np.asarray(start)
            if a.dtype.kind == 'c':
                raise TypeError('start: complex data is not supported on the device path (fp64 only)')
            if a.shape != (block, n):
                raise ValueError('start has shape %s, expected (%d, %d)' % (a.shape, block, n))
            start = np.ascontiguousarray(a, dtype=np.float64).reshape(block * n)
        elif start is not None and start.n != block * n:
            raise ValueError('start has %d entries, expected block * n = %d' % (start.n, block * n))
        route, payload = resolve_precon(self.precon, n, 'precon', 'LOBPCG')
        op = self._device_operator()
        with DeviceRun(op, _lib.MK_LOBPCG, start, None, precon_diag=payload, abstol=float(self.abstol),
                       reltol=float(self.reltol), matvec_max=int(matvec_max),
                       eig=(nev, block, 0 if which == 'SA' else 1, 0, int(seed))) as run:
            res = run.run()
            record = run.vector(nev).reshape(nev, 3)
            X = np.stack([run.vector(i) for i in range(nev)])
            hist = run.history()
            self.precon_route = run.precon_kind
        assert route == self.precon_route
        op._nMatvec += int(res.nMatvec)
        self.w = record[:, 0].copy()
        self.X = X
        self.residNorms = record[:, 1].copy()
        self.pairIters = record[:, 2].astype(np.int64)
        self.residHistory = list(hist)
        self.residNorm = np.float64(res.residNorm)
        self.anorm = np.float64(res.Anorm)
        self.threshold = np.float64(res.threshold)
        self.nMatvec = int(res.nMatvec)
        self.nIter = int(res.itn)
        self.block = int(res.aux[1])
        self.active = int(res.aux[2])
        self.workspace_bytes = int(res.aux[3])
        self.nconv = int(res.aux[4])
        self.breakdown = bool(res.aux[5])
        self.sweeps = int(res.aux[6])
        self.restarts = int(res.aux[7])
        self.converged = bool(res.converged)
        self.bestSolution = self.x = X[0]
        if self._logging():
            self.logger.info('Threshold = %8.2e' % res.threshold)
            self.logger.info('%6d  %8.2e  (%d iterations, %d of %d pairs converged, %s)'
                             % (self.nMatvec, self.residNorm, self.nIter, self.nconv, nev, self.precon_route))
        return res


def lobpcg(A, k=6, which='SA', M=None, tol=1e-10, maxiter=None, X0=None):
    """`k` extreme eigenpairs of the symmetric operator `A` by LOBPCG: returns ``(w, X)`` with the eigenvalues ascending and
    the eigenvectors in the COLUMNS of `X`, as `eigsh` does.  `M` is the preconditioner, `tol` the relative tolerance
    (``reltol``; 0 means 1e-15), `maxiter` the largest number of products, `X0` the start block with the vectors in its
    COLUMNS (``n x block``; its width is the block size).  Raises RuntimeError when the pairs have not converged."""
    s = LOBPCG(A, abstol=0.0, reltol=float(tol) if tol else 1e-15, precon=M)
    block = start = None
    if X0 is not None:
        X0 = np.asarray(X0)
        if X0.ndim != 2:
            raise ValueError('lobpcg: X0 must be an n x block array, got shape %s' % (X0.shape,))
        block, start = int(X0.shape[1]), np.ascontiguousarray(X0.T)
    s.solve(k, which=which, block=block, matvec_max=maxiter, start=start)
    if not s.converged:
        raise RuntimeError('lobpcg: %d of %d eigenpairs converged in %d products' % (s.nconv, k, s.nMatvec))
    return s.w, s.X.T
