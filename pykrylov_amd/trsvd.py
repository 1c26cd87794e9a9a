"""Thick-restart Lanczos bidiagonalisation for a few extreme singular triplets of a device matrix of any shape, the whole
cycle on the device (``csrc/mk_trsvd.hip``).

Baglama and Reichel's method (SLEPc's TRLBD): Golub-Kahan-Lanczos bidiagonalisation with a basis of `ncv` vectors on either
side; when the bases are full the SVD of the small projected matrix is computed on the host by a one-sided Jacobi iteration,
`keep` triplets are kept by one rotation of each basis on the device, and the process goes on behind them.  The short basis
is always orthogonalised in full; the long one in full (``reorth='full'``) or, following Simon and Zha, only against the
vector before (``reorth='one-sided'``), inside the product kernel.  The class follows the reference's `KrylovMethod` protocol
like the solvers here, although its result is not a solution of ``A x = b``.  The NumPy restatement the device loop is tested
against is ``tests/_trsvd_ref.py``."""
import numpy as np

from . import _lib
from .generic import DeviceRun, KrylovMethod, as_f64_vector
from .trlan import MAX_NCV, _is_int, default_keep

__docformat__ = 'restructuredtext'


def default_ncv(short, nsv):
    "The basis size `solve` takes when none is given (`short` = min(shape))."
    return min(short, MAX_NCV, max(2 * nsv + 1, 20))


class ThickRestartSVD(KrylovMethod):
    """The `nsv` largest (``'LM'``) or smallest (``'SM'``) singular values of an operator `A` of any shape, with their left
    and right singular vectors.  `A` is a `CsrOperator`, or a matrix-free operator with ``A * v`` and ``A.T * u``.

    A wide operator is swapped for its transpose first (`transposed`), so that the start vector and the fully orthogonalised
    basis live in the short space.  ``est_i = |beta X[last, i]|`` is the norm of the residual ``A' u_i - s_i v_i`` of triplet
    i (``A v_i = s_i u_i`` holds to rounding); a triplet has converged when its estimate is at most ``threshold =
    max(abstol, reltol * anorm)``, `anorm` being the largest singular value of a projected matrix so far (defaults:
    ``abstol = 0``, ``reltol = 1e-10``).  The run ends when the `nsv` wanted triplets have all converged, at a breakdown
    (the bases span a pair of singular subspaces: every triplet is exact) or when the next cycle's ``2 (ncv - keep)``
    products would exceed `matvec_max`, which is never exceeded.  There is no preconditioner and no spectral
    transformation: ``'SM'`` finds the smallest singular values where they are separated from the rest relative to the
    largest, and converges slowly, or not at all within `matvec_max`, where they are not (harmonic extraction and
    shift-invert are out of scope).

    After a breakdown in alpha (``breakdown == 2``: `A` is rank deficient on the space the start vector spans) the smallest
    singular value is zero: ``'SM'`` returns it as ``s = 0`` with a right vector in the null space and a ZERO left vector.

    After `solve`: `s` (descending, for either `which`), `U` (``nsv x nrows``, row i the left vector of ``s[i]``), `V`
    (``nsv x ncols``), `residNorms` (the estimates), `pairIters` (the cycle, from 1, at which the triplet in that place
    first converged; -1: never), `nconv`, `converged`, `breakdown` (0 none, 1 a beta, 2 an alpha, 3 a start vector
    without a positive, finite norm), `nMatvec` (products with `A` and with ``A.T`` both count), `nIter` (steps), `cycles`,
    `residHistory` (per cycle the largest estimate among the wanted triplets), `residNorm` (its last entry), `residNorm0`
    (the norm of the start vector), `anorm`, `threshold`, `ncv`, `keep`, `reorth`, `transposed`, `workspace_bytes` (the two
    basis allocations), `sweeps` (Jacobi sweeps of the last small SVD).  After a breakdown with fewer than `nsv` steps, or a
    run that halted before its first step, `s`, `U` and `V` hold only the triplets that exist.
    """

    def __init__(self, op, **kwargs):
        kwargs.setdefault('abstol', 0.0)
        kwargs.setdefault('reltol', 1.0e-10)
        KrylovMethod.__init__(self, op, **kwargs)
        self.name = 'Thick-Restart Lanczos Bidiagonalisation'
        self.acronym = 'TRSVD'
        self.prefix = self.acronym + ': '
        self.s = self.U = self.V = self.residNorms = self.pairIters = None
        self.nconv = self.cycles = self.ncv = self.keep = self.workspace_bytes = self.sweeps = self.breakdown = 0
        self.reorth = None
        self.transposed = False
        self.anorm = self.threshold = None

    def solve(self, nsv, which='LM', ncv=None, keep=None, matvec_max=None, start=None, seed=1, reorth='full', **kwargs):
        """Compute `nsv` singular triplets.

        :keywords:
            :which:      ``'LM'`` the largest, ``'SM'`` the smallest singular values
            :ncv:        basis vectors per cycle, ``nsv < ncv <= min(min(shape), 128)`` (default
                         ``min(min(shape), 128, max(2 nsv + 1, 20))``)
            :keep:       triplets kept at a restart, ``nsv <= keep < ncv`` (default ``min(nsv + (ncv - nsv) // 2, ncv - 1)``)
            :matvec_max: max. number of products with `A` and ``A.T`` together (default ``max(4 min(shape), 2 ncv)``); never
                         exceeded -- a run whose first cycle (``2 ncv`` products) does not fit ends without a triplet
            :start:      the start vector, ``min(shape)`` entries, a host array or a `DeviceArray` (default: a hashed vector
                         chosen by `seed`)
            :reorth:     ``'full'`` both bases are orthogonalised at every step; ``'one-sided'`` only the short one
        """
        if self.precon is not None or 'precon' in kwargs:
            raise ValueError('ThickRestartSVD takes no preconditioner (a spectral transformation is out of its scope)')
        if getattr(self.op, 'local_size', None) is not None:
            raise NotImplementedError('ThickRestartSVD: the operator is row-partitioned; the solver is single-GPU')
        shape = getattr(self.op, 'shape', None)
        if shape is None or len(shape) != 2:
            raise ValueError('ThickRestartSVD needs an operator with a two-dimensional shape, got %r' % (shape,))
        nrows, ncols = int(shape[0]), int(shape[1])
        short = min(nrows, ncols)
        if which not in ('LM', 'SM'):
            raise ValueError("ThickRestartSVD: which must be 'LM' or 'SM', got %r" % (which,))
        if reorth not in ('full', 'one-sided'):
            raise ValueError("ThickRestartSVD: reorth must be 'full' or 'one-sided', got %r" % (reorth,))
        if not _is_int(nsv) or nsv < 1:
            raise ValueError('ThickRestartSVD: nsv must be a positive integer, got %r' % (nsv,))
        nsv = int(nsv)
        if ncv is None:
            ncv = default_ncv(short, nsv)
        if not _is_int(ncv) or not nsv < ncv <= min(short, MAX_NCV):
            raise ValueError('ThickRestartSVD: ncv must be an integer with nsv = %d < ncv <= min(min(shape), %d) = %d, got %r'
                             % (nsv, MAX_NCV, min(short, MAX_NCV), ncv))
        ncv = int(ncv)
        if keep is None:
            keep = default_keep(nsv, ncv)
        if not _is_int(keep) or not nsv <= keep < ncv:
            raise ValueError('ThickRestartSVD: keep must be an integer with nsv = %d <= keep < ncv = %d, got %r'
                             % (nsv, ncv, keep))
        keep = int(keep)
        if matvec_max is None:
            matvec_max = max(4 * short, 2 * ncv)
        if not _is_int(matvec_max) or matvec_max < 0:
            raise ValueError('ThickRestartSVD: matvec_max must be a non-negative integer, got %r' % (matvec_max,))
        if start is not None and not isinstance(start, _lib.DeviceArray):
            start = as_f64_vector(start, short, 'start')
        op = self._device_operator()
        opT = op.T                                           # (as the least-squares solvers obtain it)
        self.transposed = nrows < ncols
        tall, wide = (opT, op) if self.transposed else (op, opT)
        with DeviceRun(tall, _lib.MK_TRSVD, start, None, transpose=wide, abstol=float(self.abstol), reltol=float(self.reltol),
                       matvec_max=int(matvec_max), reorth=1 if reorth == 'full' else 0,
                       eig=(nsv, ncv, 1 if which == 'LM' else 0, keep, int(seed))) as run:
            res = run.run()
            record = run.vector(2 * nsv).reshape(nsv, 3)
            have = int(np.sum(record[:, 0] >= 0.0))
            right = np.stack([run.vector(i) for i in range(have)]) if have else np.zeros((0, tall.shape[1]))
            left = np.stack([run.vector(nsv + i) for i in range(have)]) if have else np.zeros((0, tall.shape[0]))
            hist = run.history()
        steps = int(res.itn)
        products_t = int(res.nMatvec) - steps                # (every step begins with a product by the tall operator)
        tall._nMatvec += steps
        if wide is not tall:
            wide._nMatvec += products_t
        else:
            tall._nMatvec += products_t
        self.s = record[:have, 0].copy()
        self.U, self.V = (right, left) if self.transposed else (left, right)
        self.residNorms = record[:have, 1].copy()
        self.pairIters = record[:have, 2].astype(np.int64)
        self.residHistory = list(hist)
        self.residNorm0 = np.float64(res.residNorm0)
        self.residNorm = np.float64(res.residNorm)
        self.anorm = np.float64(res.Anorm)
        self.threshold = np.float64(res.threshold)
        self.nMatvec = int(res.nMatvec)
        self.nIter = steps
        self.cycles = int(res.aux[0])
        self.ncv = int(res.aux[1])
        self.keep = int(res.aux[2])
        self.workspace_bytes = int(res.aux[3])
        self.nconv = int(res.aux[4])
        self.breakdown = int(res.aux[5])
        self.reorth = 'full' if int(res.aux[6]) else 'one-sided'
        self.rotation_ms = float(res.aux[7])
        self.sweeps = int(res.istop)
        self.converged = bool(res.converged)
        self.bestSolution = self.x = self.V[0] if have else None
        if self._logging():
            self.logger.info('Threshold = %8.2e' % res.threshold)
            self.logger.info('%6d  %8.2e  (%d cycles, %d of %d triplets converged)' % (self.nMatvec, self.residNorm, self.cycles,
                                                                                       self.nconv, nsv))
        return res


def svds(A, k=6, which='LM', ncv=None, tol=1e-10, maxiter=None, v0=None):
    """`k` extreme singular triplets of `A` in the calling convention of ``scipy.sparse.linalg.svds``: returns
    ``(U, s, Vt)`` with the left vectors in the COLUMNS of `U` (``nrows x k``) and the right vectors in the ROWS of `Vt`
    (``k x ncols``), so that ``A ~ U diag(s) Vt`` on the space they span.  `s` is DESCENDING -- SciPy returns its singular
    values in ascending order.  `tol` is the relative tolerance (``reltol``; 0 means 1e-15), `maxiter` the largest number of
    products with `A` and ``A.T`` together, `v0` the start vector (``min(A.shape)`` entries).  Raises RuntimeError when the
    triplets have not converged."""
    s = ThickRestartSVD(A, abstol=0.0, reltol=float(tol) if tol else 1e-15)
    s.solve(k, which=which, ncv=ncv, matvec_max=maxiter, start=v0)
    if not s.converged:
        raise RuntimeError('svds: %d of %d singular triplets converged in %d products' % (s.nconv, k, s.nMatvec))
    return s.U.T, s.s, s.V
