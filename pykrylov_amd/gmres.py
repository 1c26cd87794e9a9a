"""Restarted GMRES(m) with right preconditioning, the whole cycle on the device (``csrc/mk_gmres.hip``).

The reference package has no GMRES; this class follows its `KrylovMethod` protocol like the other solvers here.  The
NumPy restatement the device loop is tested against is ``tests/_gmres_ref.py``."""
import numpy as np

from . import _lib
from .generic import DeviceRun, KrylovMethod, resolve_precon

__docformat__ = 'restructuredtext'


class GMRES(KrylovMethod):
    """Restarted GMRES for general (nonsymmetric) ``A x = b``.

    An Arnoldi step orthogonalises ``A M v_j`` against the basis by classical Gram-Schmidt, twice unless ``reorth=False``,
    and updates the QR factors of the Hessenberg matrix by one Givens rotation; the estimate ``|g_{j+1}|`` is the norm of
    the true residual ``b - A x`` (right preconditioning).  After `restart` steps x is updated and the residual formed
    afresh.  On the device a step is 1 product, groups of 8 basis columns per dot / update launch and 2 small launches;
    the basis (``restart + 1`` vectors) stays in HBM.

    After `solve`: `x` / `bestSolution`, `nMatvec`, `nIter` (Arnoldi steps), `restarts`, `converged`, `residNorm`,
    `residNorm0`, `residHistory` (`residNorm0`, then one estimate per step) and `precon_route` (how the preconditioner was
    applied, in the words of ``DeviceRun.precon_kind``).
    """

    MAX_RESTART = _lib.MK_GMRES_MAX_RESTART

    def __init__(self, op, **kwargs):
        KrylovMethod.__init__(self, op, **kwargs)
        self.name = 'Restarted Generalized Minimal Residual'
        self.acronym = 'GMRES'
        self.prefix = self.acronym + ': '
        self.restarts = 0
        self.precon_route = 'none'

    def solve(self, rhs, guess=None, matvec_max=None, restart=30, reorth=True, **kwargs):
        """Solve with right-hand side `rhs` (a host array or a `DeviceArray`).

        :keywords:
            :guess:      initial guess (default 0); the product that forms its residual is counted
            :matvec_max: max. number of operator-vector products (default 2n)
            :restart:    Arnoldi steps per cycle, 1 .. 128 (default 30; clamped to n)
            :reorth:     orthogonalise twice per step (default True)
        """
        if isinstance(restart, bool) or not isinstance(restart, (int, np.integer)) or \
                not 1 <= int(restart) <= self.MAX_RESTART:
            raise ValueError('GMRES: restart must be an integer from 1 to %d, got %r' % (self.MAX_RESTART, restart))
        if getattr(self.op, 'local_size', None) is not None:
            raise NotImplementedError('GMRES: the operator is row-partitioned; GMRES is single-GPU')
        shape = getattr(self.op, 'shape', None)
        if shape is not None and len(shape) == 2 and shape[0] != shape[1]:
            raise ValueError('GMRES needs a square operator, got shape %s' % (tuple(shape),))
        op = self._device_operator()
        n = int(op.shape[0])
        route, payload = resolve_precon(self.precon, n, 'precon', 'GMRES')
        if matvec_max is None:
            matvec_max = 2 * n
        with DeviceRun(op, _lib.MK_GMRES, rhs, guess, precon_diag=payload, abstol=float(self.abstol),
                       reltol=float(self.reltol), matvec_max=int(matvec_max), restart=int(restart),
                       reorth=int(bool(reorth))) as run:
            res = run.run()
            x = run.x()
            hist = run.history()
            self.precon_route = run.precon_kind
        assert route == self.precon_route
        op._nMatvec += int(res.nMatvec)
        self.residNorm0 = np.float64(res.residNorm0)
        self.residNorm = np.float64(res.residNorm)
        self.residHistory = list(hist)
        self.nMatvec = int(res.nMatvec)
        self.nIter = int(res.itn)
        self.restarts = int(res.aux[0])
        self.last_cycle_steps = int(res.aux[1])
        self.basis_bytes = int(res.aux[2])
        self.converged = bool(res.converged)
        self.bestSolution = self.x = x
        if self._logging():
            self.logger.info('Initial residual = %8.2e' % self.residNorm0)
            self.logger.info('Threshold = %8.2e' % res.threshold)
            self.logger.info('%6d  %8.2e  (%d restarts)' % (self.nMatvec, self.residNorm, self.restarts))
        return res
