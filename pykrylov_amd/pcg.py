"""Preconditioned conjugate gradients, the whole loop on the device (``csrc/mk_pcg.hip``).

`CG` reproduces the reference's recurrence, whose search direction is built from ``r`` and not from ``precon * r``, so no
preconditioner shortens its runs.  This class is the textbook loop beside it and follows the reference's `KrylovMethod`
protocol like the other solvers here.  The NumPy restatement the device loop is tested against is ``tests/_pcg_ref.py``."""
import numpy as np

from . import _lib
from .generic import DeviceRun, KrylovMethod, resolve_precon

__docformat__ = 'restructuredtext'


class PCG(KrylovMethod):
    """Preconditioned conjugate gradients for symmetric positive definite ``A x = b`` with a symmetric positive definite
    preconditioner ``precon`` (an approximation of the inverse of ``A``): ``z = precon * r``, ``p = z + beta p``.

    Per pass 1 product and 1 preconditioner application; on the device 3 kernels without a preconditioner or with a
    diagonal one, the product, 4 small launches and the preconditioner's own otherwise.  Without a preconditioner the run
    is `CG`'s bit for bit.

    After `solve`: `x` / `bestSolution`, `nMatvec`, `nIter` (completed passes), `converged`, `definite`, `breakdown` (0 none,
    1 the curvature test ``<p, A p> > 0`` failed: `definite` is False, `x` is untouched by that pass and `infiniteDescent` is
    that ``p``; 2 a ``<r, precon * r>`` that is not positive and finite: `x` is the last iterate), `residNorm`, `residNorm0`,
    `residHistory` (this call's: 2-norms of the recurrence residual of `x`, `residNorm0` first, then one per pass),
    `precon_route` (in the words of ``DeviceRun.precon_kind``) and `flexible`.
    """

    def __init__(self, op, **kwargs):
        KrylovMethod.__init__(self, op, **kwargs)
        self.name = 'Preconditioned Conjugate Gradient'
        self.acronym = 'PCG'
        self.prefix = self.acronym + ': '
        self.definite = True
        self.breakdown = 0
        self.flexible = False
        self.infiniteDescent = None
        self.precon_route = 'none'

    def solve(self, rhs, guess=None, matvec_max=None, flexible=False, check_curvature=True, **kwargs):
        """Solve with right-hand side `rhs` (a host array or a `DeviceArray`).

        :keywords:
            :guess:           initial guess (default 0); the product that forms its residual is counted
            :matvec_max:      max. number of operator-vector products (default 2n); never exceeded
            :flexible:        ``beta = <z', r' - r> / <r, z>`` (Polak-Ribiere) instead of ``<r', z'> / <r, z>``, for a
                              preconditioner that is not the same linear operator at every call; one more inner product
                              per pass (default False)
            :check_curvature: stop on a ``<p, A p>`` that is not positive (default True)
        """
        if not isinstance(flexible, (bool, np.bool_)):
            raise ValueError('PCG: flexible must be True or False, got %r' % (flexible,))
        if getattr(self.op, 'local_size', None) is not None:
            raise NotImplementedError('PCG: the operator is row-partitioned; PCG is single-GPU')
        shape = getattr(self.op, 'shape', None)
        if shape is not None and len(shape) == 2 and shape[0] != shape[1]:
            raise ValueError('PCG needs a square operator, got shape %s' % (tuple(shape),))
        op = self._device_operator()
        n = int(op.shape[0])
        route, payload = resolve_precon(self.precon, n, 'precon', 'PCG')
        if matvec_max is None:
            matvec_max = 2 * n
        with DeviceRun(op, _lib.MK_PCG, rhs, guess, precon_diag=payload, abstol=float(self.abstol),
                       reltol=float(self.reltol), matvec_max=int(matvec_max), check_curvature=int(bool(check_curvature)),
                       pcg=(bool(flexible),)) as run:
            res = run.run()
            x = run.x()
            hist = run.history()
            self.precon_route = run.precon_kind
            self.infiniteDescent = run.vector(1) if not res.definite else None
        assert route == self.precon_route
        op._nMatvec += int(res.nMatvec)
        self.residNorm0 = np.float64(res.residNorm0)
        self.residNorm = np.float64(res.residNorm)
        self.residHistory = list(hist)
        self.nMatvec = int(res.nMatvec)
        self.nIter = int(res.itn)
        self.flexible = bool(res.aux[0])
        self.breakdown = int(res.aux[1])
        self.converged = bool(res.converged)
        self.definite = bool(res.definite)
        self.bestSolution = self.x = x
        if self._logging():
            self.logger.info('Initial residual = %8.2e' % self.residNorm0)
            self.logger.info('Threshold = %8.2e' % res.threshold)
            self.logger.info('%6d  %8.2e  (%s)' % (self.nMatvec, self.residNorm, self.precon_route))
            if not self.definite:
                self.logger.error('Coefficient operator is not positive definite')
        return res
