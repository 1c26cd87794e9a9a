"""Multi-shift conjugate gradients, the whole loop on the device (``csrc/mk_mscg.hip``).

``(A + sigma_k I) x_k = b`` for a family of shifts in the Krylov space of one (Frommer and Maass; Jegerlehner,
hep-lat/9612014): one product per pass whatever the number of shifts, two vectors per shift, and a shift that has converged
stops costing bandwidth.  The class follows the reference's `KrylovMethod` protocol like the other solvers here.  The NumPy
restatement the device loop is tested against is ``tests/_mscg_ref.py``."""
import math

import numpy as np

from . import _lib
from .generic import DeviceRun, KrylovMethod

__docformat__ = 'restructuredtext'


class ShiftedCG(KrylovMethod):
    """Conjugate gradients for ``(A + sigma_k I) x_k = b``, `A` symmetric and every ``A + sigma_k I`` positive definite
    (the caller answers for that; negative shifts are accepted).

    CG runs on `A` itself from ``x = 0``; the residual of system k stays ``zeta_k r``, so its norm ``|zeta_k| ||r||`` costs
    nothing.  With ``threshold = max(abstol, reltol ||b||)`` a shift whose norm is at most the threshold after a pass is
    frozen: its ``x_k`` has that pass's update and is not touched again.  The loop ends when every shift is frozen or at
    `matvec_max`.  There is no preconditioner and no initial guess: both destroy the collinearity of the residuals.

    After `solve`: `xs` (``nsigma x n``), `x` / `bestSolution` (``xs[0]``), `shifts`, `zeta`, `residNorms` (per shift),
    `shiftIters` (the pass at which each shift froze, -1: not converged), `nMatvec`, `nIter` (completed passes), `converged`
    (every shift), `definite`, `breakdown` (0 none, 1 the curvature test ``<p, A p> > 0`` failed: `definite` is False, nothing
    was updated in that pass and `infiniteDescent` is that ``p``; 2 a zero or non-finite term of a ``zeta`` recurrence: every
    ``x_k`` is its last iterate), `residNorm` (the largest of `residNorms`), `residNorm0`, `residHistory` (2-norms of the
    residual of the recurrence on `A`, `residNorm0` first, then one per pass), `shiftResidHistory` (per pass the largest
    ``|zeta_k| ||r||`` over the shifts active in it) and `workspace_bytes`.
    """

    def __init__(self, op, **kwargs):
        KrylovMethod.__init__(self, op, **kwargs)
        self.name = 'Multi-shift Conjugate Gradient'
        self.acronym = 'MSCG'
        self.prefix = self.acronym + ': '
        self.definite = True
        self.breakdown = 0
        self.infiniteDescent = None
        self.xs = self.shifts = self.zeta = self.residNorms = self.shiftIters = None
        self.shiftResidHistory = []
        self.workspace_bytes = 0

    def solve(self, rhs, shifts=None, guess=None, matvec_max=None, check_curvature=True, **kwargs):
        """Solve with right-hand side `rhs` (a host array or a `DeviceArray`) for every shift of `shifts`.

        :keywords:
            :shifts:          a sequence of 1 to 32 finite floats; duplicates are allowed and the order is kept
            :matvec_max:      max. number of operator-vector products (default 2n); never exceeded
            :check_curvature: stop on a ``<p, A p>`` that is not positive (default True)
        """
        if self.precon is not None:
            raise ValueError('ShiftedCG takes no preconditioner: it would destroy the collinearity of the shifted residuals')
        if guess is not None:
            raise ValueError('ShiftedCG takes no initial guess: it would destroy the collinearity of the shifted residuals')
        if shifts is None:
            raise ValueError('ShiftedCG needs shifts: a sequence of 1 to %d finite floats' % _lib.MK_MSCG_MAX_SHIFTS)
        sig = [float(s) for s in np.asarray(shifts, dtype=np.float64).reshape(-1)]
        if not 1 <= len(sig) <= _lib.MK_MSCG_MAX_SHIFTS:
            raise ValueError('ShiftedCG takes 1 to %d shifts, got %d' % (_lib.MK_MSCG_MAX_SHIFTS, len(sig)))
        if not all(math.isfinite(s) for s in sig):
            raise ValueError('ShiftedCG: every shift must be finite, got %r' % (sig,))
        if getattr(self.op, 'local_size', None) is not None:
            raise NotImplementedError('ShiftedCG: the operator is row-partitioned; multi-shift CG is single-GPU')
        shape = getattr(self.op, 'shape', None)
        if shape is not None and len(shape) == 2 and shape[0] != shape[1]:
            raise ValueError('ShiftedCG needs a square operator, got shape %s' % (tuple(shape),))
        op = self._device_operator()
        n = int(op.shape[0])
        ns = len(sig)
        if matvec_max is None:
            matvec_max = 2 * n
        with DeviceRun(op, _lib.MK_MSCG, rhs, None, abstol=float(self.abstol), reltol=float(self.reltol),
                       matvec_max=int(matvec_max), check_curvature=int(bool(check_curvature)), shifts=sig) as run:
            res = run.run()
            xs = np.stack([run.vector(2 + k) for k in range(ns)])
            record = run.vector(2 + 2 * ns).reshape(ns, 3)
            hist = run.history()
            hist2 = run.history2()
            self.infiniteDescent = run.vector(1) if not res.definite else None
        op._nMatvec += int(res.nMatvec)
        self.shifts = np.array(sig)
        self.xs = xs
        self.zeta = record[:, 0].copy()
        self.residNorms = record[:, 1].copy()
        self.shiftIters = record[:, 2].astype(np.int64)
        self.residNorm0 = np.float64(res.residNorm0)
        self.residNorm = np.float64(res.residNorm)
        self.residHistory = list(hist)
        self.shiftResidHistory = list(hist2)
        self.nMatvec = int(res.nMatvec)
        self.nIter = int(res.itn)
        self.breakdown = int(res.aux[1])
        self.workspace_bytes = int(res.aux[3])
        self.converged = bool(res.converged)
        self.definite = bool(res.definite)
        self.bestSolution = self.x = xs[0]
        if self._logging():
            self.logger.info('Initial residual = %8.2e' % self.residNorm0)
            self.logger.info('Threshold = %8.2e' % res.threshold)
            self.logger.info('%6d  %8.2e  (%d of %d shifts converged)' % (self.nMatvec, self.residNorm, int(res.aux[2]), ns))
            if not self.definite:
                self.logger.error('Coefficient operator is not positive definite')
        return res
