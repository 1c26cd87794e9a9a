"""IDR(s) with right preconditioning, the whole cycle on the device (``csrc/mk_idr.hip``).

The reference package has no IDR(s); this class follows its `KrylovMethod` protocol like the other solvers here.  The
NumPy restatement the device loop is tested against is ``tests/_idr_ref.py``."""
import numpy as np

from . import _lib
from .generic import DeviceRun, KrylovMethod, resolve_precon

__docformat__ = 'restructuredtext'


class IDR(KrylovMethod):
    """IDR(s) of Sonneveld and van Gijzen for general (nonsymmetric) ``A x = b``, in the biorthogonal form.

    Short recurrences over ``3 s`` stored vectors (the shadow vectors P and the blocks G and U) and no restart: a cycle is
    `s` inner steps and one dimension-reduction step, one product each.  ``s = 1`` is mathematically Bi-CGSTAB; ``s`` of 4
    to 8 usually comes close to full GMRES in products.  The preconditioner is applied on the right, so the recurrence
    residual is that of ``x`` itself.  On the device an inner step is 1 product, groups of 8 columns per combination / dot /
    update launch and 2 small launches.

    After `solve`: `x` / `bestSolution`, `nMatvec`, `nIter` (inner steps plus dimension-reduction steps), `cycles`,
    `converged`, `breakdown` (0 none, 1 a zero or non-finite pivot, 2 a zero or non-finite omega; `x` is the last iterate),
    `residNorm`, `residNorm0`, `residHistory` (`residNorm0`, then one norm per product after the guess's), `precon_route`
    (in the words of ``DeviceRun.precon_kind``), `s` (the value in use) and `workspace_bytes` (P, G and U).
    """

    MAX_S = _lib.MK_IDR_MAX_S

    def __init__(self, op, **kwargs):
        KrylovMethod.__init__(self, op, **kwargs)
        self.name = 'Induced Dimension Reduction'
        self.acronym = 'IDR'
        self.prefix = self.acronym + ': '
        self.cycles = 0
        self.breakdown = 0
        self.s = None
        self.workspace_bytes = 0
        self.precon_route = 'none'

    def solve(self, rhs, guess=None, matvec_max=None, s=4, seed=1, shadow=None, **kwargs):
        """Solve with right-hand side `rhs` (a host array or a `DeviceArray`).

        :keywords:
            :guess:      initial guess (default 0); the product that forms its residual is counted
            :matvec_max: max. number of operator-vector products (default 2n); never exceeded
            :s:          shadow vectors, 1 .. 32 (default 4; clamped to n)
            :seed:       row k of P is the hashed field of ``seed + k`` with entries in [-0.5, 0.5) (default 1)
            :shadow:     the caller's P instead, an array of shape ``(s, n)``; not orthonormalised
        """
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 1 <= int(s) <= self.MAX_S:
            raise ValueError('IDR: s must be an integer from 1 to %d, got %r' % (self.MAX_S, s))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64 - self.MAX_S:
            raise ValueError('IDR: seed must be a non-negative integer below 2**64 - %d, got %r' % (self.MAX_S, seed))
        if getattr(self.op, 'local_size', None) is not None:
            raise NotImplementedError('IDR: the operator is row-partitioned; IDR is single-GPU')
        shape = getattr(self.op, 'shape', None)
        if shape is not None and len(shape) == 2 and shape[0] != shape[1]:
            raise ValueError('IDR needs a square operator, got shape %s' % (tuple(shape),))
        if shadow is not None:
            shadow = np.asarray(shadow)
            if shadow.dtype.kind == 'c':
                raise TypeError('IDR: shadow: complex data is not supported on the device path (fp64 only)')
            want = (int(s), int(shape[1])) if shape is not None else (int(s),) + shadow.shape[1:]
            if shadow.ndim != 2 or shadow.shape != want or want[0] > want[1]:
                raise ValueError('IDR: shadow has shape %s, expected (s, n) = %s with s <= n' % (shadow.shape, want))
            shadow = np.ascontiguousarray(shadow, dtype=np.float64)
        op = self._device_operator()
        n = int(op.shape[0])
        route, payload = resolve_precon(self.precon, n, 'precon', 'IDR')
        if matvec_max is None:
            matvec_max = 2 * n
        with DeviceRun(op, _lib.MK_IDR, rhs, guess, precon_diag=payload, abstol=float(self.abstol),
                       reltol=float(self.reltol), matvec_max=int(matvec_max), idr=(int(s), int(seed), shadow)) as run:
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
        self.s = int(res.aux[0])
        self.cycles = int(res.aux[1])
        self.workspace_bytes = int(res.aux[2])
        self.breakdown = int(res.aux[3])
        self.converged = bool(res.converged)
        self.bestSolution = self.x = x
        if self._logging():
            self.logger.info('Initial residual = %8.2e' % self.residNorm0)
            self.logger.info('Threshold = %8.2e' % res.threshold)
            self.logger.info('%6d  %8.2e  (s = %d, %d cycles)' % (self.nMatvec, self.residNorm, self.s, self.cycles))
        return res
