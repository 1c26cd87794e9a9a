"""`KrylovMethod`: the solver protocol of pykrylov (reference pykrylov/generic/generic.py:11-98),
plus the glue every device-resident solver of this package shares.

A solver object keeps pykrylov's constructor keywords (`abstol`, `reltol`, `precon`,
`logger`; unknown keywords are ignored as in generic.py:74-77) and result attributes.
`solve()` hands the whole loop to `libmikrylov.so`.  With a :class:`pykrylov_amd.linop.CsrOperator` (matrix
resident in HBM) the products run on the device too; any other operator of the reference's protocol
(``op * vector``) is called back on the host at each product site while the rest of the loop stays on the device
(:class:`pykrylov_amd.linop.HostOperatorShell`).  There is no host implementation of the loops in this package.
"""
import ctypes
import logging
import os
import time

import numpy as np

from . import _lib

__docformat__ = 'restructuredtext'

null_log = logging.getLogger('krylov')
null_log.setLevel(logging.INFO)
null_log.addHandler(logging.NullHandler())


class KrylovMethod(object):
    """Template of all Krylov solvers (generic.py:11-98).

    :parameters:
        :op:  the operator; ``y = op * x`` is the product with the coefficient matrix.

    :keywords:
        :abstol:  absolute stopping tolerance (default 1.0e-8)
        :reltol:  relative stopping tolerance (default 1.0e-6)
        :precon:  optional preconditioner
        :logger:  a `logging.Logger` (default: a null logger)
    """

    def __init__(self, op, **kwargs):
        self.prefix = 'Generic: '
        self.name = 'Generic Krylov Method (must be subclassed)'
        self.op = op
        self.abstol = kwargs.get('abstol', 1.0e-8)
        self.reltol = kwargs.get('reltol', 1.0e-6)
        self.precon = kwargs.get('precon', None)
        self.logger = kwargs.get('logger', null_log)
        self.residNorm = None
        self.residNorm0 = None
        self.residHistory = []
        self.nMatvec = 0
        self.nIter = 0
        self.converged = False
        self.bestSolution = None
        self.x = self.bestSolution

    def _write(self, msg):
        self.logger.info(msg)

    def solve(self, rhs, **kwargs):
        raise NotImplementedError('This method must be subclassed')

    # ------------------------------------------------------------------ device glue
    def _device_operator(self):
        """The operator as the device loop sees it: a CsrOperator (matrix in HBM, products on the device) or, for
        any other operator of the reference's protocol, a shell whose products call back into it on the host
        (the loop itself -- dots, updates, recurrences, stopping tests -- stays on the device either way)."""
        from .linop import CsrOperator, HostOperatorShell
        if isinstance(self.op, CsrOperator):
            return self.op
        view = getattr(self.op, '_device_view', None)        # block operators whose blocks all live on the device
        if view is not None:
            dev = view()
            if dev is not None:
                return dev
        sh = getattr(self, '_host_shell', None)
        if sh is None or sh.host_op is not self.op:
            if not hasattr(self.op, 'shape') or not hasattr(self.op, '__mul__'):
                raise TypeError('%s needs an operator with `.shape` and `op * vector`; got %r'
                                % (self.__class__.__name__, type(self.op).__name__))
            sh = self._host_shell = HostOperatorShell(self.op)
        return sh

    def _device_precon(self, precon):
        """How the device loop applies ``precon * r`` (generic.py:76; cg.py:91-92, bicgstab.py:96-99, ...): the payload of
        :func:`resolve_precon` -- ``None``, an fp64 array (a diagonal), the device object itself, a
        :class:`DevicePrecon` or a :class:`HostPrecon`."""
        part = getattr(self.op, 'local_size', None)
        return resolve_precon(precon, part or self.op.shape[0], 'precon', self.__class__.__name__, part is not None)[1]

    def _logging(self):
        return self.logger is not null_log and self.logger.isEnabledFor(logging.INFO)


class DevicePrecon(object):
    """A preconditioner that is itself a device operator (a CsrOperator, or a block operator with a device view): the
    loop evaluates ``precon * r`` as a product on the device (mk_solver_set_precon_csr) -- no host round trip."""

    def __init__(self, precon, dev):
        self.precon, self.dev = precon, dev

    def apply(self, r):
        return self.dev * r


class HostPrecon(object):
    """A general preconditioner for the device loop, evaluated on the host through a callback.  A square solver's
    ``precon`` is applied as the reference's loops do, ``precon * r`` (``precon(r)`` if it has no ``__mul__``); M and N of
    the least-squares solvers (`call_first`) as theirs do, ``P(v)`` (``P * v`` if it is not callable: lsqr.py:190,202)."""

    def __init__(self, precon, call_first=False):
        self.precon = precon
        self.call_first = call_first
        self.error = None
        self.calls = 0

    def apply(self, r):
        p = self.precon
        if self.call_first:
            return p(r) if callable(p) else p * r
        return p * r if hasattr(p, '__mul__') else p(r)

    def thunk(self, n):
        """The C callback on vectors of `n` entries.  What the preconditioner raises must not propagate through the C
        frames: the first exception is kept in `error` for the caller (DeviceRun._check) to re-raise."""
        def as_vector(ptr):
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_double)), shape=(n,))

        def call(user, rp, yp):
            try:
                y = np.asarray(self.apply(as_vector(rp).copy()))
                if y.shape != (n,):
                    raise ValueError('the preconditioner returned shape %s, expected (%d,)' % (y.shape, n))
                as_vector(yp)[:] = y
                self.calls += 1
                return 0
            except BaseException as exc:                    # noqa: B902
                if self.error is None:                      # (keep the root cause, not a follow-up failure)
                    self.error = exc
                return 1
        return _lib.PRECON_FN(call)


# Route word of `resolve_precon` -> the suffixes of the C setters ``mk_solver_set_precon_<square>`` and
# ``mk_solver_set_lls_precon_<lls>`` that attach it (include/mikrylov.h).  The two-sided setters of a diagonal and of a
# callback take M and N in one call: `DeviceRun._apply_precon`.
PRECON_SETTERS = {
    'diag': ('diag', ''),
    'host': ('callback', 'callback'),
    'device': ('csr', 'csr'),
    'ilu': ('ilu', 'ilu'),
    'lbfgs': ('lbfgs', 'bfgs'),
    'cheb': ('cheb', 'cheb'),
    'fsai': ('fsai', 'fsai'),
    'amg': ('amg', 'amg'),
}


def precon_setter(route, lls=False):
    "The name of the C setter of a route word, of a square or of a least-squares solver."
    suffix = PRECON_SETTERS[route][int(lls)]
    return ('mk_solver_set_lls_precon' if lls else 'mk_solver_set_precon') + ('_' + suffix if suffix else '')


def _device_object_route(precon):
    """The route word of a preconditioner that is a device object of the library, and its plural for messages: what its
    class says (`tools.DevicePreconditioner`, `lbfgs.InverseLBFGSOperator`; None on the forward L-BFGS classes, which are
    not preconditioners and stay on the host-callback route)."""
    cls = type(precon)
    return getattr(cls, 'route', None), getattr(cls, 'plural', None)


def resolve_precon(precon, size, name, owner, partitioned=False):
    """How a device loop applies a preconditioner to vectors of `size` entries: ``precon`` of a square solver
    (``precon * r``: cg.py:91-92, bicgstab.py:96-99, ...) and M / N of a least-squares solver (`u = M(Mu)`, `v = N(Nv)`:
    lsqr.py:190,202,254,266).  `name` ('precon', 'M', 'N') and `owner` (the solver's class name) go into the messages;
    `partitioned`: the solver's operator is row-partitioned.  Returns ``(route, payload)``, the route in the words of
    ``DeviceRun.precon_kind``:

    * ``'none'``, ``None``;
    * ``'diag'``: an operator that exposes its diagonal (``DiagonalOperator``, linop.py:473-516 -- the docs' Jacobi
      `DiagonalPrec`, examples/bmark.py:14-23) -- the fp64 array, applied INSIDE the kernels;
    * ``'ilu'`` / ``'lbfgs'`` / ``'cheb'`` / ``'fsai'`` / ``'amg'``: a device object of the library -- itself, applied ON the device by its own
      launches;
    * ``'device'``: a CsrOperator, or an operator with a device view (`tools.block_jacobi`, block operators of device
      matrices), square and of that size -- a :class:`DevicePrecon`, a product on the device;
    * ``'host'``: anything else that can be applied to a vector -- a :class:`HostPrecon`: the loop stays on the device and
      calls it back on the host at each preconditioner site."""
    if precon is None:
        return 'none', None

    def check_shape(shape):
        if tuple(shape) != (size, size):
            raise ValueError('%s: %s has shape %s, expected %s' % (owner, name, tuple(shape), (size, size)))
    diag = getattr(precon, 'diag', None)
    if diag is not None and not callable(diag):
        return 'diag', as_f64_vector(diag, size, name + '.diag')
    route, plural = _device_object_route(precon)
    if route is not None:
        if partitioned:
            raise NotImplementedError('%s: %s are single-GPU; the operator is row-partitioned' % (owner, plural))
        check_shape(precon.shape)
        return route, precon
    from .linop import CsrOperator
    dev = precon if isinstance(precon, CsrOperator) else None
    if dev is None and hasattr(precon, '_device_view'):
        dev = precon._device_view()
    if dev is not None and getattr(dev, 'local_size', None) is None:
        check_shape(dev.shape)
        return 'device', DevicePrecon(precon, dev)
    if not hasattr(precon, '__mul__') and not callable(precon):
        raise TypeError('%s: %s must support `%s * vector` or be callable; got %r'
                        % (owner, name, name, type(precon).__name__))
    if partitioned:
        raise NotImplementedError('%s: on a row-partitioned operator a preconditioner must be rank local and live on '
                                  'the device: a DiagonalOperator slice, or a device matrix / composite of the local '
                                  'size (e.g. pykrylov_amd.tools.block_jacobi(op, bs) of the partitioned operator); '
                                  'host callables are not called back across ranks' % owner)
    return 'host', HostPrecon(precon, call_first=name != 'precon')


def as_f64_vector(v, n, what):
    a = np.asarray(v)
    if a.dtype.kind == 'c':
        raise TypeError('%s: complex data is not supported on the device path (fp64 only)' % what)
    if a.shape != (n,):
        raise ValueError('%s has shape %s, expected (%d,)' % (what, a.shape, n))
    return np.ascontiguousarray(a, dtype=np.float64)


class DeviceRun(object):
    """One solve on the device: owns the ``mk_solver`` handle and the rhs / guess buffers."""

    def __init__(self, op, kind, rhs, guess=None, precon_diag=None, **params):
        self.lib = _lib.init()
        self.op = op
        self.precon_kind, self.precon, self.sides = 'none', None, None
        # `transpose`: the device operator A.T the least-squares kinds need (mk_solver_set_transpose); their rhs has
        # nrows(A) entries.  `sides`: their M and N, a pair of `resolve_precon` payloads.  `placement_draws`: see _draws().
        # `idr`: (s, seed, shadow) of mk_solver_set_idr, the shadow vectors None or an (s, n) fp64 array.
        # `pcg`: (flexible,) of mk_solver_set_pcg.
        # `shifts`: the shifts of multi-shift CG; they travel in the long parameter block (mk_params_shifts), whose head
        # is the mk_params every kind takes.
        # `eig`: (nev, ncv, which, keep, seed) of thick-restart Lanczos, in the second long block (mk_params_eig).  For that
        # kind `rhs` is the start vector and may be None (the hashed one).  LOBPCG (MK_LOBPCG) takes the same block with the
        # block size in `ncv`; its `rhs` is the start block, ncv * n doubles, vector after vector, or None.  The thick-restart
        # SVD (MK_TRSVD) takes the block too, with `transpose`; its `rhs` is the start vector of ncols(A) entries, or None.
        transpose = params.pop('transpose', None)
        sides = params.pop('sides', None)
        draws = params.pop('placement_draws', None)
        self.idr = params.pop('idr', None)
        self.pcg = params.pop('pcg', None)
        shifts = params.pop('shifts', None)
        eig = params.pop('eig', None)
        # `filter`: (degree, a, b, a0) of the Chebyshev filter of thick-restart Lanczos, the tail of the third long block
        # (mk_params_filter) behind `eig`; an end of [a, b] that is None or NaN is the Gershgorin end.  With `restart=1` the
        # run is the filter's probe: set-up applies the filter to `rhs`, `x()` is the result.
        self.filter = params.pop('filter', None)
        # `ring_cap`: (cap, set-ups) of CG's ring of directions, the tail of the fourth long block (mk_params_ring).
        ring_cap = params.pop('ring_cap', None)
        self._d_shadow = None
        if draws is not None:
            self.placement_draws = int(draws)
        n = getattr(op, 'local_size', None) or (op.shape[0] if transpose is not None else op.shape[1])
        if kind == _lib.MK_TRSVD:                            # (its start vector lives in the short space: ncols(A) entries)
            n = op.shape[1]
        self.n = n                                           # entries of rhs / guess
        #  entries of the solution: ncols(A) for the least-squares kinds (CRAIG-MR's lives in m-space)
        self.n_x = n if (transpose is None or kind == _lib.MK_CRAIGMR) else op.shape[1]
        # rhs / guess: host arrays (copied to HBM) or DeviceArray objects already resident there
        self._borrowed = [b for b in (rhs, guess) if isinstance(b, _lib.DeviceArray)]
        n_rhs = n * int(eig[1]) if kind == _lib.MK_LOBPCG else n
        if rhs is None and kind in (_lib.MK_TRLAN, _lib.MK_LOBPCG, _lib.MK_TRSVD):
            self.d_rhs = None
        else:
            self.d_rhs = rhs if isinstance(rhs, _lib.DeviceArray) else \
                _lib.DeviceArray.from_numpy(as_f64_vector(rhs, n_rhs, 'rhs'))
        self.d_guess = None if guess is None else (
            guess if isinstance(guess, _lib.DeviceArray) else
            _lib.DeviceArray.from_numpy(as_f64_vector(guess, n, 'guess')))
        if (self.d_rhs is not None and self.d_rhs.n != n_rhs) or (self.d_guess is not None and self.d_guess.n != n):
            raise ValueError('rhs / guess must have %d entries' % n if n_rhs == n else
                             'the start block must have %d entries' % n_rhs)
        if eig is not None and self.filter is not None:
            block = self._block = _lib.MkParamsFilter()
            block.eig.nev, block.eig.ncv, block.eig.which, block.eig.keep, block.eig.seed = [int(v) for v in eig]
            block.degree = int(self.filter[0])
            block.a, block.b, block.a0 = [float('nan') if v is None else float(v) for v in self.filter[1:]]
            p = block.eig.base                               # (a view: it writes into the block and keeps it alive)
            p.struct_size = ctypes.sizeof(_lib.MkParamsFilter)
        elif eig is not None:
            block = _lib.MkParamsEig()
            block.nev, block.ncv, block.which, block.keep, block.seed = [int(v) for v in eig]
            p = block.base                                   # (a view: it writes into the block and keeps it alive)
            p.struct_size = ctypes.sizeof(_lib.MkParamsEig)
        elif ring_cap is not None:
            block = self._block = _lib.MkParamsRing()
            block.xdefer_cap, block.xdefer_cap_setups = [int(v) for v in ring_cap]
            p = block.base                                   # (a view: it writes into the block and keeps it alive)
            p.struct_size = ctypes.sizeof(_lib.MkParamsRing)
        elif shifts is None:
            p = _lib.MkParams()
            p.struct_size = ctypes.sizeof(_lib.MkParams)
        else:
            if len(shifts) > _lib.MK_MSCG_MAX_SHIFTS:
                raise ValueError('at most %d shifts, got %d' % (_lib.MK_MSCG_MAX_SHIFTS, len(shifts)))
            block = _lib.MkParamsShifts()
            block.nsigma = len(shifts)
            for k, v in enumerate(shifts):
                block.sigma[k] = float(v)
            p = block.base                                   # (a view: it writes into the block and keeps it alive)
            p.struct_size = ctypes.sizeof(_lib.MkParamsShifts)
        p.kind = kind
        for k, v in params.items():
            setattr(p, k, v)
        self._params = p
        self.handle = ctypes.c_void_p()
        _lib.check(self.lib.mk_solver_create(op.handle, ctypes.byref(p), ctypes.byref(self.handle)))
        self.transpose = transpose
        try:                                                 # (no handle may outlive a failed constructor)
            self._borrowed += [p for p in (precon_diag,) + tuple(sides or ()) if isinstance(p, _lib.DeviceArray)]
            self.precon_kind, self.precon, self._precon_arg = self._resolve_precon(precon_diag, n)
            self.sides = None if sides is None else [self._resolve_precon(p, k) for p, k in zip(sides, op.shape)]
            if self.idr is not None and self.idr[2] is not None:
                self._d_shadow = _lib.DeviceArray.from_numpy(np.ascontiguousarray(self.idr[2], dtype=np.float64))
            self._apply_precon(self.handle)
        except Exception:
            self.lib.mk_solver_destroy(self.handle)
            self.handle = ctypes.c_void_p()
            raise
        self.result = _lib.MkResult()
        self._setup_done = False
        self.placement = {"count": 1, "chosen": 0, "per_draw_ms_per_pass": [], "probe_seconds": 0.0, "passes_per_draw": 0}

    def _resolve_precon(self, precon, n):
        """A preconditioner on vectors of `n` entries as `resolve_precon` returned it: its kind, the object this run keeps
        for it (a diagonal: the DeviceArray, which `close` frees unless it is the caller's) and a call that gives what the
        C setter of the kind takes."""
        if precon is None:
            return 'none', None, None
        route = _device_object_route(precon)[0]
        if route is not None:
            return route, precon, precon._live
        if isinstance(precon, DevicePrecon):
            return 'device', precon, lambda: precon.dev.handle
        if isinstance(precon, HostPrecon):
            cb = precon.thunk(n)                             # (the closure keeps the thunk alive)
            return 'host', precon, lambda: cb
        # a diagonal: a DeviceArray already resident in HBM (the caller's), or a host array (copied there)
        d = precon if isinstance(precon, _lib.DeviceArray) else \
            _lib.DeviceArray.from_numpy(as_f64_vector(precon, n, 'precon.diag'))
        return 'diag', d, lambda: d.ptr

    def _slots(self):
        """(kind, kept object) of every preconditioner of this run: the square solver's, then M and N."""
        return [(self.precon_kind, self.precon)] + [(kind, p) for kind, p, _ in self.sides or ()]

    def _check(self, rc):
        if rc != 0 and hasattr(self.op, 'raise_pending'):
            self.op.raise_pending()                           # what a matrix-free operator raised in its callback
        for kind, hp in self._slots():                        # ... or a host preconditioner in its
            if rc != 0 and kind == 'host' and hp.error is not None:
                err, hp.error = hp.error, None
                raise err
        _lib.check(rc)

    # Placement draws -- OPT-IN since round 4 (MK_PLACEMENT_DRAWS=k > 1, or `placement_draws=k` on the
    # DeviceRun).  How fast the fused update kernels run on a large problem depends on where the solver's vectors happen
    # to lie in HBM -- a property of the allocations, constant for their lifetime, 3-6 % of a CG pass at 512^3.  With
    # draws on, the first set-up creates k solver objects (each allocates its own vectors; spacer allocations in between
    # keep the draws apart), runs 4 + 12 real passes on each and keeps the fastest; the kept object is set up again
    # afterwards, so nothing of the probe survives but the choice.  A draw costs about 0.2 s and 4 GB (transient) at
    # 512^3 and pays back only after thousands of passes, which is why it is not the default: a solve that converges in
    # ~100 passes would get slower.  What was drawn is recorded in `self.placement`.
    # AUTOMATIC, QUICK draws (round 5) for the one class where they decide the product kernel too: CG with fused passes on a
    # brick-march matrix (formats 9 - 11) streams no matrix data to speak of, everything its kernels move lives in the solver's
    # own vectors, and about three draws in eight land in the fast state (pass 1.72 instead of 1.88 ms at 512^3,
    # profiles/r05_placement_draws_fused_march.txt).  There 6 draws of 2 + 6 passes run by themselves (about 25 ms each at
    # 512^3; all six: the states come in four levels, and stopping at the first draw that beats the first one was seen to
    # settle for a middle one) unless MK_PLACEMENT_DRAWS / `placement_draws` says otherwise (1 = off).
    def _auto_draw_class(self):
        if self._params.kind != _lib.MK_CG:
            return False
        fmt = ctypes.c_int32(0)
        try:
            _lib.check(self.lib.mk_csr_format_info(self.op.handle, ctypes.byref(fmt), None, None, None, None))
        except Exception:
            return False
        return 9 <= fmt.value <= 11

    def _draws(self):
        if self._setup_done or getattr(self, '_drawn', False):
            return 1
        want = getattr(self, 'placement_draws', None)
        self._quick_draws = False
        if want is None:
            env = os.environ.get('MK_PLACEMENT_DRAWS')
            want = int(env) if env else 0
        if want == 0:                                        # nobody asked: the automatic rule
            want, self._quick_draws = 6, True
        min_mb = float(os.environ.get('MK_PLACEMENT_MIN_MB', '256'))      # (tests lower it to draw on small problems)
        if want <= 1 or 8 * self.n <= min_mb * 1024 * 1024:
            return 1
        if getattr(self.op, 'local_size', None) is not None or 'host' in [kind for kind, _ in self._slots()]:
            return 1
        from .linop import CsrOperator
        if not isinstance(self.op, CsrOperator):             # (matrix-free shells: every pass calls back to the host)
            return 1
        if self._quick_draws and not self._auto_draw_class():
            return 1
        # the search costs about 65 passes' worth of time and buys 3-9 % per pass: it pays after about a thousand passes, so a
        # caller whose iteration budget is below that keeps the first solver object
        if self._quick_draws and 0 < int(self._params.matvec_max) < 1000:
            return 1
        return min(want, 8)

    def _apply_precon(self, handle):
        """Attach the transpose and the preconditioner(s) to a solver handle (the constructor's, and every placement
        draw's)."""
        lib = self.lib
        if self.transpose is not None:
            _lib.check(lib.mk_solver_set_transpose(handle, self.transpose.handle))
        if self.idr is not None:
            _lib.check(lib.mk_solver_set_idr(handle, int(self.idr[0]), int(self.idr[1]),
                                             None if self._d_shadow is None else self._d_shadow.ptr))
        if self.pcg is not None:
            _lib.check(lib.mk_solver_set_pcg(handle, int(bool(self.pcg[0]))))
        if self.precon_kind != 'none':
            user = (None,) if self.precon_kind == 'host' else ()
            _lib.check(getattr(lib, precon_setter(self.precon_kind))(handle, self._precon_arg(), *user))
        if self.sides is None:
            return
        # M and N: the callbacks, then the diagonals (a NULL side of these two setters leaves another kind alone), then
        # the device kinds side by side
        kinds = [kind for kind, _, _ in self.sides]
        if 'host' in kinds:
            fns = [arg() if kind == 'host' else ctypes.cast(None, _lib.PRECON_FN) for kind, _, arg in self.sides]
            _lib.check(getattr(lib, precon_setter('host', lls=True))(handle, fns[0], None, fns[1], None))
        if 'diag' in kinds:
            diags = [arg() if kind == 'diag' else None for kind, _, arg in self.sides]
            _lib.check(getattr(lib, precon_setter('diag', lls=True))(handle, *diags))
        for side, (kind, _, arg) in enumerate(self.sides):
            if kind not in ('none', 'host', 'diag'):
                _lib.check(getattr(lib, precon_setter(kind, lls=True))(handle, side, arg()))

    def _timed_passes(self, handle, warm=4, passes=12):
        g = None if self.d_guess is None else self.d_guess.ptr
        self._check(self.lib.mk_solver_setup(handle, None if self.d_rhs is None else self.d_rhs.ptr, g))
        done = ctypes.c_int64(0)
        self._check(self.lib.mk_solver_iterate(handle, warm, ctypes.byref(done)))
        self._check(self.lib.mk_sync())
        t0 = time.perf_counter()
        self._check(self.lib.mk_solver_iterate(handle, passes, ctypes.byref(done)))
        self._check(self.lib.mk_sync())
        return (time.perf_counter() - t0) / max(1, done.value) if done.value == passes else float('inf')

    PROBE_RING = (8, 1)                                      # mk_params_ring of a placement probe: m <= 8 at its first set-up

    def _probe_params(self):
        """The parameter block the objects of a placement search are created with.  CG's ring of directions takes what the
        memory rule of the library gives it (33 vectors at 512^3), and several objects are alive during the search: each
        would get a different depth and be timed at it.  So every probe's first set-up is bounded at one depth, and only the
        kept object's set-up afterwards -- the others are gone by then -- grows the ring.  A caller's own `ring_cap` stays."""
        p = self._params
        if p.kind != _lib.MK_CG or p.struct_size != ctypes.sizeof(_lib.MkParams):
            return p
        block = self._probe_block = _lib.MkParamsRing()
        ctypes.memmove(ctypes.byref(block), ctypes.byref(p), ctypes.sizeof(_lib.MkParams))
        block.base.struct_size = ctypes.sizeof(_lib.MkParamsRing)
        block.xdefer_cap, block.xdefer_cap_setups = self.PROBE_RING
        return block.base

    def _draw_placement(self, draws):
        self._drawn = True
        params = self._probe_params()
        if params is not self._params:                       # (the constructor's object has not been set up: it holds no vectors)
            h = ctypes.c_void_p()
            _lib.check(self.lib.mk_solver_create(self.op.handle, ctypes.byref(params), ctypes.byref(h)))
            try:
                self._apply_precon(h)
            except Exception:
                self.lib.mk_solver_destroy(h)
                raise
            self.lib.mk_solver_destroy(self.handle)
            self.handle = h
        spacers, best, best_t = [], self.handle, None
        t_probe = time.perf_counter()
        per_draw, chosen = [], 0
        quick = getattr(self, '_quick_draws', False)
        warm, passes = (2, 6) if quick else (4, 12)
        try:
            best_t = self._timed_passes(self.handle, warm, passes)
            per_draw.append(1e3 * best_t)
            for k in range(1, draws):
                try:
                    sp_mb = int(os.environ.get('MK_PLACEMENT_SPACER_MB', '176'))
                    spacers.append(_lib.DeviceArray(((sp_mb + (sp_mb // 2) * k) << 20) // 8 + 512 * k, zero=False))
                    h = ctypes.c_void_p()
                    _lib.check(self.lib.mk_solver_create(self.op.handle, ctypes.byref(params), ctypes.byref(h)))
                except Exception:
                    break                                     # (no memory for another draw: keep what we have)
                try:
                    self._apply_precon(h)
                    t = self._timed_passes(h, warm, passes)
                except Exception:
                    self.lib.mk_solver_destroy(h)
                    break
                per_draw.append(1e3 * t)
                if t < 0.99 * best_t:
                    self.lib.mk_solver_destroy(best)
                    best, best_t, chosen = h, t, k
                else:
                    self.lib.mk_solver_destroy(h)
        finally:
            self.handle = best
            for sp in spacers:
                sp.free()
            self.placement = {"count": len(per_draw), "chosen": chosen, "per_draw_ms_per_pass": per_draw,
                              "probe_seconds": time.perf_counter() - t_probe, "passes_per_draw": warm + passes,
                              "automatic": bool(quick)}

    def setup(self):
        draws = self._draws()
        if draws > 1:
            self._draw_placement(draws)
        self._check(self.lib.mk_solver_setup(self.handle, None if self.d_rhs is None else self.d_rhs.ptr,
                                             None if self.d_guess is None else self.d_guess.ptr))
        self._setup_done = True

    def iterate(self, max_iters):
        done = ctypes.c_int64(0)
        self._check(self.lib.mk_solver_iterate(self.handle, int(max_iters), ctypes.byref(done)))
        return done.value

    def finish(self):
        _lib.check(self.lib.mk_solver_finish(self.handle, ctypes.byref(self.result)))
        return self.result

    def run(self):
        """setup + loop until the reference's `while` condition fails + epilogue."""
        self.setup()
        res = self.finish()
        while not res.halted:
            self.iterate(1 << 20)
            res = self.finish()
        return res

    def x(self):
        p = ctypes.c_void_p()
        _lib.check(self.lib.mk_solver_x(self.handle, ctypes.byref(p)))
        return _lib.download(p.value, self.n_x)

    def unapplied(self):
        """Completed passes whose direction has not reached x yet (CG with a deferred x update: 0 after every `iterate`)."""
        c = ctypes.c_int64()
        _lib.check(self.lib.mk_solver_unapplied(self.handle, ctypes.byref(c)))
        return int(c.value)

    def vector(self, index):
        p, ln = ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(self.lib.mk_solver_vector(self.handle, index, ctypes.byref(p), ctypes.byref(ln)))
        return _lib.download(p.value, ln.value)

    def x_first(self):
        """x[0] of the current iterate (eight bytes from the device: what the reference's `show` tables print)."""
        px = ctypes.c_void_p()
        _lib.check(self.lib.mk_solver_x(self.handle, ctypes.byref(px)))
        v = ctypes.c_double()
        _lib.check(self.lib.mk_memcpy_d2h(ctypes.byref(v), px.value, 8))
        return v.value

    def history(self):
        n = int(self.result.hist_len)
        out = np.empty(n, dtype=np.float64)
        _lib.check(self.lib.mk_solver_history(self.handle, out.ctypes.data, n))
        return out

    def history2(self):
        """The second history channel (MINRES, least squares: the direct-error estimates)."""
        out = np.empty(int(self.result.hist_len), dtype=np.float64)
        _lib.check(self.lib.mk_solver_history2(self.handle, out.ctypes.data, len(out)))
        return out

    def time_product(self, which=0, launches=200):
        """Average duration (us) of the pass's product kernel `which` (0 first, 1 second / A.T), launched back to
        back without its gate and bracketed by one HIP event pair.  Destroys the loop's vectors: call it last."""
        avg = ctypes.c_double(float('nan'))
        _lib.check(self.lib.mk_solver_time_product(self.handle, int(which), int(launches), ctypes.byref(avg)))
        return avg.value

    def timing(self):
        it_ms, sp_ms, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        _lib.check(self.lib.mk_solver_timing(self.handle, ctypes.byref(it_ms), ctypes.byref(sp_ms),
                                             ctypes.byref(cnt)))
        return {"iterate_ms": it_ms.value, "spmv_ms": sp_ms.value, "spmv_launches": cnt.value}

    def close(self):
        if getattr(self, 'handle', None) is not None and self.handle.value:
            self.lib.mk_solver_destroy(self.handle)
            self.handle = ctypes.c_void_p()
        diags = [p for kind, p in self._slots() if kind == 'diag']
        for b in [self.d_rhs, self.d_guess, getattr(self, '_d_shadow', None)] + diags:
            if b is not None and not any(b is x for x in getattr(self, '_borrowed', [])):
                b.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_guess_matvec_max(solver, kind, rhs, kwargs, count_guess_product):
    """Shared body of the BiCGSTAB / CGS / TFQMR `solve` methods: keywords `guess` and `matvec_max`
    (default 2n), result attributes `converged, nMatvec, bestSolution, x, residNorm, residNorm0`
    (reference bicgstab.py:148-151, cgs.py:120-123, tfqmr.py:156-159).  These solvers keep no history."""
    op = solver._device_operator()
    pdiag = solver._device_precon(solver.precon)
    n = getattr(op, 'global_size', None) or rhs.shape[0]        # same limit on every rank of a partitioned run
    guess = kwargs.get('guess', None)
    matvec_max = kwargs.get('matvec_max', 2 * n)
    with DeviceRun(op, kind, rhs, guess, precon_diag=pdiag, abstol=float(solver.abstol),
                   reltol=float(solver.reltol), matvec_max=int(matvec_max)) as run:
        res = run.run()
        x = run.x()
    # the product that forms the initial residual from a guess is counted by the operator, but by the
    # solver only in BiCGSTAB (bicgstab.py:64-65 vs cgs.py:59-60, tfqmr.py:58-59)
    op._nMatvec += int(res.nMatvec) + (1 if (guess is not None and not count_guess_product) else 0)
    solver.residNorm0 = np.float64(res.residNorm0)
    if solver._logging():
        solver.logger.info('Initial residual = %8.2e' % solver.residNorm0)
        solver.logger.info('Threshold = %8.2e' % res.threshold)
        solver.logger.info('%6d  %8.2e' % (res.nMatvec, res.residNorm))
    solver.converged = bool(res.converged)
    solver.nMatvec = int(res.nMatvec)
    solver.bestSolution = solver.x = x
    solver.residNorm = np.float64(res.residNorm)
    return res
