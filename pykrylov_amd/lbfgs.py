"""Limited-memory BFGS operators resident in HBM (reference pykrylov/linop/lbfgs.py).

`InverseLBFGSOperator` keeps its (s, y) pairs in two device rings and applies the two-loop recursion as a chain of fused
HIP kernels (csrc/mk_lbfgs.hip); given to a solver as ``precon=`` it is applied on the device at every preconditioner
site (mk_solver_set_precon_lbfgs), with no host round trip.  `CompactLBFGSOperator` and `LBFGSOperator` are the forward
approximations: the dots against the stored columns and the combined update run on the device, the small 2p x 2p system
in between is assembled from Gram entries cached at `store` time and solved with ``np.linalg.solve``, the call the
reference makes.  `StructuredLBFGSOperator` is not provided: the reference's constructor raises TypeError
(lbfgs.py:277 passes `self` twice), so there is no behaviour to restate.
"""
import ctypes

import numpy as np

from . import _lib
from .generic import as_f64_vector
from .linop import LinearOperator

__docformat__ = 'restructuredtext'

MAX_PAIRS = 64      # MK_LBFGS_MAX_PAIRS (include/mikrylov.h)


class InverseLBFGSOperator(LinearOperator):
    """Inverse L-BFGS approximation ``H`` (lbfgs.py:14-127): ``H * v`` by the two-loop recursion, on the device.

    ``InverseLBFGSOperator(n, npairs=5, scaling=False)`` with ``1 <= npairs <= 64`` (`MAX_PAIRS`).  The reference's surface
    is kept: `npairs`, `insert`, `accept_threshold`, `ys` (``None`` marks an empty slot), `gamma`, `s` / `y` (downloaded
    as ``(n, npairs)`` arrays), `store(new_s, new_y)`, `restart()`.  In addition: `handle` (the ``mk_lbfgs*``), `info`,
    `free()`, and `store` takes :class:`pykrylov_amd._lib.DeviceArray` arguments without a host copy.  The device object
    is created on first use, so argument errors are raised without a GPU."""

    route, plural = 'lbfgs', 'L-BFGS operators'     # (generic.resolve_precon: the device loop applies the two-loop recursion)
    _use_gamma = True

    def __init__(self, n, npairs=5, **kwargs):
        scaling = kwargs.pop('scaling', False)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError('n must be an integer >= 1, got %r' % (n,))
        if isinstance(npairs, bool) or not isinstance(npairs, (int, np.integer)) or not 1 <= npairs <= MAX_PAIRS:
            raise ValueError('npairs must be an integer in 1 .. %d, got %r' % (MAX_PAIRS, npairs))
        self.n = int(n)
        self._npairs = int(npairs)
        self.scaling = bool(scaling)
        self.accept_threshold = 1.0e-20                      # lbfgs.py:51
        self.gamma = 1.0                                     # lbfgs.py:59
        self._handle = None
        self._freed = False
        self._lib = None
        self._bufs = {}
        self._insert = 0
        self._count = 0
        self._ys = [None] * self._npairs
        self._yy = [None] * self._npairs
        kwargs.pop('symmetric', None)
        LinearOperator.__init__(self, self.n, self.n, matvec=self.lbfgs_matvec, symmetric=True, **kwargs)

    # ------------------------------------------------------------------ the device object
    def _live(self):
        if self._freed:
            raise ValueError('the L-BFGS operator has been freed')
        if self._handle is None:
            lib = _lib.init()
            h = ctypes.c_void_p()
            _lib.check(lib.mk_lbfgs_create(self.n, self._npairs, int(self.scaling), ctypes.byref(h)))
            self._lib, self._handle = lib, h.value
        return self._handle

    handle = property(lambda self: self._live(), doc="Opaque ``mk_lbfgs*`` for libmikrylov.")
    npairs = property(lambda self: self._npairs, doc="The maximum number of {s, y} pairs stored.")
    insert = property(lambda self: self._insert, doc="Slot the next accepted pair goes to.")
    ys = property(lambda self: list(self._ys), doc="s_k'y_k per slot; None marks an empty slot.")

    @property
    def info(self):
        names = ('n', 'npairs', 'scaling', 'insert', 'stored', 'launches_last_apply', 'applies', 'accepted', 'rejected',
                 'bytes', 'column_stride', 'max_pairs')
        v = (ctypes.c_int64 * _lib.MK_LBFGS_INFO_LEN)()
        _lib.check(self._lib_of().mk_lbfgs_info(self._live(), v, _lib.MK_LBFGS_INFO_LEN))
        return dict(zip(names, (int(x) for x in v)))

    def _lib_of(self):
        self._live()
        return self._lib

    def _buf(self, name):
        b = self._bufs.get(name)
        if b is None:
            b = self._bufs[name] = _lib.DeviceArray(self.n, zero=False)
        return b

    def _refresh(self):
        """The host view of the ring state after a store / restart."""
        lib, h, k = self._lib_of(), self._live(), self._npairs
        v = (ctypes.c_int64 * _lib.MK_LBFGS_INFO_LEN)()
        _lib.check(lib.mk_lbfgs_info(h, v, _lib.MK_LBFGS_INFO_LEN))
        self._insert, self._count = int(v[3]), int(v[4])
        ys, yy = np.empty(k), np.empty(k)
        _lib.check(lib.mk_lbfgs_gram(h, None, None, ys.ctypes.data, yy.ctypes.data))
        self._ys = [ys[i] if i < self._count else None for i in range(k)]
        self._yy = [yy[i] if i < self._count else None for i in range(k)]

    def _rings(self):
        lib, h = self._lib_of(), self._live()
        s, y = np.empty((self._npairs, self.n)), np.empty((self._npairs, self.n))
        _lib.check(lib.mk_lbfgs_download(h, s.ctypes.data, y.ctypes.data))
        return s, y

    s = property(lambda self: np.ascontiguousarray(self._rings()[0].T), doc="The s ring, downloaded as (n, npairs).")
    y = property(lambda self: np.ascontiguousarray(self._rings()[1].T), doc="The y ring, downloaded as (n, npairs).")

    # ------------------------------------------------------------------ the reference's methods
    def _device_vector(self, v, what):
        """Device pointer of a pair member: a DeviceArray as it is, anything else checked and uploaded."""
        if isinstance(v, _lib.DeviceArray):
            if v.n != self.n or v.dtype != np.dtype(np.float64) or not v.ptr:
                raise ValueError('%s must be a live float64 DeviceArray of %d entries' % (what, self.n))
            return None, v
        return as_f64_vector(v, self.n, what), None

    def store(self, new_s, new_y):
        """Store the pair if ``new_s . new_y > accept_threshold`` (lbfgs.py:70-87); returns whether it was accepted.
        The dot is computed on the device.  Both vectors are checked before anything is written to the device."""
        if self._freed:
            raise ValueError('the L-BFGS operator has been freed')
        hs, ds = self._device_vector(new_s, 'new_s')
        hy, dy = self._device_vector(new_y, 'new_y')
        h = self._live()
        if ds is None:
            ds = self._buf('s')
            ds.upload(hs)
        if dy is None:
            dy = self._buf('y')
            dy.upload(hy)
        ok = ctypes.c_int32(0)
        _lib.check(self._lib.mk_lbfgs_store(h, ds.ptr, dy.ptr, float(self.accept_threshold), ctypes.byref(ok)))
        if ok.value:
            self._refresh()
        else:
            self.logger.debug('Rejecting (s,y) pair')
        return bool(ok.value)

    def restart(self):
        """Clear all data on past updates (lbfgs.py:89-95)."""
        _lib.check(self._lib_of().mk_lbfgs_restart(self._live()))
        self._refresh()

    def _newest_gamma(self):
        """ys / y'y of the newest pair when scaling is on and a pair is stored (lbfgs.py:116-119), else None."""
        last = (self._insert - 1) % self._npairs
        if self.scaling and self._ys[last] is not None:
            return self._ys[last] / self._yy[last]
        return None

    def _checked(self, v):
        if self._freed:
            raise ValueError('the L-BFGS operator has been freed')
        return as_f64_vector(v, self.n, 'vector')

    def _times_vector(self, x):
        self._checked(x)                                     # complex data and wrong shapes never reach the device
        return LinearOperator._times_vector(self, x)

    def lbfgs_matvec(self, v):
        """``H * v`` by the two-loop recursion (lbfgs.py:97-127): 2p + 1 fused launches for p stored pairs."""
        v = self._checked(v)
        h = self._live()
        g = self._newest_gamma()
        if g is not None:
            self.gamma = g
        d_in, d_out = self._buf('in'), self._buf('out')
        d_in.upload(v)
        _lib.check(self._lib.mk_lbfgs_apply(h, d_in.ptr, d_out.ptr))
        return d_out.to_numpy()

    def apply_device(self, d_in, d_out):
        """``out = H * in`` on DeviceArray vectors (``d_in is d_out`` allowed); nothing crosses to the host."""
        for d in (d_in, d_out):
            if not isinstance(d, _lib.DeviceArray) or d.n != self.n or d.dtype != np.dtype(np.float64) or not d.ptr:
                raise ValueError('apply_device needs live float64 DeviceArray vectors of %d entries' % self.n)
        _lib.check(self._lib_of().mk_lbfgs_apply(self._live(), d_in.ptr, d_out.ptr))

    def free(self):
        """Release this object's reference; a solver that still applies the operator keeps it alive."""
        for b in getattr(self, '_bufs', {}).values():
            b.free()
        self._bufs = {}
        if getattr(self, '_handle', None):
            try:
                self._lib.mk_lbfgs_destroy(self._handle)
            except Exception:
                pass
        self._handle = None
        self._freed = True

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class CompactLBFGSOperator(InverseLBFGSOperator):
    """Forward L-BFGS approximation ``B`` in compact form (lbfgs.py:176-254); with the same pairs it is the inverse of
    `InverseLBFGSOperator`, with `scaling` on or off.  Per product: one multi-dot pass over the 2p stored columns, a
    2p x 2p solve on the host, one combined update."""

    route = None            # no preconditioner: a solver given it calls it back on the host

    def _minimat(self, p, gamma):
        """The reference's small matrix (lbfgs.py:228-243) from the Gram entries cached when each pair was stored."""
        k = self._npairs
        ss, sy = np.empty((k, k)), np.empty((k, k))
        _lib.check(self._lib.mk_lbfgs_gram(self._live(), ss.ctypes.data, sy.ctypes.data, None, None))
        order = [(self._insert - p + i) % k for i in range(p)]            # oldest to newest
        m = np.zeros([2 * p, 2 * p])
        for ki, a in enumerate(order):
            m[p + ki, p + ki] = -self._ys[a]
            m[ki, ki] = ss[a, a] / gamma
            for li, b in enumerate(order[:ki]):
                m[ki, p + li] = sy[a, b]
                m[p + li, ki] = m[ki, p + li]
                m[ki, li] = ss[a, b] / gamma
                m[li, ki] = m[ki, li]
        return m

    def lbfgs_matvec(self, v):
        v = self._checked(v)
        h = self._live()
        lib, p = self._lib, self._count
        gamma = 1.0
        if self._use_gamma:
            g = self._newest_gamma()
            if g is not None:
                self.gamma = g
                gamma = g
        d_in, d_out = self._buf('in'), self._buf('out')
        d_in.upload(v)
        use = int(self._use_gamma)
        b = None
        if p > 0:
            a = np.empty(2 * p)
            _lib.check(lib.mk_lbfgs_forward_dots(h, d_in.ptr, use, a.ctypes.data))
            b = np.ascontiguousarray(np.linalg.solve(self._minimat(p, gamma), a))      # lbfgs.py:247
        _lib.check(lib.mk_lbfgs_forward_combine(h, d_in.ptr, use, None if b is None else b.ctypes.data, d_out.ptr))
        return d_out.to_numpy()


class LBFGSOperator(CompactLBFGSOperator):
    """Forward L-BFGS approximation ``B`` (lbfgs.py:130-173).

    The reference's outer-product form builds ``np.outer(a, a)``, an n x n array, per product, and never reads `gamma`:
    with ``scaling=True`` its ``B`` is therefore not the inverse of its ``H`` (its `CompactLBFGSOperator` is).  This class
    computes the same matrix -- the BFGS update of the identity -- through the compact machinery with ``gamma = 1``,
    whatever `scaling` says, so ``LBFGSOperator * v`` equals ``CompactLBFGSOperator(scaling=False) * v`` bit for bit and
    agrees with the reference's product to rounding."""

    _use_gamma = False
