"""Small helpers of the solver path (reference pykrylov/tools/utils.py)."""
import ctypes
import math

import numpy as np

from . import _lib
from .linop import LinearOperator


def machine_epsilon():
    "Double-precision machine epsilon (utils.py:7-9)."
    return np.finfo(np.double).eps


def check_symmetric(op, repeats=10):
    """Cheap randomized symmetry test (utils.py:63-85): for `repeats` random x checks
    ``<Ax, Ax> == <x, A(Ax)>`` up to ``(s + eps) * eps**(1/3)``.

    Like the reference it reseeds the global NumPy RNG with 1 and draws the vectors with
    ``np.random.random`` (so traces with ``check=True`` can be compared).  For a
    :class:`CsrOperator` both products and both inner products run on the GPU; the products
    are counted in ``op.nMatvec`` as the reference does.
    """
    from .linop import CsrOperator
    op = getattr(op, 'host_op', op)                           # (solver-side shell of a matrix-free operator)
    if getattr(op, 'local_size', None) is not None:
        return _check_symmetric_partitioned(op, repeats)
    m, n = op.shape
    if m != n:
        return False
    eps = machine_epsilon()
    np.random.seed(1)
    on_device = isinstance(op, CsrOperator)
    if on_device:
        lib = _lib.init()
        dx, dw, dr = (_lib.DeviceArray(n, zero=False) for _ in range(3))
        s, t = ctypes.c_double(), ctypes.c_double()
    for _ in range(repeats):
        x = np.random.random(n)
        if on_device:
            dx.upload(x)
            op.spmv_device(dx.ptr, dw.ptr)
            op.spmv_device(dw.ptr, dr.ptr)
            _lib.check(lib.mk_dot(n, dw.ptr, dw.ptr, ctypes.byref(s)))
            _lib.check(lib.mk_dot(n, dx.ptr, dr.ptr, ctypes.byref(t)))
            sv, tv = s.value, t.value
        else:                       # an operator defined by host callables lives on the host by definition
            w = op * x
            r = op * w
            sv, tv = np.dot(w, w), np.dot(x, r)
        if abs(sv - tv) > (sv + eps) * eps ** (1.0 / 3):
            return False
    return True


def _check_symmetric_partitioned(op, repeats):
    """The same test on a row-partitioned operator (pykrylov_amd.dist): every rank draws the same global random
    vector and keeps its slice, products are preceded by the operator's exchange, inner products are summed over
    the ranks -- so all ranks reach the same verdict.  Collective: call it on every rank."""
    lib = _lib.init()
    c0, c1 = op.row_range
    n_local, n_ext, n_global = c1 - c0, op.shape[1], op.global_size
    eps = machine_epsilon()
    np.random.seed(1)
    dx, dw = _lib.DeviceArray(n_ext), _lib.DeviceArray(n_ext)
    dr = _lib.DeviceArray(n_local, zero=False)
    pair = (ctypes.c_double * 2)()
    s, t = ctypes.c_double(), ctypes.c_double()
    ok = True
    for _ in range(repeats):
        x = np.random.random(n_global)[c0:c1]
        _lib.check(lib.mk_memcpy_h2d(dx.ptr, np.ascontiguousarray(x).ctypes.data, 8 * n_local))
        _lib.check(lib.mk_exchange(op.handle, dx.ptr))
        op.spmv_device(dx.ptr, dw.ptr)                        # w = A x   (local rows, written into [0, n_local))
        _lib.check(lib.mk_exchange(op.handle, dw.ptr))
        op.spmv_device(dw.ptr, dr.ptr)                        # r = A w
        _lib.check(lib.mk_dot(n_local, dw.ptr, dw.ptr, ctypes.byref(s)))
        _lib.check(lib.mk_dot(n_local, dx.ptr, dr.ptr, ctypes.byref(t)))
        pair[0], pair[1] = s.value, t.value
        _lib.check(lib.mk_comm_allreduce_host(pair, 2))
        if abs(pair[0] - pair[1]) > (pair[0] + eps) * eps ** (1.0 / 3):
            ok = False                                        # keep going: the collectives must stay matched
    for b in (dx, dw, dr):
        b.free()
    return ok


def block_jacobi(op, block_size):
    """Block-Jacobi preconditioner of a device matrix as a DEVICE operator: the diagonal blocks of `op` (size
    `block_size`, the last one possibly smaller) are inverted once on the host (NumPy, batched) and the inverses are
    stored as a block-diagonal :class:`CsrOperator`.  Passed as ``precon=`` it is applied inside the device loop as a
    product (``precon * r``, generic/generic.py:76; mk_solver_set_precon_csr) -- no host round trip per iteration,
    unlike a general callable preconditioner.  `block_size` = 1 gives the Jacobi (diagonal) preconditioner as a matrix.
    """
    from .linop import CsrOperator
    indptr, indices, data = op.to_csr_arrays()
    n = op.shape[0]
    nloc = getattr(op, 'local_size', None)
    if nloc is not None:
        # row-partitioned operator (pykrylov_amd.dist): the RANK-LOCAL preconditioner -- blocks of this rank's diagonal
        # block only (its columns are numbered [own | received], so owned columns are those below the local size);
        # blocks never straddle ranks, the result has no exchange plan and is applied without communication
        n = int(nloc)
        if getattr(op, 'exchange_mode', 0) == 1:              # all-gather layout: column = n_local + GLOBAL column
            c0 = int(op.row_range[0])
            indices = indices.astype(np.int64) - n - c0       # owned columns -> 0 .. n-1, everything else outside
            own = (indices >= 0) & (indices < n)
        else:
            own = indices < n
        rows_all = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
        counts = np.bincount(rows_all[own], minlength=n)
        indices, data = indices[own], data[own]
        indptr = np.concatenate([[0], np.cumsum(counts)])
    elif op.shape[0] != op.shape[1]:
        raise ValueError('block_jacobi needs a square operator')
    bs = int(block_size)
    if bs < 1:
        raise ValueError('block_size must be positive')
    nb = (n + bs - 1) // bs
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = indices.astype(np.int64)
    inblk = (rows // bs) == (cols // bs)
    blocks = np.zeros((nb, bs, bs))
    blocks[rows[inblk] // bs, rows[inblk] % bs, cols[inblk] % bs] = data[inblk]
    tail = n - (nb - 1) * bs
    if tail < bs:                                            # pad the last block with an identity corner
        k = np.arange(tail, bs)
        blocks[nb - 1, k, k] = 1.0
    inv = np.linalg.inv(blocks)
    # block-diagonal CSR of the inverses (dense blocks; the padding of the last block is dropped)
    r = np.repeat(np.arange(nb * bs, dtype=np.int64), bs)
    c = (r // bs) * bs + np.tile(np.arange(bs, dtype=np.int64), nb * bs)
    v = inv.reshape(-1)
    keep = (r < n) & (c < n)
    r, c, v = r[keep], c[keep], v[keep]
    ip = np.zeros(n + 1, dtype=np.int64)
    ip[1:] = np.cumsum(np.bincount(r, minlength=n))
    return CsrOperator(ip, c, v, (n, n), symmetric=bool(getattr(op, 'symmetric', False)))


def _device_matrix(op, what, noun, symmetric=True, factor=False):
    """Kind / shape checks of the matrix a device object is made from (`ilu0`, `ic0`, `chebyshev`, `lanczos`, `fsai`,
    `amg`), made before the device is touched; `noun` names what is single-GPU.  The order of the two groups is each
    caller's own and stays as it was: a row-partitioned operator is not square (its columns are [own | received]), so
    `ilu0` / `ic0` (`factor`) say ValueError "square" of it and the others NotImplementedError "row-partitioned";
    tests/test_ilu_cpu.py pins the first order on an object that is no CsrOperator either."""
    shape = getattr(op, 'shape', None)
    if shape is None or len(shape) != 2:
        raise TypeError('%s needs an operator with a `.shape`; got %r' % (what, type(op).__name__))

    def shaped():
        if shape[0] != shape[1]:
            raise ValueError('%s needs a square operator, got shape %s' % (what, (shape,)))
        if symmetric and not getattr(op, 'symmetric', False):
            raise ValueError('%s needs a symmetric operator (declared with symmetric=True)' % what)

    def placed():
        from .linop import CsrOperator
        if getattr(op, 'local_size', None) is not None:
            raise NotImplementedError('%s: the operator is row-partitioned; %s%s single-GPU%s' % (
                what, noun, ' are' if factor else ' is', ' (rank-local factors are not available)' if factor else ''))
        if not isinstance(op, CsrOperator):
            raise TypeError('%s: %r holds no CSR arrays on the device; form its matrix (e.g. `to_csr_arrays()` of a device '
                            'operator) and wrap it in a CsrOperator%s' % (what, type(op).__name__,
                                                                         ' to factor it' if factor else ''))
    for check in ((shaped, placed) if factor else (placed, shaped)):
        check()
    return op


def _checked_int(what, name, v, lo, hi, must=None):
    """`v` as an int if it is an integer (no bool) from `lo` to `hi`; ValueError naming `what` and `name` otherwise."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError('%s: %s must be %s, got %r' % (what, name, must or 'an integer from %d to %d' % (lo, hi), v))
    return int(v)


class DevicePreconditioner(LinearOperator):
    """What the device preconditioner objects of this module share: a handle of libmikrylov.so whose entry points are
    ``mk_<_abi>_apply`` / ``_info`` / ``_destroy``.  ``self * v`` applies the object to a NumPy vector,
    `apply_device` to DeviceArray vectors; a solver given it as ``precon=`` (``M=`` / ``N=``) applies it on the device
    (``mk_solver_set_precon_<route>``, `generic.PRECON_SETTERS`).  `free()` releases this object's reference; a solver
    that still applies the object keeps it alive.  A kind gives the class attributes below, creates its handle and ends
    its constructor with `_attach`."""

    route = None            # the word of `generic.resolve_precon`
    plural = None           # '... are single-GPU'
    _noun = None            # '... has been freed'
    _abi = None             # the stem of mk_<stem>_apply / _info / _destroy
    _info_names = ()
    _handle = _buf = _op = None

    def _attach(self, handle, n, symmetric, op=None):
        """`op`: the matrix the object was made from, where its Python owner has to stay alive beside the library's count."""
        self._lib = _lib.init()
        self._handle, self._n, self._op = handle, int(n), op
        LinearOperator.__init__(self, self._n, self._n, matvec=self._apply, symmetric=symmetric, dtype=np.float64)

    def _live(self):
        if not self._handle:
            raise ValueError('%s has been freed' % self._noun)
        return self._handle

    handle = property(lambda self: self._live(), doc="The opaque handle for libmikrylov; ValueError once freed.")

    def _call(self, entry, *args):
        h = self._live()
        _lib.check(getattr(self._lib, 'mk_%s_%s' % (self._abi, entry))(h, *args))

    def _read_info(self, names, *level):
        cap = getattr(_lib, 'MK_%s_INFO_LEN' % self._abi.upper())
        v = (ctypes.c_int64 * cap)()
        self._call('info', *(level + (v, cap)))
        return dict(zip(names, (int(x) for x in v)))

    info = property(lambda self: self._read_info(self._info_names), doc="``mk_<kind>_info`` as a dict.")

    def _times_vector(self, x):
        self._live()                                         # (a freed object says so before anything else)
        return LinearOperator._times_vector(self, x)

    def _apply(self, r):
        self._live()
        if self._buf is None:
            self._buf = _lib.DeviceArray(self._n, zero=False)
        self._buf.upload(np.ascontiguousarray(r, dtype=np.float64))
        self._call('apply', self._buf.ptr, self._buf.ptr)
        return self._buf.to_numpy()

    def apply_device(self, d_in, d_out):
        "``d_out = self * d_in`` on DeviceArray vectors (`d_in is d_out` allowed); enqueued on the library's stream."
        self._live()
        for d in (d_in, d_out):
            if not isinstance(d, _lib.DeviceArray) or d.n != self._n or d.dtype != np.float64 or not d.ptr:
                raise ValueError('apply_device needs live float64 DeviceArray vectors of %d entries' % self._n)
        self._call('apply', d_in.ptr, d_out.ptr)

    def free(self):
        if self._buf is not None:
            self._buf.free()
            self._buf = None
        if self._handle:
            try:
                getattr(self._lib, 'mk_%s_destroy' % self._abi)(self._handle)
            except Exception:
                pass
            self._handle = None
        self._op = None

    def __del__(self):
        self.free()


def ilu0(op):
    """ILU(0) of a square device matrix (a :class:`CsrOperator`) as a DEVICE preconditioner: the factor is computed on the
    GPU on the pattern of `op` (every row must store its diagonal), and ``precon * r`` -- inside a solver's loop or on a
    NumPy vector -- is the pair of level-scheduled triangular solves ``U^-1 L^-1 r`` (mk_ilu_apply).  Passed as
    ``precon=`` to CG / BiCGSTAB / CGS / TFQMR / MINRES / SYMMLQ it is applied at the reference's preconditioner sites
    without a host round trip.  Raises MkError on a zero pivot (naming the row)."""
    _device_matrix(op, 'ilu0', 'the incomplete factorizations', symmetric=False, factor=True)
    return IluPreconditioner(op, 0)


def ic0(op):
    """IC(0) (incomplete Cholesky, no fill) of a symmetric device matrix: ``M = L L^T`` on the lower pattern of `op`, as a
    symmetric device preconditioner like :func:`ilu0` (MINRES' symmetry check of the preconditioner passes).  Raises
    ValueError for an operator not declared symmetric, MkError for a pattern that is not symmetric or a pivot that is not
    positive (naming the row)."""
    _device_matrix(op, 'ic0', 'the incomplete factorizations', factor=True)
    return IluPreconditioner(op, 1)


class IluPreconditioner(DevicePreconditioner):
    """M^-1 of an ILU(0) / IC(0) factor resident in HBM (`ilu0`, `ic0`), a :class:`DevicePreconditioner`.  Attributes: `kind`
    ('ilu0' / 'ic0'), `levels` and `launches` (forward, backward sweep), `info` (mk_ilu_info as a dict)."""

    route, plural, _noun, _abi = 'ilu', 'incomplete factorizations', 'the factor', 'ilu'
    _info_names = ('kind', 'rows', 'nnz', 'levels_forward', 'levels_backward', 'launches_forward', 'launches_backward',
                   'widest_level', 'bytes', 'fuse_rows', 'analysis_us', 'factor_us')

    def __init__(self, op, kind):
        lib = _lib.init()
        h = ctypes.c_void_p()
        fn = lib.mk_ic0_create if kind else lib.mk_ilu0_create
        _lib.check(fn(op.handle, ctypes.byref(h)))
        self._nnz = int(op.nnz)
        self.kind = 'ic0' if kind else 'ilu0'
        self._attach(h.value, op.shape[0], bool(kind), op)   # (`op`: its pattern; factor_arrays() pairs it with the values)

    levels = property(lambda self: (self.info['levels_forward'], self.info['levels_backward']))
    launches = property(lambda self: (self.info['launches_forward'], self.info['launches_backward']))

    def factor_arrays(self):
        """``(indptr, indices, values, diag)``: the factor on the pattern of the operator (values as described in
        include/mikrylov.h, mk_ilu_download) and the position of each row's diagonal entry."""
        self._live()
        indptr, indices, _ = self._op.to_csr_arrays()
        vals = np.empty(self._nnz, dtype=np.float64)
        diag = np.empty(self._n, dtype=np.int32)
        self._call('download', vals.ctypes.data, diag.ctypes.data)
        return indptr, indices, vals, diag


def _lanczos_args(what, steps, seed):
    """`steps` and `seed` of `lanczos` (and of ``chebyshev(interval='lanczos')``), checked before the device is touched."""
    return (_checked_int(what, 'steps', steps, 1, 2 ** 31 - 1, 'a positive integer'),
            _checked_int(what, 'seed', seed, 0, 2 ** 64 - 1, 'an integer from 0 to 2**64 - 1'))


class LanczosResult(object):
    """What `lanczos` returns.  `alpha` (alpha_1 .. alpha_m) and `beta` (beta_1 .. beta_{m+1}; beta_1 is the norm of the
    start vector and no entry of T) as the device computed them, `steps` = m as done, `ritz` the eigenvalues of the m x m
    tridiagonal T in ascending order, ``residuals[i] = |beta_{m+1} S[m-1, i]|`` with S the eigenvectors of T (the residual
    norm of Ritz pair i), ``bounds = (ritz[0], ritz[-1] + residuals[-1])`` -- the upper end is the k-step Lanczos bound of
    Zhou and Li for the largest eigenvalue --, and `info` (steps, launches, bytes, elapsed_us, nonfinite)."""

    def __init__(self, alpha, beta, info):
        self.alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        self.beta = np.ascontiguousarray(beta, dtype=np.float64)
        self.steps = m = len(self.alpha)
        self.info = info
        # a small dense host solve, like the compact form of L-BFGS: no LAPACK in the library
        T = np.diag(self.alpha) + np.diag(self.beta[1:m], 1) + np.diag(self.beta[1:m], -1)
        self.ritz, S = np.linalg.eigh(T)
        self.residuals = np.abs(self.beta[m] * S[m - 1, :])
        self.bounds = (float(self.ritz[0]), float(self.ritz[-1] + self.residuals[-1]))

    def __repr__(self):
        return 'LanczosResult(steps=%d, bounds=(%.6g, %.6g))' % ((self.steps,) + self.bounds)


def lanczos(op, steps=10, scale_diag=False, seed=1, start=None):
    """``min(steps, n)`` steps of the symmetric Lanczos process on a symmetric device matrix (a :class:`CsrOperator` declared
    ``symmetric=True``), run ON the device (mk_csr_lanczos: the product kernel with ``<v, A v>`` fused and one stream kernel
    per step, the scalars downloaded once at the end), as a spectrum estimate: a :class:`LanczosResult` whose `bounds` are
    an interval for `chebyshev`.  ``scale_diag=True`` estimates the spectrum of ``D^-1/2 A D^-1/2`` (every row must store a
    positive diagonal entry; MkError naming the row otherwise), which is that of the ``D^-1 A`` a scaled `chebyshev` iterates
    on.  The start vector is `start` (n finite numbers) or, by default, a hashed vector of `seed` -- on purpose not a vector
    of ones, which is orthogonal to the top eigenvector of ``poisson2d(m)`` for even m.  The run stops early at a breakdown
    (`steps` then reads less than asked for: the Ritz values are eigenvalues).  No reorthogonalisation; do not go below the
    default of 10 steps for an upper bound that is to hold."""
    _device_matrix(op, 'lanczos', 'the Lanczos estimate')
    steps, seed = _lanczos_args('lanczos', steps, seed)
    n = int(op.shape[0])
    if n == 0:
        raise ValueError('lanczos: the operator has no rows')
    if start is not None:
        start = np.ascontiguousarray(start, dtype=np.float64)
        if start.shape != (n,):
            raise ValueError('lanczos: start must have %d entries, got shape %s' % (n, start.shape))
        if not np.all(np.isfinite(start)) or not np.any(start):
            raise ValueError('lanczos: start must be finite and not zero')
    lib = _lib.init()
    m = min(steps, n)
    alpha, beta = (ctypes.c_double * m)(), (ctypes.c_double * (m + 1))()
    v = (ctypes.c_int64 * _lib.MK_LANCZOS_INFO_LEN)()
    d_start = _lib.DeviceArray.from_numpy(start) if start is not None else None
    try:
        _lib.check(lib.mk_csr_lanczos(op.handle, steps, int(bool(scale_diag)), seed, d_start.ptr if d_start else None,
                                      alpha, beta, v, _lib.MK_LANCZOS_INFO_LEN))
    finally:
        if d_start is not None:
            d_start.free()
    info = dict(zip(('steps', 'launches', 'bytes', 'elapsed_us', 'nonfinite'), (int(x) for x in v)))
    done = info['steps']
    return LanczosResult(alpha[:done], beta[:done + 1], info)


def chebyshev(op, degree=4, lmin=None, lmax=None, ratio=30.0, scale_diag=False, interval='gershgorin', steps=10, seed=1):
    """Chebyshev polynomial preconditioner ``z = p_k(A) r`` of a symmetric device matrix (a :class:`CsrOperator` declared
    ``symmetric=True``) as a DEVICE preconditioner: `degree` = k steps of the Chebyshev iteration for ``A z = r`` from
    ``z = 0`` on the interval ``[lmin, lmax]`` (Saad, Alg. 12.1), each step ONE product of `op` in the storage format it has,
    with the step's vector updates fused into the product's row epilogue -- no triangular solve, no level schedule.

    `lmax` defaults to the Gershgorin bound of the matrix (computed on the device), `lmin` to ``lmax / ratio`` (30: the
    convention of hypre and Ifpack2 where no lower estimate is given).  ``scale_diag=True`` runs the iteration on
    ``D^-1 A`` (Jacobi scaling; every row must store a nonzero diagonal, MkError naming the row otherwise) -- the operator is
    then symmetric in the D inner product only.  ``1 <= degree <= 64``.  Passed as ``precon=`` to BiCGSTAB / CGS / TFQMR /
    MINRES / SYMMLQ, or as ``M=`` / ``N=`` to the least-squares solvers, it is applied without a host round trip.

    ``interval='lanczos'`` takes whichever of `lmin` and `lmax` is not given from ``lanczos(op, steps, scale_diag,
    seed).bounds`` instead -- an interval from the matrix: the smallest Ritz value, and the largest plus its residual norm (an
    under-estimated `lmax` is the dangerous end: the residual polynomial grows without bound beyond it; an over-estimated
    `lmin` leaves the preconditioner positive definite).  ValueError if the smallest Ritz value is not positive; where the
    Krylov space held one eigenvalue only, ``lmin = lmax / ratio``.  It costs `steps` products and stream passes once, and is
    not always the better interval, hence opt-in.  `interval_source` of the result names, per end, where it
    came from: ``'gershgorin'``, ``'lanczos'`` or ``'given'``."""
    _device_matrix(op, 'chebyshev', 'the Chebyshev preconditioner')
    if interval not in ('gershgorin', 'lanczos'):
        raise ValueError("chebyshev: interval must be 'gershgorin' or 'lanczos', got %r" % (interval,))
    degree = _checked_int('chebyshev', 'degree', degree, 1, _lib.MK_CHEB_MAX_DEGREE)
    for name, v in (('lmin', lmin), ('lmax', lmax)):
        if v is not None and not (np.isfinite(v) and v > 0):
            raise ValueError('chebyshev: %s must be positive and finite, got %r' % (name, v))
    if lmin is not None and lmax is not None and not lmin < lmax:
        raise ValueError('chebyshev: the interval needs 0 < lmin < lmax, got lmin = %r, lmax = %r' % (lmin, lmax))
    if lmin is None and not (np.isfinite(ratio) and ratio > 1):
        raise ValueError('chebyshev: ratio must be finite and > 1, got %r' % (ratio,))
    source = tuple(interval if v is None else 'given' for v in (lmin, lmax))
    estimate = None
    if interval == 'lanczos':
        if lmin is not None and lmax is not None:
            raise ValueError("chebyshev: interval='lanczos' with lmin and lmax both given leaves nothing to estimate")
        steps, seed = _lanczos_args('chebyshev', steps, seed)
        estimate = lanczos(op, steps, scale_diag, seed)
        if not estimate.ritz[0] > 0:
            raise ValueError('chebyshev: the smallest Ritz value of %d Lanczos steps is %r: the matrix is not positive '
                             'definite' % (estimate.steps, float(estimate.ritz[0])))
        lo, hi = estimate.bounds
        if lmax is None:
            lmax = hi
        if lmin is None:
            # (a Krylov space of one eigenvalue: no lower estimate)
            lmin = lo if lo < hi * (1.0 - 2.0 ** -26) else float(lmax) / float(ratio)
        if not lmin < lmax:
            raise ValueError('chebyshev: the interval needs 0 < lmin < lmax, got lmin = %r, lmax = %r (Lanczos bounds %r)'
                             % (lmin, lmax, (lo, hi)))
    M = ChebyshevPreconditioner(op, degree, lmin, lmax, float(ratio), bool(scale_diag))
    M.interval_source = source
    M.lanczos = estimate
    return M


class ChebyshevPreconditioner(DevicePreconditioner):
    """``p_k(A)`` of a symmetric device matrix, resident in HBM (`chebyshev`), a :class:`DevicePreconditioner`.  Attributes:
    `degree`, `interval` (``(lmin, lmax)`` as used), `interval_source` (per end ``'gershgorin'``, ``'lanczos'`` or
    ``'given'``), `lanczos` (the :class:`LanczosResult` behind ``interval='lanczos'``, else None), `coefficients` (``c0`` and
    the arrays ``c1``, ``c2`` of the steps), `scaled`, `info` (mk_cheb_info as a dict)."""

    route, plural, _noun, _abi = 'cheb', 'Chebyshev preconditioners', 'the Chebyshev preconditioner', 'cheb'
    _info_names = ('rows', 'degree', 'scaled', 'launches', 'bytes', 'setup_us', 'lmin_default', 'lmax_default')

    def __init__(self, op, degree, lmin, lmax, ratio, scale_diag):
        lib = self._lib = _lib.init()
        self.degree = int(degree)
        self.scaled = bool(scale_diag)
        self.interval_source = tuple('gershgorin' if v is None else 'given' for v in (lmin, lmax))
        self.lanczos = None
        if lmin is None and lmax is not None:
            lmin = float(lmax) / ratio
        elif lmin is None and ratio != 30.0:
            # lmin = (default lmax) / ratio: the Gershgorin bound first, from an object of degree 1
            probe = self._create(op, 1, 0.0, 0.0)
            try:
                lmin = self._coefficients(probe, 1)[1] / ratio
            finally:
                lib.mk_cheb_destroy(probe)
        h = self._create(op, self.degree, 0.0 if lmin is None else float(lmin), 0.0 if lmax is None else float(lmax))
        self._attach(h, op.shape[0], True, op)

    def _create(self, op, degree, lmin, lmax):
        h = ctypes.c_void_p()
        _lib.check(self._lib.mk_cheb_create(op.handle, degree, lmin, lmax, int(self.scaled), ctypes.byref(h)))
        return h.value

    def _coefficients(self, handle, degree):
        v = (ctypes.c_double * (3 + 2 * degree))()
        _lib.check(self._lib.mk_cheb_coefficients(handle, v))
        return np.array(v[:], dtype=np.float64)

    @property
    def interval(self):
        "``(lmin, lmax)`` as used."
        c = self._coefficients(self._live(), self.degree)
        return float(c[0]), float(c[1])

    @property
    def coefficients(self):
        "``(c0, c1, c2)``: the scalar of the first direction and the two coefficient arrays of the steps 1 .. degree."
        c = self._coefficients(self._live(), self.degree)
        return float(c[2]), c[3::2].copy(), c[4::2].copy()


def _filter_end(what, name, v):
    "An end of a filter's interval: None (the Gershgorin end, NaN for the library) or a finite number."
    if v is None:
        return float('nan')
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError('%s: %s must be None (the Gershgorin end) or a finite number, got %r' % (what, name, v))
    return float(v)


def cheb_filter(op, degree=16, interval=(None, None), ref=None):
    """The scaled Chebyshev filter ``y = rho(A) x`` of Zhou and Saad for a symmetric device matrix (a :class:`CsrOperator`
    declared ``symmetric=True``), resident on the device: the spectral transformation of :class:`ThickRestartLanczos`
    (``solve(..., filter=F)``).  ``interval = (a, b)`` is the UNWANTED part of the spectrum and `ref` = a0 a reference point
    strictly outside it on the wanted side (``a0 < a``: the smallest eigenvalues are wanted, ``a0 > b``: the largest);
    ``rho(t) = T_d((t - c)/e) / T_d((a0 - c)/e)`` with ``e = (b - a)/2``, ``c = (b + a)/2``, ``d = degree`` (1 .. 128) is
    below ``1 / T_d((a0 - c)/e)`` in modulus on ``[a, b]`` and grows monotonically beyond the end `ref` lies at.  An end
    given as None is the Gershgorin end of the matrix, computed on the device.  An apply is `degree` products of `op` in the
    storage format it has, the vector work fused into the product's row epilogue.

    An eigenvalue of `A` inside ``[a, b]`` is damped, not found: `interval` must leave the wanted eigenvalues outside
    (:func:`cheb_filter_for` chooses an interval that does)."""
    _device_matrix(op, 'cheb_filter', 'the Chebyshev filter')
    degree = _checked_int('cheb_filter', 'degree', degree, 1, _lib.MK_FILTER_MAX_DEGREE)
    try:
        a, b = interval
    except (TypeError, ValueError):
        raise ValueError('cheb_filter: interval must be a pair (a, b), got %r' % (interval,))
    a, b = _filter_end('cheb_filter', 'interval[0]', a), _filter_end('cheb_filter', 'interval[1]', b)
    if ref is None or np.isnan(_filter_end('cheb_filter', 'ref', ref)):
        raise ValueError('cheb_filter: ref (the reference point a0 on the wanted side of the interval) must be given')
    ref = float(ref)
    if a >= b:
        raise ValueError('cheb_filter: the interval needs a < b, got %r' % ((a, b),))
    if a <= ref <= b:
        raise ValueError('cheb_filter: ref = %r lies inside the unwanted interval %r; it must lie strictly outside, on the '
                         'wanted side' % (ref, (a, b)))
    return ChebyshevFilter(op, degree, a, b, ref)


FILTER_RANGE = 2.0 ** 16   # largest T_d(z0) `cheb_filter_for` allows: see `cheb_filter_degree_cap`


def cheb_filter_degree_cap(a, b, a0):
    """The largest degree d with ``T_d(z0) <= 2**16``, ``z0 = |a0 - c| / e`` (at least 1).  A wanted eigenvalue may lie anywhere
    between `a0` and the cut, where ``rho`` falls from 1 to ``1 / T_d(z0)``.  Lanczos on ``B = rho(A)`` resolves an
    eigenvector of B to about ``eps |B|`` absolutely, so the residual on `A` of a pair whose ``rho`` is ``1 / T_d(z0)`` cannot
    be brought below about ``eps T_d(z0) |A|``: with ``T_d(z0) <= 2**16`` that floor is ``2**-36``, about 1.5e-11, one decade
    below the eigensolver's default ``reltol``.  (Beyond ``2**26`` such a pair is invisible altogether: the recurrence's
    breakdown test is ``beta <= 2**-26 tmax``.)  A bound from the arithmetic, not a tuned number; it binds where the wanted
    end is well separated, which is where a filter has little to offer anyway."""
    z0 = abs(float(a0) - 0.5 * (float(b) + float(a))) / (0.5 * (float(b) - float(a)))
    return max(1, int(math.acosh(FILTER_RANGE) / math.acosh(z0)))


def cheb_filter_for(op, nev, which='SA', degree=16, steps=None, seed=1):
    """A :func:`cheb_filter` for the `nev` smallest (``'SA'``) or largest (``'LA'``) eigenvalues of `op`, its interval chosen
    from a pilot run ``lanczos(op, steps=steps or default_ncv(n, nev), seed=seed)``.  For ``'SA'``, with `ritz` ascending and
    zero-based: ``a = ritz[nev]``, `b` the Gershgorin upper end, ``a0 = ritz[0] - residuals[0]``; ``'LA'`` is the mirror
    (``b = ritz[-1 - nev]``, `a` the Gershgorin lower end, ``a0 = ritz[-1] + residuals[-1]``).  By Cauchy interlacing
    ``ritz[i] >= lambda_i``, so the cut never lies below the (nev+1)-th eigenvalue: the wanted eigenvalues stay outside the
    damped interval whatever the pilot run found.  That is a guarantee, not a tuned number, and it is loose: a tighter
    ``interval=`` of :func:`cheb_filter`, from a rough first solve, converges in fewer steps.  ValueError if the pilot run
    gives fewer than ``nev + 1`` Ritz values or `a0` falls inside the interval.  `degree` is an upper limit: the object's
    `degree` is ``min(degree, cheb_filter_degree_cap(a, b, a0))``, so that no wanted eigenvalue is damped beyond what the
    eigensolver's tolerance can recover.  The object records the pilot run's products as `pilotMatvec` (and the run itself as
    `pilot`)."""
    from .trlan import default_ncv
    _device_matrix(op, 'cheb_filter_for', 'the Chebyshev filter')
    if which not in ('SA', 'LA'):
        raise ValueError("cheb_filter_for: which must be 'SA' or 'LA', got %r" % (which,))
    n = int(op.shape[0])
    nev = _checked_int('cheb_filter_for', 'nev', nev, 1, max(n - 1, 1))
    degree = _checked_int('cheb_filter_for', 'degree', degree, 1, _lib.MK_FILTER_MAX_DEGREE)
    pilot = lanczos(op, steps=default_ncv(n, nev) if steps is None else steps, seed=seed)
    if len(pilot.ritz) < nev + 1:
        raise ValueError('cheb_filter_for: the pilot run gave %d Ritz values, %d are needed for the cut behind the %d wanted '
                         'eigenvalues (more steps, or a breakdown: the matrix has few distinct eigenvalues)'
                         % (len(pilot.ritz), nev + 1, nev))
    if which == 'SA':
        interval, ref = (float(pilot.ritz[nev]), None), float(pilot.ritz[0] - pilot.residuals[0])
    else:
        interval, ref = (None, float(pilot.ritz[-1 - nev])), float(pilot.ritz[-1] + pilot.residuals[-1])
    cut = interval[0] if which == 'SA' else interval[1]
    if (which == 'SA' and not ref < cut) or (which == 'LA' and not ref > cut):
        raise ValueError('cheb_filter_for: the reference point %r does not lie on the wanted side of the cut %r (the pilot '
                         "run's extreme Ritz values coincide)" % (ref, cut))
    try:
        probe = cheb_filter(op, 1, interval, ref)            # (resolves the Gershgorin end)
        try:
            interval = probe.interval
        finally:
            probe.free()
        F = cheb_filter(op, min(degree, cheb_filter_degree_cap(interval[0], interval[1], ref)), interval, ref)
    except _lib.MkError as err:                              # (a0 inside once the Gershgorin end is known, a < b violated)
        raise ValueError('cheb_filter_for: %s' % err)
    F.pilot = pilot
    F.pilotMatvec = int(pilot.steps)
    return F


class ChebyshevFilter(LinearOperator):
    """``rho(A)`` of a symmetric device matrix, resident in HBM (`cheb_filter`, `cheb_filter_for`): ``F * v`` on a NumPy
    vector, `apply_device` on DeviceArray vectors (the input is not modified), ``filter=F`` of :class:`ThickRestartLanczos`.
    The C ABI has no function for it: the object is a thick-restart Lanczos solver handle created with the block
    ``mk_params_filter`` in its probe mode (``restart = 1``), whose set-up applies the filter.  Attributes: `degree`,
    `interval` (``(a, b)`` as used), `ref`, `side` (``'SA'`` / ``'LA'``: the end `ref` lies at), `coefficients` (``c``,
    ``e`` and the arrays ``p``, ``q`` of the steps), `pilotMatvec` (products of the pilot run that chose the interval; 0 for a
    given one), `info` (a dict), `free()`.  It is no preconditioner: as ``precon=`` it would be applied through the host
    like any operator."""

    _info_names = ('rows', 'degree', 'side', 'launches', 'bytes', 'setup_us', 'a_default', 'b_default')

    def __init__(self, op, degree, a, b, ref):
        from .generic import DeviceRun
        self._lib = _lib.init()
        self.degree = int(degree)
        self.pilot, self.pilotMatvec = None, 0
        self._op, self._n = op, int(op.shape[0])
        self._in = self._out = None
        self._run = DeviceRun(op, _lib.MK_TRLAN, None, abstol=0.0, reltol=0.0, matvec_max=1, restart=1,
                              eig=(1, 2, 0, 0, 1), filter=(self.degree, a, b, ref))
        try:
            self._table = self._run.vector(2)                # (nev + 1: the filter's table)
        except Exception:
            self._run.close()
            raise
        LinearOperator.__init__(self, self._n, self._n, matvec=self._apply, symmetric=True, dtype=np.float64)

    def _live(self):
        if self._run is None:
            raise ValueError('the Chebyshev filter has been freed')
        return self._run

    interval = property(lambda self: (float(self._table[0]), float(self._table[1])), doc="``(a, b)`` as used.")
    ref = property(lambda self: float(self._table[2]), doc="The reference point a0.")
    side = property(lambda self: 'LA' if self._table[2] > self._table[1] else 'SA',
                    doc="``'SA'`` if `ref` lies below the interval (the smallest eigenvalues are wanted), ``'LA'`` if above.")

    @property
    def coefficients(self):
        "``(c, e, p, q)``: the centre and the half width of the interval and the coefficient arrays of the steps 1 .. degree."
        t = self._table[:5 + 2 * self.degree]
        return float(t[3]), float(t[4]), t[5::2].copy(), t[6::2].copy()

    @property
    def info(self):
        "rows, degree, side (0 / 1), launches per apply, device bytes held, set-up time (us), whether a / b is Gershgorin's."
        return dict(zip(self._info_names, (int(v) for v in self._table[5 + 2 * self.degree:])))

    def _times_vector(self, x):
        self._live()                                         # (a freed object says so before anything else)
        return LinearOperator._times_vector(self, x)

    def _probe(self, ptr):
        "The solver's set-up applies the filter to the vector at `ptr`; returns the device pointer of the result."
        run = self._live()
        _lib.check(self._lib.mk_solver_setup(run.handle, ptr, None))
        out = ctypes.c_void_p()
        _lib.check(self._lib.mk_solver_x(run.handle, ctypes.byref(out)))
        return out.value

    def _apply(self, r):
        self._live()
        if self._in is None:
            self._in = _lib.DeviceArray(self._n, zero=False)
        self._in.upload(np.ascontiguousarray(r, dtype=np.float64))
        return _lib.download(self._probe(self._in.ptr), self._n)

    def apply_device(self, d_in, d_out):
        "``d_out = self * d_in`` on DeviceArray vectors (`d_in is d_out` allowed: the result is formed in the object's own vector)."
        self._live()
        for d in (d_in, d_out):
            if not isinstance(d, _lib.DeviceArray) or d.n != self._n or d.dtype != np.float64 or not d.ptr:
                raise ValueError('apply_device needs live float64 DeviceArray vectors of %d entries' % self._n)
        _lib.check(self._lib.mk_memcpy_d2d(d_out.ptr, self._probe(d_in.ptr), 8 * self._n))

    def free(self):
        if getattr(self, '_in', None) is not None:
            self._in.free()
            self._in = None
        if getattr(self, '_run', None) is not None:
            self._run.close()
            self._run = None
        self._op = None

    def __del__(self):
        self.free()


def _pattern_power(indptr, indices, n, power):
    """``(indptr, indices)`` of the lower triangle of the pattern of ``A**power`` (`power` >= 2), the symbolic product formed
    on the host with NumPy: the pairs (i, k) with k in row j of A for every (i, j) held so far, made unique by sorting
    their keys ``i * n + k``.  Rows come out sorted."""
    indptr = np.asarray(indptr, dtype=np.int64)
    cols = np.asarray(indices, dtype=np.int64)
    length = np.diff(indptr)
    bi, bj = np.repeat(np.arange(n, dtype=np.int64), length), cols
    for step in range(power - 1):
        cnt = length[bj]
        first = np.cumsum(cnt) - cnt
        pos = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(first, cnt) + np.repeat(indptr[bj], cnt)
        ii, kk = np.repeat(bi, cnt), cols[pos]
        if step == power - 2:                                # (the last product: only the lower triangle is wanted)
            low = kk <= ii
            ii, kk = ii[low], kk[low]
        key = np.unique(ii * n + kk)
        bi, bj = key // n, key % n
    ip = np.zeros(n + 1, dtype=np.int64)
    ip[1:] = np.cumsum(np.bincount(bi, minlength=n))
    return ip, bj


def fsai(op, power=1, pattern=None):
    """FSAI preconditioner (factorized sparse approximate inverse, Kolotilina and Yeremin) of a symmetric positive definite
    device matrix (a :class:`CsrOperator` declared ``symmetric=True``) as a DEVICE preconditioner: for ``A ~ L L^T`` a sparse
    lower-triangular ``G ~ L^-1`` on a fixed pattern, computed on the GPU by one small dense SPD solve per row (all rows
    independent: no level schedule), and ``M^-1 = G^T G`` -- an apply is two sparse products through the library's product
    kernels and storage formats.

    The pattern of G is the lower triangle of the pattern of ``A**power``, `power` = 1 (the default: the stored lower triangle
    of `op`, extracted on the device), 2 or 3.  For ``power > 1`` the symbolic product is a HOST set-up step: it is formed
    with NumPy from ``op.to_csr_arrays()``, once (a device symbolic product is not available).  ``pattern=(indptr,
    indices)`` gives the pattern explicitly instead (lower triangular, every row sorted, without duplicates and ending with
    its diagonal entry); it excludes ``power != 1``.  No row of the pattern may hold more than 32 entries: ValueError naming
    the row otherwise.  Passed as ``precon=`` to CG / BiCGSTAB / CGS / TFQMR / MINRES / SYMMLQ / GMRES, or as ``M=`` / ``N=``
    to the least-squares solvers, it is applied without a host round trip.  Raises MkError naming the row for a pattern that
    is not as described, a row without a stored diagonal entry and a breakdown (the matrix is not positive definite)."""
    _device_matrix(op, 'fsai', 'the FSAI preconditioner')
    power = _checked_int('fsai', 'power', power, 1, 3, '1, 2 or 3')
    n = int(op.shape[0])
    if pattern is not None:
        if power != 1:
            raise ValueError('fsai: give either `pattern` or `power`, not both (got power = %d with a pattern)' % power)
        try:
            ip, ix = pattern
        except (TypeError, ValueError):
            raise ValueError('fsai: pattern must be a pair (indptr, indices)')
        ip, ix = np.asarray(ip), np.asarray(ix)
        if ip.ndim != 1 or ix.ndim != 1 or ip.dtype.kind not in 'iu' or ix.dtype.kind not in 'iu':
            raise ValueError('fsai: pattern must be a pair of 1-D integer arrays (indptr, indices)')
        if ip.shape != (n + 1,) or int(ip[0]) != 0 or int(ip[-1]) != ix.size or ix.size >= 2 ** 31:
            raise ValueError('fsai: pattern indptr must have %d entries, start at 0 and end at len(indices) = %d'
                             % (n + 1, ix.size))
        if ix.size and not (0 <= int(ix.min()) and int(ix.max()) < n):
            raise ValueError('fsai: pattern indices must lie in 0 .. %d' % (n - 1))
    elif power > 1:
        indptr, indices, _ = op.to_csr_arrays()
        ip, ix = _pattern_power(indptr, indices, n, power)
    if pattern is not None or power > 1:
        length = np.diff(ip)
        if length.size and int(length.max()) > _lib.MK_FSAI_MAX_ROW:
            row = int(np.argmax(length > _lib.MK_FSAI_MAX_ROW))
            raise ValueError('fsai: row %d of the pattern has %d entries, more than %d: lower `power` (or give a sparser '
                             '`pattern`)' % (row, int(length[row]), _lib.MK_FSAI_MAX_ROW))
        pattern = (np.ascontiguousarray(ip, dtype=np.int32), np.ascontiguousarray(ix, dtype=np.int32))
    return FsaiPreconditioner(op, power, pattern)


class FsaiPreconditioner(DevicePreconditioner):
    """``G^T G`` of an FSAI factor resident in HBM (`fsai`), a :class:`DevicePreconditioner`.  Attributes: `power`, `info`
    (mk_fsai_info as a dict).  `factor_arrays()` downloads G.  The object does not keep the matrix it was computed from."""

    route, plural, _noun, _abi = 'fsai', 'FSAI preconditioners', 'the FSAI preconditioner', 'fsai'
    _info_names = ('rows', 'nnz', 'longest_row', 'launches', 'bytes', 'format_g', 'format_gt', 'setup_us')

    def __init__(self, op, power=1, pattern=None):
        lib = _lib.init()
        self.power = int(power)
        h = ctypes.c_void_p()
        ip, ix = (None, None) if pattern is None else pattern
        rc = lib.mk_fsai_create(op.handle, None if ip is None else ip.ctypes.data, None if ix is None else ix.ctypes.data,
                                ctypes.byref(h))
        if rc != 0:
            msg = lib.mk_last_error().decode(errors='replace')
            if 'more than MK_FSAI_MAX_ROW' in msg:           # (the pattern came from the device: power = 1)
                raise ValueError('fsai: %s: lower `power` (or give a sparser `pattern`)' % msg.split(': ', 1)[-1])
            _lib.check(rc)
        self._attach(h.value, op.shape[0], True)

    def factor_arrays(self):
        "``(indptr, indices, values)`` of G: lower triangular CSR, every row ending with its diagonal entry."
        nnz = self.info['nnz']
        indptr = np.empty(self._n + 1, dtype=np.int32)
        indices = np.empty(nnz, dtype=np.int32)
        values = np.empty(nnz, dtype=np.float64)
        self._call('download', indptr.ctypes.data, indices.ctypes.data, values.ctypes.data)
        return indptr, indices, values

    def factor_handles(self):
        """Borrowed ``mk_csr*`` handles of G and of its transpose, for ``mk_csr_set_format`` / ``mk_csr_format_info``; they
        belong to this object."""
        g, gt = ctypes.c_void_p(), ctypes.c_void_p()
        self._call('factors', ctypes.byref(g), ctypes.byref(gt))
        return g.value, gt.value


def _amg_real(name, v, ok, what):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not ok(float(v)):
        raise ValueError('amg: %s must be a finite number %s, got %r' % (name, what, v))
    return float(v)


def amg(op, theta=0.0, degree=1, ratio=4.0, omega=4.0 / 3.0, coarse_max=256, max_levels=10, seed=1, expand_cap=0):
    """Smoothed-aggregation algebraic multigrid of a symmetric device matrix with a positive diagonal (a :class:`CsrOperator`
    declared ``symmetric=True``) as a DEVICE preconditioner whose apply is one V(1,1)-cycle.  The hierarchy is set up on the
    GPU: per level the strength graph (`theta`; ``v*v > theta**2 * a_ii * a_jj``), MIS(2) roots from hashed keys (`seed`),
    aggregates, the prolongator ``P = T - (omega / lmax) D^-1 A T`` with `lmax` the Gershgorin bound of ``D^-1 A``, and the
    Galerkin product ``P^T (A P)`` as two expand-sort-compress products in row chunks of at most `expand_cap` expanded
    entries (0: 2**26; the hierarchy does not depend on it).  Coarsening stops at `coarse_max` rows (1 .. 1024), at
    `max_levels` levels (1 .. 16) or when a level does not shrink; a last level of at most `coarse_max` rows is inverted on
    the host and applied as a dense matrix, a larger one (or one whose Cholesky factorization breaks down) is solved by its
    smoother alone.  The smoother of every level is the diagonally scaled Chebyshev polynomial of `degree` on
    ``[lmax / ratio, lmax]`` (`chebyshev`).  Passed as ``precon=`` to CG / BiCGSTAB / CGS / TFQMR / MINRES / SYMMLQ / GMRES /
    IDR, or as ``M=`` / ``N=`` to the least-squares solvers, it is applied without a host round trip.  ValueError naming the
    row for a diagonal entry that is missing, zero or negative (on any level)."""
    _device_matrix(op, 'amg', 'the AMG preconditioner')
    theta = _amg_real('theta', theta, lambda v: v >= 0.0, '>= 0')
    ratio = _amg_real('ratio', ratio, lambda v: v > 1.0, '> 1')
    omega = _amg_real('omega', omega, lambda v: v > 0.0, '> 0')
    degree = _checked_int('amg', 'degree', degree, 1, _lib.MK_CHEB_MAX_DEGREE)
    coarse_max = _checked_int('amg', 'coarse_max', coarse_max, 1, _lib.MK_AMG_MAX_COARSE)
    max_levels = _checked_int('amg', 'max_levels', max_levels, 1, _lib.MK_AMG_MAX_LEVELS)
    seed = _checked_int('amg', 'seed', seed, 0, 2 ** 64 - 1)
    expand_cap = _checked_int('amg', 'expand_cap', expand_cap, 0, 2 ** 31 - 1)
    return AmgPreconditioner(op, theta, degree, ratio, omega, coarse_max, max_levels, seed, expand_cap)


class AmgPreconditioner(DevicePreconditioner):
    """One V(1,1)-cycle of a smoothed-aggregation hierarchy resident in HBM (`amg`), a :class:`DevicePreconditioner`.
    Attributes: `info` (the totals of mk_amg_info as a dict), `levels` (one dict per level), `operator_complexity`,
    `grid_complexity`; `level_arrays(l)` downloads a level, `coarse_inverse()` the dense inverse of the last one,
    `level_handles(l)` gives the borrowed ``mk_csr*`` of a level."""

    route, plural, _noun, _abi = 'amg', 'AMG preconditioners', 'the AMG preconditioner', 'amg'
    _info_names = ('levels', 'bytes', 'setup_us', 'launches', 'coarse_dense', 'operator_complexity_x1000',
                   'grid_complexity_x1000', 'nnz_total', 'rows_total', 'coarse_why')

    def __init__(self, op, theta, degree, ratio, omega, coarse_max, max_levels, seed, expand_cap):
        lib = _lib.init()
        self.params = dict(theta=theta, degree=degree, ratio=ratio, omega=omega, coarse_max=coarse_max,
                           max_levels=max_levels, seed=seed, expand_cap=expand_cap)
        h = ctypes.c_void_p()
        rc = lib.mk_amg_create(op.handle, theta, degree, ratio, omega, coarse_max, max_levels, seed, expand_cap, ctypes.byref(h))
        if rc != 0:
            msg = lib.mk_last_error().decode(errors='replace')
            if 'has no positive diagonal entry' in msg:
                raise ValueError('amg: %s' % msg.split(': ', 1)[-1])
            _lib.check(rc)
        self._attach(h.value, op.shape[0], True, op)

    def _info(self, level, names):
        "mk_amg_info takes a level: -1 the totals, else the level's figures."
        return self._read_info(names, level)

    @property
    def info(self):
        d = self._info(-1, self._info_names)
        d['coarse_solver'] = 'inverse' if d['coarse_dense'] else 'smoother'
        return d

    @property
    def levels(self):
        names = ('rows', 'nnz', 'nnz_p', 'aggregates', 'mis_rounds', 'expanded_ap', 'expanded_rap', 'chunks_ap', 'chunks_rap',
                 'chunks_p')
        out = []
        for l in range(self.info['levels']):
            d = self._info(l, names)
            lmax = ctypes.c_double()
            self._call('download', l, None, ctypes.byref(lmax))
            d['lmax'] = lmax.value
            out.append(d)
        return out

    @property
    def operator_complexity(self):
        i = self.info
        return i['nnz_total'] / float(self._info(0, ('rows', 'nnz'))['nnz'] or 1)

    @property
    def grid_complexity(self):
        return self.info['rows_total'] / float(self._n or 1)

    def level_handles(self, level):
        """Borrowed ``mk_csr*`` handles ``(A_l, P, R)`` of a level, for ``mk_csr_set_format`` / ``mk_csr_format_info``; P and R
        are None on the last level.  They belong to this object."""
        out = []
        last = level == self.info['levels'] - 1
        for which in range(3):
            if which and last:
                out.append(None)
                continue
            h = ctypes.c_void_p()
            self._call('level', level, which, ctypes.byref(h))
            out.append(h.value)
        return tuple(out)

    def _csr_arrays(self, handle):
        nr, nc, nnz = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self._lib.mk_csr_shape(handle, ctypes.byref(nr), ctypes.byref(nc), ctypes.byref(nnz)))
        indptr = np.empty(nr.value + 1, dtype=np.int32)
        indices = np.empty(nnz.value, dtype=np.int32)
        data = np.empty(nnz.value, dtype=np.float64)
        _lib.check(self._lib.mk_csr_download(handle, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data))
        return indptr, indices, data, (nr.value, nc.value)

    def level_arrays(self, level):
        """A level to the host as a dict: ``'A'``, ``'P'``, ``'R'`` as ``(indptr, indices, data, shape)``, ``'agg'`` and
        ``'lmax'``; P, R and agg are None on the last level."""
        a, p, r = self.level_handles(level)
        out = {'A': self._csr_arrays(a), 'P': None, 'R': None, 'agg': None}
        lmax = ctypes.c_double()
        if p is not None:
            out['P'], out['R'] = self._csr_arrays(p), self._csr_arrays(r)
            agg = np.empty(out['A'][3][0], dtype=np.int32)
            self._call('download', level, agg.ctypes.data, ctypes.byref(lmax))
            out['agg'] = agg
        else:
            self._call('download', level, None, ctypes.byref(lmax))
        out['lmax'] = lmax.value
        return out

    def coarse_inverse(self):
        "The dense inverse of the last level (row major), or None when that level is solved by its smoother alone."
        if not self.info['coarse_dense']:
            return None
        n = self._info(self.info['levels'] - 1, ('rows',))['rows']
        inv = np.empty((n, n), dtype=np.float64)
        self._call('coarse', inv.ctypes.data)
        return inv
