"""NumPy restatement of the device Lanczos spectrum estimate (pykrylov_amd/csrc/mk_lanczos.hip, pykrylov_amd.tools.lanczos),
operation by operation: the start vector, the recurrence with its stop tests, and the Ritz values, residuals and bounds from
the same ``numpy.linalg.eigh`` call -- written with the oracle's CSR product and the elementwise order of the device
kernels, so that equal inputs and an equal summation order give equal bits.  Test infrastructure only."""
import numpy as np

from oracle import csr_ref, gpu_order
from tests import _cheb_ref

STOP = 2.0 ** -26          # the run stops after step j when beta_{j+1} is not > STOP * max_{i<=j}(|alpha_i| + [i>1] beta_i)


class NumpyDots(object):
    """np.dot for both inner products (the order of the CPU figures)."""

    def alfa(self, v, t):
        return float(np.dot(v, t))

    def yy(self, a, b):
        return float(np.dot(a, b))


class GpuDots(object):
    """The device's trees: <v, t> fused into the product kernel (`geometry` = gpu_order.launch_geometry(op), or the
    small-matrix rule), <r2, y> a stream kernel's."""

    def __init__(self, n, geometry=None):
        self.ntiles = (n + gpu_order.BLOCK - 1) // gpu_order.BLOCK
        self.grid, self.tile_map = geometry if geometry else (None, 1)

    def alfa(self, v, t):
        return gpu_order.total(gpu_order.spmv_partials(v, t, self.ntiles, self.grid, self.tile_map))

    def yy(self, a, b):
        return gpu_order.stream_dot(a, b)


def start_vector(n, seed):
    """The default start vector: the splitmix64 cell field less one, entries in [-0.5, 0.5)."""
    return csr_ref.cell_field(np.arange(n), seed) - 1.0


class Result(object):
    """`alpha`, `beta` (beta_1 .. beta_{m+1}), `steps`, and what tools.LanczosResult derives from them, the same way."""

    def __init__(self, alpha, beta):
        self.alpha = np.array(alpha, dtype=np.float64)
        self.beta = np.array(beta, dtype=np.float64)
        self.steps = m = len(self.alpha)
        T = np.diag(self.alpha) + np.diag(self.beta[1:m], 1) + np.diag(self.beta[1:m], -1)
        self.ritz, S = np.linalg.eigh(T)
        self.residuals = np.abs(self.beta[m] * S[m - 1, :])
        self.bounds = (float(self.ritz[0]), float(self.ritz[-1] + self.residuals[-1]))


def lanczos(A, steps=10, scale_diag=False, seed=1, start=None, dots=None, matvec=None):
    """m = min(steps, n) steps of the recurrence of mk_lanczos.hip on the oracle matrix `A`; `dots` supplies the two inner
    products (default np.dot), `matvec` the product (default the oracle's left-to-right CSR product)."""
    dots = NumpyDots() if dots is None else dots
    mv = A.matvec if matvec is None else matvec
    n = A.shape[0]
    m = min(int(steps), n)
    r2 = start_vector(n, seed) if start is None else np.array(start, dtype=np.float64)
    dinv = None
    if scale_diag:
        d = _cheb_ref.diagonal(A)
        if not np.all(d > 0):
            raise ValueError("row %d has no positive diagonal entry" % int(np.flatnonzero(~(d > 0))[0]))
        dinv = 1.0 / d
    y = dinv * r2 if scale_diag else r2
    beta = [float(np.sqrt(dots.yy(r2, y)))]
    if not (np.isfinite(beta[0]) and beta[0] > 0.0):
        raise ValueError("beta_1 = %r" % beta[0])
    alpha, tmax, r1 = [], 0.0, None
    for j in range(1, m + 1):
        b = beta[j - 1]
        s = 1.0 / b
        v = s * y
        t = mv(v)
        if j > 1:
            c = b / beta[j - 2]
            t = t - c * r1
        a = dots.alfa(v, t)
        alpha.append(a)
        if not np.isfinite(a):
            raise ValueError("alpha of step %d is not finite" % j)
        tm = abs(a)
        if j > 1:
            tm = tm + b
        tmax = max(tmax, tm)
        cc = -a / b
        ynew = cc * r2 + t
        r1, r2 = r2, ynew
        y = dinv * r2 if scale_diag else r2
        with np.errstate(invalid="ignore"):
            bn = float(np.sqrt(dots.yy(r2, y)))
        beta.append(bn)
        if not np.isfinite(bn):
            raise ValueError("beta of step %d is not finite" % j)
        if not bn > STOP * tmax:
            break
    return Result(alpha, beta)
