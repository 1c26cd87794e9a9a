"""The cases that run the device loops and preconditioners AT their documented limits (tests/test_gpu_limits.py), the table
LIMITS that says where every `MK_..._MAX...` macro of include/mikrylov.h is run at its value, and the restatement of every case,
computed once per process and left unchanged.  What the GPU tests rely on -- that a run does not end before it has met the limit:
a full first cycle, a second cycle, a third iteration, a wrapped ring, a split run -- is asserted on the restatements alone by
tests/test_limits_cpu.py, so that a wrong choice of matrix or budget fails without a GPU.  No test functions here.

The matrices that the per-solver test files do not know by name are entered into their caches here, so that their `reference`,
`rhs_of` and `solve` helpers serve these cases as they serve their own."""
import numpy as np

from oracle import csr_ref, gpu_order
from oracle.gpu_order import stream_dot
from tests import _ilu_ref as ilu_ref, _lbfgs_ref as lbfgs_ref
import test_gpu_amg as amg
import test_gpu_gmres as gm
import test_gpu_idr as idr
import test_gpu_lobpcg as lob
import test_gpu_trlan as tl
import test_gpu_trsvd as sv

# ---------------------------------------------------------------------------------------------- 1. GMRES(m)
GMRES_MATRIX = "poisson1d_301"
GMRES_RESTARTS = (127, 128)                                  # 15 groups of 8 columns and one of 7; 16 full groups
GMRES_ARGS = dict(reltol=1e-10, matvec_max=140)


def gmres_reference(restart, reorth):
    gm._MAT.setdefault(GMRES_MATRIX, csr_ref.poisson1d(301))
    return gm.reference(GMRES_MATRIX, restart=restart, reorth=reorth, **GMRES_ARGS)


# ---------------------------------------------------------------------------------------------- 2. IDR(s)
IDR_MATRIX = "poisson2d_20"
IDR_S = (31, 32)
IDR_ARGS = dict(reltol=1e-10, matvec_max=150)


def idr_reference(s):
    idr._MAT.setdefault(IDR_MATRIX, csr_ref.poisson2d(20))
    return idr.reference(IDR_MATRIX, s=s, **IDR_ARGS)


# ---------------------------------------------------------------------------------------------- 3. thick-restart Lanczos
# The first cycle takes ncv products, every later one ncv - keep, and a run makes whole cycles only: ncv + (ncv - keep) products
# are the smallest budget with a restart in it.  keep = 121 is 7 rotation launches of 16 columns and one of 9, all reading 128
# columns, the first seven into the spare columns; the second cycle's 7 steps orthogonalise against 122 .. 128 vectors, the
# last of them 16 full groups of 8.
TRLAN_MATRIX = "poisson2d_20"
TRLAN_NCV = 128
TRLAN_NEV = 4
TRLAN_KEEP = 121
TRLAN_ARGS = dict(ncv=TRLAN_NCV, keep=TRLAN_KEEP, matvec_max=TRLAN_NCV + (TRLAN_NCV - TRLAN_KEEP))


def trlan_reference(which):
    tl._MAT.setdefault(TRLAN_MATRIX, csr_ref.poisson2d(20))
    return tl.reference(TRLAN_MATRIX, TRLAN_NEV, which=which, **TRLAN_ARGS)


# ---------------------------------------------------------------------------------------------- 4. thick-restart SVD
# Two products per step.  401 x 251: both lengths odd, two workgroups on the long side.  From the small end of the spectrum: the
# largest triplets of such a matrix (and the smallest of a 301 x 151 one) all meet 1e-10 within the first 128 steps, and a run
# that has converged does not restart.
TRSVD_MATRIX = "rnd_401_251"
TRSVD_NCV = 128
TRSVD_NSV = 4
TRSVD_KEEP = 121
TRSVD_ARGS = dict(which="SM", ncv=TRSVD_NCV, keep=TRSVD_KEEP, matvec_max=2 * TRSVD_NCV + 2 * (TRSVD_NCV - TRSVD_KEEP))


def trsvd_matrix():
    return sv._MAT.setdefault(TRSVD_MATRIX, sv.rnd(401, 251, 5, 7))


def trsvd_reference(reorth, geometry=None):
    """`geometry`: the launch geometry of the tall operator's product (the one-sided mode's <u, u> is summed in it).  A grid
    of one workgroup per tile that is no multiple of 8 is what `GpuDots` assumes without one (every tile order is round robin
    then), so it is dropped: the CPU test and the GPU test share one run."""
    R = trsvd_matrix().shape[0]
    if geometry is not None and not isinstance(geometry[1], tuple) and geometry[0] % 8 != 0 and \
            geometry[0] == gpu_order.grid_spmv((R + gpu_order.BLOCK - 1) // gpu_order.BLOCK):
        geometry = None
    return sv.reference(TRSVD_MATRIX, TRSVD_NSV, geometry=geometry, reorth=reorth, **TRSVD_ARGS)


# ---------------------------------------------------------------------------------------------- 5. LOBPCG
# nev = block: block products for the start, then one per active column and iteration.  Four iterations' worth: P exists from
# the second iteration on, so the third and the fourth work on S = [X, W, P] of 3 x block columns.
LOBPCG_MATRIX = "poisson2d_20"
LOBPCG_BLOCKS = (15, 16)
_LOBPCG = {}


def lobpcg_args(block):
    return dict(which="SA", block=block, matvec_max=5 * block)


def lobpcg_reference(block):
    if block not in _LOBPCG:
        _LOBPCG[block] = lob.restate(lob.matrix(LOBPCG_MATRIX), block, **lobpcg_args(block))
    return _LOBPCG[block]


# ---------------------------------------------------------------------------------------------- 6. L-BFGS
LBFGS_N = 1001
LBFGS_NPAIRS = (9, 63, 64)
LBFGS_WRAPS = (2, 5)                                         # pairs stored beyond npairs: the ring wraps, its first slot is not 0
LBFGS_POOL = max(LBFGS_NPAIRS) + 6
_LBFGS = {}


def lbfgs_pool():
    if "pool" not in _LBFGS:
        S, Y = lbfgs_ref.make_pairs(LBFGS_N, LBFGS_POOL, 31 + LBFGS_N)
        _LBFGS["pool"] = (S, Y, np.random.default_rng(77 + LBFGS_N).standard_normal(LBFGS_N))
    return _LBFGS["pool"]


def lbfgs_ops(npairs, wrap):
    return [(lbfgs_ref.STORE, i) for i in range(npairs + wrap)]


def lbfgs_reference(npairs, scaling, wrap):
    """(the restated operator after the replay, H v, the compact B v, the compact B v with gamma = 1)."""
    key = (npairs, scaling, wrap)
    if key not in _LBFGS:
        S, Y, v = lbfgs_pool()
        R = lbfgs_ref.RefLBFGS(LBFGS_N, npairs, scaling, dot=stream_dot)
        lbfgs_ref.replay(R, lbfgs_ops(npairs, wrap), S, Y)
        _LBFGS[key] = (R, R.inverse(v), R.compact(v), R.compact(v, use_gamma=False))
    return _LBFGS[key]


# ---------------------------------------------------------------------------------------------- 7. Chebyshev
CHEB_MATRIX = "poisson2d_100"
CHEB_DEGREES = (63, 64)
FILTER_MATRIX = "poisson2d_31"
FILTER_DEGREES = (127, 128)

# ---------------------------------------------------------------------------------------------- 8. AMG
# (matrix, rows of every level): a dense coarsest level of more than one row per lane -- two, two, and exactly four.
AMG_COARSE_MAX = 1024
AMG_CASES = (("poisson2d_17", (289,)), ("poisson2d_50", (2500, 364)), ("poisson2d_32", (1024,)))


def amg_reference(name, **kw):
    return amg.reference(name, coarse_max=AMG_COARSE_MAX, **kw)


# ---------------------------------------------------------------------------------------------- 9. ILU(0) / IC(0)
ILU_RUN_MAX = 2048                                           # MK_ILU_RUN_MAX of csrc/mk_ilu.hip
ILU_FUSE_DEFAULT = 256                                       # MK_ILU_FUSE_DEFAULT
ILU_BLOCK = 256                                              # rows per workgroup of a level that is a launch of its own
# (matrix, MK_ILU_FUSE_ROWS or None for the default, launches of either sweep)
ILU_CASES = (("poisson1d_4500", None, 3), ("poisson1d_4500", 0, 4500),
             ("poisson2d_17", 16, 3), ("poisson2d_17", 17, 1), ("poisson2d_17", 1, 33),
             ("diagonal_600", 600, 1), ("diagonal_600", 0, 1))
_ILU = {}


def ilu_matrix(name):
    if name not in _ILU:
        if name == "poisson1d_4500":
            _ILU[name] = csr_ref.poisson1d(4500)
        elif name == "poisson2d_17":
            _ILU[name] = csr_ref.poisson2d(17)
        else:                                                # the `diagonal` of tests/test_gpu_ilu.py with 600 rows
            assert name == "diagonal_600"
            d = 1.0 + np.random.default_rng(5).random(600)
            _ILU[name] = csr_ref.from_coo(np.arange(600), np.arange(600), d, (600, 600))
    return _ILU[name]


def ilu_reference(name, kind):
    """(the matrix, the factor's values, the level widths of the forward and of the backward sweep, x, M^-1 x)."""
    key = (name, kind)
    if key not in _ILU:
        A = ilu_matrix(name)
        vals = (ilu_ref.ic0 if kind == "ic0" else ilu_ref.ilu0)(A.indptr, A.indices, A.data)
        widths = tuple([len(r) for r in ilu_ref.levels(A.indptr, A.indices, fw)] for fw in (True, False))
        x = np.random.default_rng(11).standard_normal(A.shape[0])
        _ILU[key] = (A, vals, widths[0], widths[1], x, ilu_ref.apply_rows(A.indptr, A.indices, vals, x, kind))
    return _ILU[key]


# ---------------------------------------------------------------------------------------------- the table
# (macro of include/mikrylov.h, the largest value a GPU test runs it at, the test).  tests/test_limits_cpu.py compares the rows
# with the header: a new limit needs a row here, that is, a test at the limit; a changed limit needs its test moved.
# MK_AMG_MAX_LEVELS bounds an argument and sizes nothing: 16 levels would take a matrix of more than 3^15 rows, so the value is
# run as the argument `max_levels` of a hierarchy that ends earlier.
_HERE = "test_gpu_limits.py::"
LIMITS = (
    ("MK_GMRES_MAX_RESTART", max(GMRES_RESTARTS), _HERE + "test_gmres_at_the_restart_limit"),
    ("MK_IDR_MAX_S", max(IDR_S), _HERE + "test_idr_at_the_shadow_limit"),
    ("MK_MSCG_MAX_SHIFTS", 32, "test_gpu_mscg.py::test_bits"),
    ("MK_TRLAN_MAX_NCV", min(TRLAN_NCV, TRSVD_NCV), _HERE + "test_trlan_at_the_basis_limit, " + _HERE + "test_trsvd_at_the_basis_limit"),
    ("MK_LOBPCG_MAX_BLOCK", max(LOBPCG_BLOCKS), _HERE + "test_lobpcg_at_the_block_limit"),
    ("MK_LBFGS_MAX_PAIRS", max(LBFGS_NPAIRS), _HERE + "test_lbfgs_at_the_pair_limit"),
    ("MK_CHEB_MAX_DEGREE", max(CHEB_DEGREES), _HERE + "test_chebyshev_applied_at_the_degree_limit"),
    ("MK_FILTER_MAX_DEGREE", max(FILTER_DEGREES), _HERE + "test_chebyshev_filter_applied_at_the_degree_limit"),
    ("MK_FSAI_MAX_ROW", 32, "test_gpu_fsai.py::test_row_length_edges"),
    ("MK_AMG_MAX_LEVELS", 16, _HERE + "test_amg_with_a_dense_level_of_several_rows_per_lane"),
    ("MK_AMG_MAX_COARSE", max(rows[-1] for _, rows in AMG_CASES), _HERE + "test_amg_with_a_dense_level_of_several_rows_per_lane"),
)
