"""Least-squares solvers behind pykrylov's `lls` classes (reference pykrylov/lls/*.py).

`LSQRFramework`, `LSMRFramework`, `CRAIGFramework`, `CRAIGMRFramework` keep the reference's `solve`
signatures and result attributes; the Golub-Kahan bidiagonalisation (one product with A and one with
A' per iteration) and every scalar recurrence run on the GPU (``csrc/mk_lls.hip``).  With a
:class:`pykrylov_amd.linop.CsrOperator` both products run on the device (the transpose is built there on first
use); any other operator with ``A * v`` and ``A.T * u`` is called back on the host at each product site
(:class:`pykrylov_amd.linop.HostOperatorShell`).  Preconditioners `M`, `N` are resolved like the square solvers'
``precon``: a diagonal (``DiagonalOperator``, linop.py:473-516; ``mk_solver_set_lls_precon``) acts inside the kernels; a
device matrix or composite (``tools.block_jacobi``), an incomplete factorization (``tools.ilu0`` / ``tools.ic0``), an
``InverseLBFGSOperator``, a Chebyshev polynomial preconditioner (``tools.chebyshev``), an FSAI preconditioner
(``tools.fsai``) and an AMG preconditioner (``tools.amg``) are applied on the device at the
`u = M(Mu)` / `v = N(Nv)` sites (``mk_solver_set_lls_precon_csr / _ilu / _bfgs / _cheb / _fsai / _amg``); any other callable is called back on the host there
(``mk_solver_set_lls_precon_callback``).  After a solve `solver.precon_route` names the route of each side.  On several GPUs
the operator is split into row blocks with a replicated column space (:func:`pykrylov_amd.dist.partition_row_blocks`).
"""
from .solvers import LSQRFramework, LSMRFramework, CRAIGFramework, CRAIGMRFramework   # noqa: F401
