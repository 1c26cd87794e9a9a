"""Device ILU(0) / IC(0): analysis and factor time, apply time, levels and launches with and without thin-level fusion, the
same apply as a host callback, and BiCGSTAB on random_diagdom(10**6) with no / diagonal / block-Jacobi(4) / ILU(0)
preconditioning.  One JSON line per matrix (and one per BiCGSTAB run).

    python tools/ilu_bench.py [--quick] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def apply_us(M, n, reps):
    """Median of `reps` device applies (in place, one vector), each timed from its enqueue to the end of the stream."""
    from pykrylov_amd import _lib
    lib = _lib.init()
    d = _lib.DeviceArray.from_numpy(np.random.default_rng(0).standard_normal(n))
    _lib.check(lib.mk_ilu_apply(M.handle, d.ptr, d.ptr))
    _lib.check(lib.mk_sync())
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _lib.check(lib.mk_ilu_apply(M.handle, d.ptr, d.ptr))
        _lib.check(lib.mk_sync())
        out.append(1e6 * (time.perf_counter() - t0))
    d.free()
    return float(np.median(out))


def host_apply_us(M, n, reps):
    """The same apply as the host callback path runs it: copy to the host, reference apply, copy back."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _ilu_ref as ref
    ip, ix, vals, _ = M.factor_arrays()
    lev = (ref.levels(ip, ix, True), ref.levels(ip, ix, False))
    from pykrylov_amd import _lib
    d = _lib.DeviceArray.from_numpy(np.random.default_rng(0).standard_normal(n))
    out = []
    for _ in range(max(3, reps // 10)):
        t0 = time.perf_counter()
        r = d.to_numpy()
        d.upload(ref.apply(ip, ix, vals, r, M.kind, lev))
        _lib.check(_lib.init().mk_sync())
        out.append(1e6 * (time.perf_counter() - t0))
    d.free()
    return float(np.median(out))


def matrix_line(name, make, kinds, reps, host):
    from pykrylov_amd import tools
    op = make()
    n = op.shape[0]
    line = {"matrix": name, "rows": n, "nnz": op.nnz}
    for kind in kinds:
        for fuse in (None, "0"):
            if fuse is None:
                os.environ.pop("MK_ILU_FUSE_ROWS", None)
            else:
                os.environ["MK_ILU_FUSE_ROWS"] = fuse
            M = getattr(tools, kind)(op)
            info = M.info
            tag = kind + ("" if fuse is None else "_unfused")
            line[tag] = {"levels": list(M.levels), "launches": list(M.launches), "widest": info["widest_level"],
                         "analysis_ms": info["analysis_us"] / 1e3, "factor_ms": info["factor_us"] / 1e3,
                         "bytes": info["bytes"], "apply_us": round(apply_us(M, n, reps), 1)}
            if fuse is None and host:
                line[tag]["host_callback_apply_us"] = round(host_apply_us(M, n, reps), 1)
            M.free()
    os.environ.pop("MK_ILU_FUSE_ROWS", None)
    op.free()
    print(json.dumps(line), flush=True)


def bicgstab_lines(n):
    import pykrylov_amd
    from pykrylov_amd import gallery, tools, _lib
    from pykrylov_amd.linop import DiagonalOperator
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _ilu_ref as ref
    op = gallery.random_diagdom(n)
    ip, ix, data = op.to_csr_arrays()
    rows = np.repeat(np.arange(n), np.diff(ip))
    diag = data[ix == rows]
    rhs = np.ones(n)
    t0 = time.perf_counter()
    M = tools.ilu0(op)
    t_ilu = time.perf_counter() - t0
    _, _, vals, _ = M.factor_arrays()
    cases = [("none", lambda: None, 0.0), ("diagonal", lambda: DiagonalOperator(1.0 / diag), 0.0),
             ("block_jacobi4", lambda: tools.block_jacobi(op, 4), None), ("ilu0", lambda: M, t_ilu),
             ("ilu0_host_callback", lambda: ref.HostIlu(ip, ix, vals, "ilu0", vectorised=True), t_ilu)]
    for name, make, setup_s in cases:
        t0 = time.perf_counter()
        P = make()
        t_make = time.perf_counter() - t0
        s = pykrylov_amd.BiCGSTAB(op, precon=P, reltol=1e-8, abstol=0.0)
        _lib.check(_lib.init().mk_sync())
        t0 = time.perf_counter()
        s.solve(rhs, matvec_max=4 * n)
        _lib.check(_lib.init().mk_sync())
        t_solve = time.perf_counter() - t0
        print(json.dumps({"bicgstab": "random_diagdom(%d)" % n, "precon": name, "converged": bool(s.converged),
                          "matvecs": int(s.nMatvec), "solve_s": round(t_solve, 4),
                          "precon_setup_s": round(t_make if setup_s is None else setup_s + t_make, 4)}), flush=True)
    M.free()
    op.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small matrices only")
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    from pykrylov_amd import CsrOperator, gallery
    sys.path.insert(0, ROOT)
    from oracle import csr_ref

    def mtx(name, sym):
        def make():
            A = csr_ref.read_matrix_market(os.path.join(ROOT, "tests", "golden", name + ".mtx"))
            return CsrOperator(A.indptr, A.indices, A.data, A.shape, symmetric=sym)
        return make
    matrix_line("jpwh_991", mtx("jpwh_991", False), ("ilu0",), a.reps, True)
    matrix_line("1138bus", mtx("1138bus", True), ("ilu0", "ic0"), a.reps, True)
    if a.quick:
        return
    matrix_line("random_diagdom(10**6)", lambda: gallery.random_diagdom(10 ** 6), ("ilu0",), a.reps, True)
    matrix_line("poisson3d(64)", lambda: gallery.poisson3d(64), ("ilu0", "ic0"), a.reps, True)
    matrix_line("poisson2d(1000)", lambda: gallery.poisson2d(1000), ("ic0",), max(5, a.reps // 5), False)
    bicgstab_lines(10 ** 6)


if __name__ == "__main__":
    main()
