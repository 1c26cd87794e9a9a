"""Device AMG preconditioner (tools.amg): set-up time, the hierarchy and the median apply time for smoother degrees 1, 2 and 3
against a byte model at a plain copy's rate, and CG and MINRES to 1e-8 relative with no preconditioner, with IC(0), with
Chebyshev of degree 4, with FSAI and with AMG of degree 1, 2 and 3 -- iterations and wall time -- on poisson2d(2000) and
poisson3d(256).  One JSON line per matrix and degree and one per solver run, printed as they are measured.

    python tools/amg_bench.py [--quick] [--reps 20] [--n2d 2000] [--n3d 256] [--skip ic0,...]

Times are medians over `reps` samples; a sample enqueues `inner` applies back to back and waits for the stream once, so it
measures device time per apply and not the host's wait.  Report, not a test: nothing is asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.cheb_bench import fmt_of, median_us  # noqa: E402

DEGREES = (1, 2, 3)


def copy_rate_gb_s(reps):
    """Bytes moved per second by a device-to-device copy of 256 MiB (read + write)."""
    from pykrylov_amd import _lib
    lib = _lib.init()
    n = 1 << 25
    a, b = _lib.DeviceArray(n), _lib.DeviceArray(n)
    us = median_us(lambda: _lib.check(lib.mk_memcpy_d2d(b.ptr, a.ptr, 8 * n)), reps, 5)
    a.free()
    b.free()
    return 16.0 * n / us / 1e3


def model_bytes(levels, degree, dense):
    """Bytes one V(1,1)-cycle moves with every matrix as plain CSR (12 bytes per nonzero, 4 per row) and every vector read or
    written once per kernel that touches it."""
    def smoother(n, nnz):
        return 40 * n + degree * (12 * nnz + 4 * n + 56 * n)    # init; per step the matrix, d in, dinv, res and out in and out, d out
    total = 0
    for k, lv in enumerate(levels):
        n, nnz = lv["rows"], lv["nnz"]
        if k == len(levels) - 1:
            total += 8 * n * n + 16 * n if dense else smoother(n, nnz)
            break
        nc, nnzp = levels[k + 1]["rows"], lv["nnz_p"]
        total += 2 * smoother(n, nnz)
        total += 2 * (12 * nnz + 4 * n + 24 * n)                 # r = b - A x: x, b in, r out
        total += 12 * nnzp + 4 * nc + 8 * n + 8 * nc             # b_next = R r
        total += 12 * nnzp + 4 * n + 8 * nc + 16 * n             # x += P e
        total += 24 * n                                          # x = x + S(r)
    return total


def matrix_lines(name, make, reps, copy_rate):
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    dx, dy = _lib.DeviceArray.from_numpy(np.random.default_rng(0).standard_normal(n)), _lib.DeviceArray(n)
    spmv = median_us(lambda: op.spmv_device(dx.ptr, dy.ptr), reps, 20)
    base = {"matrix": name, "rows": n, "nnz": op.nnz, "format": fmt_of(op), "plain_product_us": round(spmv, 2),
            "copy_gb_per_s": round(copy_rate, 1)}
    for degree in DEGREES:
        setups = []
        M = None
        for _ in range(2):                                       # (the first creation loads the code objects)
            if M is not None:
                M.free()
            _lib.check(lib.mk_sync())
            t0 = time.perf_counter()
            M = tools.amg(op, degree=degree)
            _lib.check(lib.mk_sync())
            setups.append(time.perf_counter() - t0)
        us = median_us(lambda: _lib.check(lib.mk_amg_apply(M.handle, dx.ptr, dy.ptr)), reps, 5)
        info, levels = M.info, M.levels
        model = model_bytes(levels, degree, info["coarse_dense"])
        line = dict(base, degree=degree, setup_s_first=round(setups[0], 4), setup_s=round(setups[1], 4),
                    setup_us_library=info["setup_us"], apply_us=round(us, 2), launches=info["launches"],
                    model_bytes=model, model_us_at_copy_rate=round(model / copy_rate / 1e3, 2),
                    ratio_to_model=round(us / (model / copy_rate / 1e3), 2), products_of_a=round(us / spmv, 2),
                    levels=[lv["rows"] for lv in levels], nnz=[lv["nnz"] for lv in levels],
                    mis_rounds=[lv["mis_rounds"] for lv in levels],
                    expanded=[[lv["expanded_ap"], lv["expanded_rap"]] for lv in levels],
                    chunks=[[lv["chunks_ap"], lv["chunks_rap"]] for lv in levels],
                    operator_complexity=round(M.operator_complexity, 4), grid_complexity=round(M.grid_complexity, 4),
                    coarse=info["coarse_solver"], bytes=info["bytes"])
        print(json.dumps(line), flush=True)
        M.free()
    for d in (dx, dy):
        d.free()
    op.free()


def solver_lines(name, make, skip, solver, reltol=1e-8):
    """`solver` = 'cg' or 'minres'.  CG here is the reference's recurrence, whose search direction is built from r and not
    from precon * r (cg.py:104,150-151): no preconditioner shortens its runs, so the counts that show what a preconditioner
    is worth are MINRES's."""
    from pykrylov_amd import CG, Minres, _lib, tools
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    dx, dy = _lib.DeviceArray.from_numpy(np.ones(n)), _lib.DeviceArray(n)
    op.spmv_device(dx.ptr, dy.ptr)
    rhs = dy.to_numpy()                                          # b = A ones
    for d in (dx, dy):
        d.free()
    cases = [("none", lambda: None), ("ic0", lambda: tools.ic0(op)), ("chebyshev4", lambda: tools.chebyshev(op, degree=4)),
             ("fsai", lambda: tools.fsai(op))]
    cases += [("amg%d" % k, lambda k=k: tools.amg(op, degree=k)) for k in DEGREES]
    for label, make_precon in cases:
        if label in skip:
            continue
        t0 = time.perf_counter()
        try:
            P = make_precon()
        except Exception as exc:                                 # (e.g. IC(0) breaks down: reported, not fatal)
            print(json.dumps({solver: name, "precon": label, "error": str(exc)[:200]}), flush=True)
            continue
        _lib.check(lib.mk_sync())
        t_setup = time.perf_counter() - t0
        best = None
        for _ in range(2):                                       # (the second run is warm)
            s = CG(op, precon=P, reltol=reltol, abstol=0.0) if solver == "cg" else Minres(op)
            _lib.check(lib.mk_sync())
            t0 = time.perf_counter()
            if solver == "cg":                                   # (no preconditioner shortens it: a budget of 500 products then)
                s.solve(rhs, matvec_max=5000 if P is None else 500)
            else:
                s.solve(rhs, precon=P, show=False, check=False, etol=0.0, rtol=reltol, itnlim=5000)
            _lib.check(lib.mk_sync())
            best = time.perf_counter() - t0
        err = float(np.abs(s.x - 1.0).max())
        done = {"matvecs": int(s.nMatvec), "converged": bool(s.converged)} if solver == "cg" else \
            {"itn": int(s.itn), "istop": int(s.istop)}
        print(json.dumps(dict({solver: name, "reltol": reltol, "precon": label}, **done, solve_s=round(best, 4),
                              precon_setup_s=round(t_setup, 4), max_error=float("%.3g" % err), format=fmt_of(op))), flush=True)
        if P is not None:
            P.free()
    op.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="poisson2d(300) and poisson3d(48)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n2d", type=int, default=2000)
    ap.add_argument("--n3d", type=int, default=256)
    ap.add_argument("--skip", default="", help="comma-separated CG cases to leave out (e.g. ic0)")
    ap.add_argument("--no-solves", action="store_true", help="set-up and apply times only")
    a = ap.parse_args()
    from pykrylov_amd import gallery
    n2, n3 = (300, 48) if a.quick else (a.n2d, a.n3d)
    rate = copy_rate_gb_s(a.reps)
    for name, make in (("poisson2d(%d)" % n2, lambda: gallery.poisson2d(n2)), ("poisson3d(%d)" % n3, lambda: gallery.poisson3d(n3))):
        matrix_lines(name, make, a.reps, rate)
        for solver in () if a.no_solves else ("cg", "minres"):
            solver_lines(name, make, set(a.skip.split(",")), solver)


if __name__ == "__main__":
    main()
