"""Device PCG (pykrylov_amd.PCG, csrc/mk_pcg.hip).  (a) Time per pass without a preconditioner and with a diagonal one at
n = 2^20 and 2^24 on a Poisson matrix, beside CG's three-kernel pass (MK_CG_FUSE=0) at the same size and the byte model of
DESIGN.md 3.12 at the bandwidth a plain device-to-device copy reaches in the same run.  (b) PCG with `tools.amg` against MINRES
with it and plain CG on poisson2d(2000) and poisson3d(256), to 1e-8 relative.  (c) The same with `ic0`, `fsai` and
`chebyshev(4)` on poisson2d(2000).  One JSON line per measurement.

    python tools/pcg_bench.py [--quick] [--reps 10] [--skip ic0]

A pass sample is `--passes` passes enqueued in one `iterate` call and timed by the HIP events around it, after a warm-up call;
the median over `--reps` samples is reported.  A solve is run twice and the second, warm, run is reported (IC(0), whose
level-scheduled sweeps take tens of seconds at this size, once).  Report, not a test: nothing is asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gmres_bench import median_us                                # noqa: E402


def pass_samples(run, passes, reps):
    run.setup()
    run.iterate(passes)                                          # (code objects, the storage format)
    out = []
    for _ in range(reps):
        if run.iterate(passes) != passes:                        # (a run that halted)
            break
        out.append(1e3 * run.timing()["iterate_ms"] / passes)
    return out


def pass_lines(name, make, reps, passes):
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    rng = np.random.default_rng(0)
    dx, dy = _lib.DeviceArray.from_numpy(rng.standard_normal(n)), _lib.DeviceArray(n)
    spmv = median_us(lambda: op.spmv_device(dx.ptr, dy.ptr), reps, 20)
    copy = median_us(lambda: _lib.check(lib.mk_memcpy_d2d(dy.ptr, dx.ptr, 8 * n)), reps, 20)
    bw = 16.0 * n / (copy * 1e-6)                                # bytes per second of a plain copy: 8 n in, 8 n out
    b = op * (1.0 + rng.random(n))
    diag = 1.0 / (4.0 + rng.random(n))
    base = dict(abstol=0.0, reltol=0.0, matvec_max=1 << 40, check_curvature=0)
    os.environ["MK_CG_FUSE"] = "0"                               # CG's three-kernel pass (read at every set-up)
    # (bytes per row beyond the product: CG reads its diagonal in K2 only, PCG in K2 and K3)
    cases = (("cg", _lib.MK_CG, None, {}, 64), ("cg", _lib.MK_CG, diag, {}, 72),
             ("pcg", _lib.MK_PCG, None, {"pcg": (False,)}, 64), ("pcg", _lib.MK_PCG, diag, {"pcg": (False,)}, 80),
             ("pcg_flexible", _lib.MK_PCG, None, {"pcg": (True,)}, 64), ("pcg_flexible", _lib.MK_PCG, diag, {"pcg": (True,)}, 80))
    for label, kind, d, extra, per_row in cases:
        with DeviceRun(op, kind, b, precon_diag=d, **dict(base, **extra)) as run:
            out = pass_samples(run, passes, reps)
            product = run.time_product(0, 50) if out else float("nan")      # (destroys the loop's vectors: last)
        if not out:
            print(json.dumps({"matrix": name, "rows": n, "loop": label, "error": "the run halted before a sample"}), flush=True)
            continue
        us = float(np.median(out))
        model = per_row * n
        beyond = us - product
        print(json.dumps({"matrix": name, "rows": n, "loop": label, "route": "none" if d is None else "diag",
                          "samples": len(out), "passes_per_sample": passes, "pass_us": round(us, 2),
                          "product_kernel_us": round(product, 2), "plain_product_us": round(spmv, 2), "copy_us": round(copy, 2),
                          "copy_TBps": round(bw / 1e12, 3), "beyond_product_us": round(beyond, 2),
                          "model_bytes_beyond_product": model, "model_us_at_copy_rate": round(1e6 * model / bw, 2),
                          "ratio_to_model": round(beyond / (1e6 * model / bw), 3)}), flush=True)
    del os.environ["MK_CG_FUSE"]
    for d in (dx, dy):
        d.free()
    op.free()


def solve_lines(name, make, precons, skip, reltol=1e-8):
    from pykrylov_amd import CG, PCG, Minres, _lib, tools
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    dx, dy = _lib.DeviceArray.from_numpy(np.ones(n)), _lib.DeviceArray(n)
    op.spmv_device(dx.ptr, dy.ptr)
    rhs = dy.to_numpy()                                          # b = A ones
    for d in (dx, dy):
        d.free()
    makers = {"none": lambda: None, "amg": lambda: tools.amg(op), "ic0": lambda: tools.ic0(op), "fsai": lambda: tools.fsai(op),
              "chebyshev4": lambda: tools.chebyshev(op, degree=4)}
    for label in precons:
        if label in skip:
            continue
        t0 = time.perf_counter()
        try:
            P = makers[label]()
        except Exception as exc:                                 # (e.g. IC(0) breaks down: reported, not fatal)
            print(json.dumps({"solve": name, "precon": label, "error": str(exc)[:200]}), flush=True)
            continue
        _lib.check(lib.mk_sync())
        t_setup = time.perf_counter() - t0
        solvers = ("cg", "pcg") if P is None else ("pcg", "pcg_flexible", "minres")
        for solver in solvers:
            best = None
            for _ in range(1 if label == "ic0" else 2):          # (the second run is warm)
                _lib.check(lib.mk_sync())
                t0 = time.perf_counter()
                if solver == "minres":
                    s = Minres(op)
                    s.solve(rhs, precon=P, show=False, check=False, etol=0.0, rtol=reltol, itnlim=20000)
                elif solver == "cg":
                    s = CG(op, reltol=reltol, abstol=0.0)
                    s.solve(rhs, matvec_max=20000)
                else:
                    s = PCG(op, precon=P, reltol=reltol, abstol=0.0)
                    s.solve(rhs, matvec_max=20000, flexible=solver == "pcg_flexible")
                _lib.check(lib.mk_sync())
                best = time.perf_counter() - t0
            err = float(np.abs(s.x - 1.0).max())
            true_rel = float(np.linalg.norm(rhs - op * s.x) / np.linalg.norm(rhs))
            done = {"itn": int(s.itn), "istop": int(s.istop)} if solver == "minres" else \
                {"passes": int(s.nMatvec), "converged": bool(s.converged)}
            print(json.dumps(dict({"solve": name, "reltol": reltol, "solver": solver, "precon": label}, **done,
                                  solve_s=round(best, 4), precon_setup_s=round(t_setup, 4), max_error=float("%.3g" % err),
                                  true_relative_residual=float("%.3g" % true_rel))), flush=True)
        if P is not None:
            P.free()
    op.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small matrices only")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--skip", default="", help="comma-separated preconditioners to leave out (e.g. ic0)")
    ap.add_argument("--no-solves", action="store_true", help="pass times only")
    a = ap.parse_args()
    from pykrylov_amd import gallery
    skip = set(a.skip.split(","))
    if a.quick:
        pass_lines("poisson2d(100)", lambda: gallery.poisson2d(100), a.reps, a.passes)
        if not a.no_solves:
            solve_lines("poisson2d(300)", lambda: gallery.poisson2d(300), ("none", "amg", "ic0", "fsai", "chebyshev4"), skip)
        return
    pass_lines("poisson2d(1024), n = 2^20", lambda: gallery.poisson2d(1024), a.reps, a.passes)
    pass_lines("poisson3d(256), n = 2^24", lambda: gallery.poisson3d(256), a.reps, a.passes)
    if a.no_solves:
        return
    solve_lines("poisson2d(2000)", lambda: gallery.poisson2d(2000), ("none", "amg", "ic0", "fsai", "chebyshev4"), skip)
    solve_lines("poisson3d(256)", lambda: gallery.poisson3d(256), ("none", "amg"), skip)


if __name__ == "__main__":
    main()
