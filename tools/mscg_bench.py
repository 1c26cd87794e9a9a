"""Device multi-shift CG (pykrylov_amd.ShiftedCG, csrc/mk_mscg.hip).  (a) Time per pass at n = 2^20 and 2^24 on a Poisson
matrix for nsigma = 1, 8 and 32 with every shift active, beside the byte model of DESIGN.md 3.13 at the bandwidth a plain
device-to-device copy reaches in the same run.  (b) poisson2d(2000) with eight shifts to 1e-8 relative in one multi-shift run,
against eight separate `PCG` solves on ``A + sigma_k I``.  One JSON line per measurement.

    python tools/mscg_bench.py [--quick] [--reps 10] [--passes 20] [--no-solves]

A pass sample is `--passes` passes enqueued in one `iterate` call and timed by the HIP events around it, after a warm-up call;
the median over `--reps` samples is reported.  A solve is run twice and the second, warm, run is reported.  Report, not a
test: nothing is asserted.
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
from pcg_bench import pass_samples                               # noqa: E402

GROUP = 8                                                        # columns per K3 launch (GM_GROUP, csrc/mk_multicol.h)


def model_bytes(n, nsigma, active=None):
    """Bytes of a pass beside the product: K2 24 n, the base p 16 n, per group launch 8 n, per active shift 32 n."""
    active = nsigma if active is None else active
    return (24 + 16 + 8 * ((nsigma + GROUP - 1) // GROUP) + 32 * active) * n


def pass_lines(name, make, reps, passes, counts=(1, 8, 32)):
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    rng = np.random.default_rng(0)
    dx, dy = _lib.DeviceArray.from_numpy(rng.standard_normal(n)), _lib.DeviceArray(n)
    copy = median_us(lambda: _lib.check(lib.mk_memcpy_d2d(dy.ptr, dx.ptr, 8 * n)), reps, 20)
    bw = 16.0 * n / (copy * 1e-6)                                # bytes per second of a plain copy: 8 n in, 8 n out
    b = op * (1.0 + rng.random(n))
    base = dict(abstol=0.0, reltol=0.0, matvec_max=1 << 40, check_curvature=0)      # (no shift ever freezes)
    for ns in counts:
        shifts = [float(s) for s in np.geomspace(1e-3, 1.0, ns)]
        with DeviceRun(op, _lib.MK_MSCG, b, shifts=shifts, **base) as run:
            out = pass_samples(run, passes, reps)
            product = run.time_product(0, 50) if out else float("nan")      # (destroys the loop's vectors: last)
        if not out:
            print(json.dumps({"matrix": name, "rows": n, "nsigma": ns, "error": "the run halted before a sample"}), flush=True)
            continue
        us = float(np.median(out))
        model = model_bytes(n, ns)
        beyond = us - product
        print(json.dumps({"matrix": name, "rows": n, "loop": "mscg", "nsigma": ns, "samples": len(out),
                          "passes_per_sample": passes, "pass_us": round(us, 2), "product_kernel_us": round(product, 2),
                          "copy_us": round(copy, 2), "copy_TBps": round(bw / 1e12, 3), "beyond_product_us": round(beyond, 2),
                          "model_bytes_beyond_product": model, "model_us_at_copy_rate": round(1e6 * model / bw, 2),
                          "ratio_to_model": round(beyond / (1e6 * model / bw), 3)}), flush=True)
    for d in (dx, dy):
        d.free()
    op.free()


def solve_lines(name, make, shifts, reltol=1e-8):
    from pykrylov_amd import PCG, IdentityOperator, ShiftedCG, _lib
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    rhs = op * np.ones(n)

    def timed(fn):
        best = None
        for _ in range(2):                                       # (the second run is warm)
            _lib.check(lib.mk_sync())
            t0 = time.perf_counter()
            out = fn()
            _lib.check(lib.mk_sync())
            best = time.perf_counter() - t0
        return best, out

    def multi():
        s = ShiftedCG(op, reltol=reltol, abstol=0.0)
        s.solve(rhs, shifts, matvec_max=20000)
        return s
    t_multi, s = timed(multi)
    true = [float(np.linalg.norm(rhs - (op * s.xs[k] + sg * s.xs[k])) / np.linalg.norm(rhs)) for k, sg in enumerate(shifts)]
    print(json.dumps({"solve": name, "reltol": reltol, "solver": "mscg", "shifts": list(shifts), "products": s.nMatvec,
                      "converged": bool(s.converged), "freeze_passes": [int(v) for v in s.shiftIters],
                      "solve_s": round(t_multi, 4), "worst_true_relative_residual": float("%.3g" % max(true)),
                      "workspace_MB": round(s.workspace_bytes / 1e6, 1)}), flush=True)
    eye = IdentityOperator(n)
    total, products, worst = 0.0, 0, 0.0
    for k, sg in enumerate(shifts):
        Ak = op if sg == 0.0 else op + sg * eye                 # (a composed device operator: the shift rides in the product)

        def single():
            p = PCG(Ak, reltol=reltol, abstol=0.0)
            p.solve(rhs, matvec_max=20000)
            return p
        t, p = timed(single)
        total += t
        products += p.nMatvec
        worst = max(worst, float(np.linalg.norm(rhs - (op * p.x + sg * p.x)) / np.linalg.norm(rhs)))
        print(json.dumps({"solve": name, "reltol": reltol, "solver": "pcg", "shift": sg, "products": p.nMatvec,
                          "converged": bool(p.converged), "solve_s": round(t, 4)}), flush=True)
    print(json.dumps({"solve": name, "reltol": reltol, "solver": "pcg, one solve per shift", "products": products,
                      "solve_s": round(total, 4), "worst_true_relative_residual": float("%.3g" % worst),
                      "mscg_speedup": round(total / t_multi, 2)}), flush=True)
    op.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small matrices only")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--no-solves", action="store_true", help="pass times only")
    a = ap.parse_args()
    from pykrylov_amd import gallery
    shifts = [0.0, 1e-3, 1e-2, 0.1, 0.5, 1.0, 2.0, 4.0]
    if a.quick:
        pass_lines("poisson2d(100)", lambda: gallery.poisson2d(100), a.reps, a.passes)
        if not a.no_solves:
            solve_lines("poisson2d(300)", lambda: gallery.poisson2d(300), shifts)
        return
    pass_lines("poisson2d(1024), n = 2^20", lambda: gallery.poisson2d(1024), a.reps, a.passes)
    pass_lines("poisson3d(256), n = 2^24", lambda: gallery.poisson3d(256), a.reps, a.passes)
    if not a.no_solves:
        solve_lines("poisson2d(2000)", lambda: gallery.poisson2d(2000), shifts)


if __name__ == "__main__":
    main()
