"""Device IDR(s) (pykrylov_amd.IDR, csrc/mk_idr.hip): time per step at n = 2^20 and 2^24 for s = 1, 4 and 8 against the byte
model of DESIGN.md 3.10 at the bandwidth a plain device-to-device copy reaches in the same run, and the time to 1e-8 on
random_diagdom(10**6) beside Bi-CGSTAB and GMRES(30).  One JSON line per (matrix, s) and one per solve.

    python tools/idr_bench.py [--quick] [--reps 10]

A sample is one whole cycle (s passes: the inner steps, the dimension-reduction step and f = P r of the next cycle) enqueued
in one `iterate` call and timed by the HIP events around it; the first cycle of a run is left out.  Report, not a test:
nothing is asserted.
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

GROUP = 8                                                        # columns per launch (GM_GROUP)


def groups(k):
    return -(-k // GROUP)


def cycle_model_bytes(n, s):
    """Bytes of a cycle beyond its s + 1 products, without a preconditioner.  Inner step k: the combination
    (16 (s - k) + 16 + 32 (groups(s - k) - 1)) n, the dots (8 s + 8 groups(s)) n, the fused update 48 n at k = 0 and
    (16 k + 32 groups(k) + 32) n after it.  The dimension-reduction step: 16 n for its two dots, 40 n for r and x, and the
    dots of f = P r."""
    dots = (8 * s + 8 * groups(s)) * n
    inner = 0
    for k in range(s):
        inner += (16 * (s - k) + 16 + 32 * (groups(s - k) - 1)) * n + dots
        inner += 48 * n if k == 0 else (16 * k + 32 * groups(k) + 32) * n
    return inner + 56 * n + dots


def step_lines(name, make, reps, ss=(1, 4, 8)):
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
    for s in ss:
        with DeviceRun(op, _lib.MK_IDR, b, abstol=0.0, reltol=0.0, matvec_max=1 << 40, idr=(s, 1, None)) as run:
            run.setup()
            run.iterate(s)                                       # (code objects, the storage format)
            out = []
            for _ in range(reps):
                if run.iterate(s) != s + 1:                      # (a run that broke down or ran out of residual)
                    break
                out.append(1e3 * run.timing()["iterate_ms"])
            res = run.finish()
        if not out:
            print(json.dumps({"matrix": name, "rows": n, "s": s, "error": "the run halted before a cycle was timed",
                              "breakdown": int(res.aux[3])}), flush=True)
            continue
        cyc = float(np.median(out))
        model = cycle_model_bytes(n, s)
        other = cyc - (s + 1) * spmv
        print(json.dumps({"matrix": name, "rows": n, "s": s, "cycles_timed": len(out), "plain_product_us": round(spmv, 2),
                          "copy_us": round(copy, 2), "copy_TBps": round(bw / 1e12, 3), "cycle_us": round(cyc, 1),
                          "step_us": round(cyc / (s + 1), 2), "beyond_products_us": round(other, 1),
                          "model_bytes_beyond_products": model, "model_us_at_copy_rate": round(1e6 * model / bw, 1),
                          "ratio_to_model": round(other / (1e6 * model / bw), 3), "workspace_bytes": int(res.aux[2])}), flush=True)
    for d in (dx, dy):
        d.free()
    op.free()


def solve_lines(n, reltol=1e-8):
    from pykrylov_amd import GMRES, IDR, BiCGSTAB, _lib, gallery
    lib = _lib.init()
    op = gallery.random_diagdom(n)
    b = op * np.ones(n)
    for label, make, kw in (("bicgstab", lambda: BiCGSTAB(op, reltol=reltol), {}),
                            ("gmres30", lambda: GMRES(op, reltol=reltol), {"restart": 30}),
                            ("idr1", lambda: IDR(op, reltol=reltol), {"s": 1}),
                            ("idr4", lambda: IDR(op, reltol=reltol), {"s": 4}),
                            ("idr8", lambda: IDR(op, reltol=reltol), {"s": 8})):
        best = None
        for _ in range(2):                                       # (the second run is warm)
            s = make()
            _lib.check(lib.mk_sync())
            t0 = time.perf_counter()
            s.solve(b, **kw)
            _lib.check(lib.mk_sync())
            best = time.perf_counter() - t0
        err = float(np.max(np.abs(s.x - 1.0)))
        print(json.dumps({"solve": "random_diagdom(%d)" % n, "reltol": reltol, "solver": label, "products": int(s.nMatvec),
                          "converged": bool(s.converged), "residNorm": float(s.residNorm), "max_error": err,
                          "solve_ms": round(1e3 * best, 2)}), flush=True)
    op.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small matrices only")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    from pykrylov_amd import gallery
    if a.quick:
        step_lines("poisson2d(100)", lambda: gallery.poisson2d(100), a.reps)
        solve_lines(10 ** 4)
        return
    step_lines("poisson2d(1024), n = 2^20", lambda: gallery.poisson2d(1024), a.reps)
    step_lines("poisson3d(256), n = 2^24", lambda: gallery.poisson3d(256), a.reps)
    solve_lines(10 ** 6)


if __name__ == "__main__":
    main()
