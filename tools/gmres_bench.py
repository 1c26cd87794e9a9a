"""Device GMRES(m) (pykrylov_amd.GMRES, csrc/mk_gmres.hip): time per Arnoldi step at n = 2^20 and 2^24 for restart 10 and 30
against the byte model of DESIGN.md 3.8 at the bandwidth a plain device-to-device copy reaches in the same run, and the time
to 1e-8 on random_diagdom(10**6) beside Bi-CGSTAB.  One JSON line per (matrix, restart) and one per solve.

    python tools/gmres_bench.py [--quick] [--reps 10]

A sample is one whole cycle (restart passes: the steps, the cycle end and the restart's residual product) enqueued in one
`iterate` call and timed by the HIP events around it; the first cycle of a run is left out.  Report, not a test: nothing is
asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUP = 8                                                        # basis columns per launch (GM_GROUP)


def median_us(enqueue, reps, inner):
    from pykrylov_amd import _lib
    lib = _lib.init()
    for _ in range(2):
        enqueue()
    _lib.check(lib.mk_sync())
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            enqueue()
        _lib.check(lib.mk_sync())
        out.append(1e6 * (time.perf_counter() - t0) / inner)
    return float(np.median(out))


def cycle_model_bytes(n, m, reorth):
    """Bytes of a cycle beyond its m + 1 products: per step (1 + reorth) (16 j + 24 ceil(j / G)) n + 16 n (the last step
    writes no v_{m+1}: 16 n less), the cycle end (8 m + 16 ceil(m / G)) n + 24 n and the restart 40 n."""
    steps = sum((1 + reorth) * (16 * j + 24 * -(-j // GROUP)) * n + 16 * n for j in range(1, m + 1)) - 16 * n
    return steps + (8 * m + 16 * -(-m // GROUP)) * n + 24 * n + 40 * n


def step_lines(name, make, reps, restarts=(10, 30)):
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
    for m in restarts:
        for reorth in (1, 0):
            with DeviceRun(op, _lib.MK_GMRES, b, abstol=0.0, reltol=0.0, matvec_max=1 << 40, restart=m, reorth=reorth) as run:
                run.setup()
                run.iterate(m)                                   # (code objects, the storage format)
                out = []
                for _ in range(reps):
                    assert run.iterate(m) == m
                    out.append(1e3 * run.timing()["iterate_ms"])
                res = run.finish()
            cyc = float(np.median(out))
            model = cycle_model_bytes(n, m, reorth)
            other = cyc - (m + 1) * spmv
            print(json.dumps({"matrix": name, "rows": n, "restart": m, "reorth": reorth, "plain_product_us": round(spmv, 2),
                              "copy_us": round(copy, 2), "copy_TBps": round(bw / 1e12, 3), "cycle_us": round(cyc, 1),
                              "step_us": round(cyc / m, 2), "beyond_products_us": round(other, 1),
                              "model_bytes_beyond_products": model, "model_us_at_copy_rate": round(1e6 * model / bw, 1),
                              "ratio_to_model": round(other / (1e6 * model / bw), 3), "basis_bytes": int(res.aux[2])}), flush=True)
    for d in (dx, dy):
        d.free()
    op.free()


def solve_lines(n, reltol=1e-8):
    from pykrylov_amd import GMRES, BiCGSTAB, _lib, gallery
    lib = _lib.init()
    op = gallery.random_diagdom(n)
    b = op * np.ones(n)
    for label, make, kw in (("bicgstab", lambda: BiCGSTAB(op, reltol=reltol), {}),
                            ("gmres10", lambda: GMRES(op, reltol=reltol), {"restart": 10}),
                            ("gmres30", lambda: GMRES(op, reltol=reltol), {"restart": 30}),
                            ("gmres30_cgs1", lambda: GMRES(op, reltol=reltol), {"restart": 30, "reorth": False})):
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
                          "solve_s": round(best, 4)}), flush=True)
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
