"""Device Chebyshev polynomial preconditioner (tools.chebyshev): the apply of degree 2, 4 and 8 next to k plain products of
the same matrix and to the IC(0) apply, and MINRES to rtol = 1e-8 with no preconditioner, with IC(0) and with Chebyshev of
degree 4 and 8, on the default interval (Gershgorin / 30) and on the device Lanczos estimate's (interval='lanczos').
`--lanczos`: the Lanczos estimate alone -- microseconds per step next to the plain product, and the set-up time of
chebyshev(interval='lanczos') against the default -- on poisson3d(256) and poisson2d(1000).  Symmetric structured-grid
matrices only.  One JSON line per matrix and one per MINRES run.

    python tools/cheb_bench.py [--quick] [--lanczos] [--reps 30]

Times are medians over `reps` samples; a sample enqueues `inner` applies (products) back to back and waits for the stream
once, so it measures device time per apply and not the host's wait.  Report, not a test: nothing is asserted.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_us(enqueue, reps, inner):
    from pykrylov_amd import _lib
    lib = _lib.init()
    for _ in range(2):                                           # (first launches load code objects, build the format)
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


def fmt_of(op):
    from pykrylov_amd import _lib
    fmt = ctypes.c_int32()
    _lib.check(_lib.init().mk_csr_format_info(op.handle, ctypes.byref(fmt), None, None, None, None))
    return fmt.value


def matrix_line(name, make, reps, degrees=(2, 4, 8)):
    """Apply times of one matrix; the byte model of a step: the plain product's traffic + 40 n bytes."""
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    rng = np.random.default_rng(0)
    dx, dy = _lib.DeviceArray.from_numpy(rng.standard_normal(n)), _lib.DeviceArray(n)
    line = {"matrix": name, "rows": n, "nnz": op.nnz}
    spmv = median_us(lambda: op.spmv_device(dx.ptr, dy.ptr), reps, 20)
    line["format"] = fmt_of(op)
    line["plain_product_us"] = round(spmv, 2)
    for scaled in (False, True):
        for k in degrees:
            M = tools.chebyshev(op, degree=k, scale_diag=scaled)
            us = median_us(lambda: _lib.check(lib.mk_cheb_apply(M.handle, dx.ptr, dy.ptr)), reps, 10)
            line["cheb%d%s" % (k, "_scaled" if scaled else "")] = {
                "apply_us": round(us, 2), "k_products_us": round(k * spmv, 2), "ratio_to_k_products": round(us / (k * spmv), 3),
                "setup_us": M.info["setup_us"], "bytes": M.info["bytes"], "interval": list(M.interval)}
            M.free()
    line["format_after"] = fmt_of(op)
    t0 = time.perf_counter()
    F = tools.ic0(op)
    line["ic0"] = {"setup_s": round(time.perf_counter() - t0, 4), "levels": list(F.levels), "launches": list(F.launches),
                   "apply_us": round(median_us(lambda: _lib.check(lib.mk_ilu_apply(F.handle, dx.ptr, dy.ptr)),
                                               max(5, reps // 3), 1), 1)}
    F.free()
    for d in (dx, dy):
        d.free()
    op.free()
    print(json.dumps(line), flush=True)


def lanczos_line(name, make, reps):
    """The Lanczos estimate (tools.lanczos) of one matrix.  A run allocates and frees its vectors and downloads once, so the
    time per step is the difference of a 20-step and a 10-step run over 10; the byte model of a step is the
    plain product's traffic + 56 n bytes -- 48 n more than the product, which writes 8 n itself."""
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    dx, dy = _lib.DeviceArray.from_numpy(np.random.default_rng(0).standard_normal(n)), _lib.DeviceArray(n)
    line = {"lanczos": name, "rows": n, "nnz": op.nnz}
    spmv = median_us(lambda: op.spmv_device(dx.ptr, dy.ptr), reps, 20)
    line["format"] = fmt_of(op)
    line["plain_product_us"] = round(spmv, 2)
    for d in (dx, dy):
        d.free()

    def run_us(steps, scaled):
        out = []
        for _ in range(max(5, reps // 3)):
            _lib.check(lib.mk_sync())
            t0 = time.perf_counter()
            r = tools.lanczos(op, steps=steps, scale_diag=scaled)
            out.append(1e6 * (time.perf_counter() - t0))
        return float(np.median(out)), r
    for scaled in (False, True):
        run_us(10, scaled)                                       # (code objects)
        t10, r10 = run_us(10, scaled)
        t20, r20 = run_us(20, scaled)
        step = (t20 - t10) / 10.0
        line["scaled" if scaled else "plain"] = {
            "run10_us": round(t10, 1), "run20_us": round(t20, 1), "step_us": round(step, 2),
            "step_over_product": round(step / spmv, 3), "product_rate_fraction": round(spmv / step, 3) if step > 0 else None,
            "steps": [r10.steps, r20.steps], "launches": [r10.info["launches"], r20.info["launches"]],
            "bytes": r20.info["bytes"], "bounds10": list(r10.bounds), "bounds20": list(r20.bounds)}
        for label, kw in (("setup_default_us", {}), ("setup_lanczos_us", {"interval": "lanczos"})):
            out = []
            for _ in range(max(5, reps // 3)):
                _lib.check(lib.mk_sync())
                t0 = time.perf_counter()
                M = tools.chebyshev(op, degree=4, scale_diag=scaled, **kw)
                _lib.check(lib.mk_sync())
                out.append(1e6 * (time.perf_counter() - t0))
                iv = M.interval
                M.free()
            line["scaled" if scaled else "plain"][label] = round(float(np.median(out)), 1)
            line["scaled" if scaled else "plain"][label.replace("setup", "interval").replace("_us", "")] = list(iv)
    line["format_after"] = fmt_of(op)
    op.free()
    print(json.dumps(line), flush=True)


def minres_lines(name, make, rtol=1e-8):
    from pykrylov_amd import Minres, _lib, tools
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    rhs = np.ones(n)
    cases = [("none", lambda: None, 0), ("ic0", lambda: tools.ic0(op), 0), ("chebyshev4", lambda: tools.chebyshev(op, degree=4), 4),
             ("chebyshev8", lambda: tools.chebyshev(op, degree=8), 8),
             ("chebyshev4_lanczos", lambda: tools.chebyshev(op, degree=4, interval="lanczos"), 4),
             ("chebyshev8_lanczos", lambda: tools.chebyshev(op, degree=8, interval="lanczos"), 8)]
    for label, make_precon, k in cases:
        t0 = time.perf_counter()
        P = make_precon()
        _lib.check(lib.mk_sync())
        t_setup = time.perf_counter() - t0
        best = None
        for _ in range(2):                                       # (the second run is warm)
            s = Minres(op)
            _lib.check(lib.mk_sync())
            t0 = time.perf_counter()
            s.solve(rhs, precon=P, show=False, check=False, etol=0.0, rtol=rtol)
            _lib.check(lib.mk_sync())
            best = time.perf_counter() - t0
        # products with A: one per iteration, k per apply of the Chebyshev object, one apply per iteration and one at set-up
        products = int(s.itn) + k * (int(s.itn) + 1)
        print(json.dumps({"minres": name, "rtol": rtol, "precon": label, "itn": int(s.itn), "istop": int(s.istop),
                          "products_with_A": products, "solve_s": round(best, 4), "precon_setup_s": round(t_setup, 4),
                          "interval": list(P.interval) if k else None, "format": fmt_of(op)}), flush=True)
        if P is not None:
            P.free()
    op.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small matrix only")
    ap.add_argument("--lanczos", action="store_true", help="the Lanczos estimate alone, on poisson3d(256) and poisson2d(1000)")
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    from pykrylov_amd import gallery
    if a.lanczos:
        for name, make in ((("poisson2d(100)", lambda: gallery.poisson2d(100)),) if a.quick else
                           (("poisson3d(256)", lambda: gallery.poisson3d(256)), ("poisson2d(1000)", lambda: gallery.poisson2d(1000)))):
            lanczos_line(name, make, a.reps)
        return
    if a.quick:
        matrix_line("poisson2d(100)", lambda: gallery.poisson2d(100), a.reps)
        lanczos_line("poisson2d(100)", lambda: gallery.poisson2d(100), a.reps)
        minres_lines("poisson2d(100)", lambda: gallery.poisson2d(100))
        return
    for name, make in (("poisson2d(1000)", lambda: gallery.poisson2d(1000)), ("poisson3d(64)", lambda: gallery.poisson3d(64))):
        matrix_line(name, make, a.reps)
        lanczos_line(name, make, a.reps)
        minres_lines(name, make)


if __name__ == "__main__":
    main()
