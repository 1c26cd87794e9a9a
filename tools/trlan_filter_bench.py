"""Chebyshev-filtered thick-restart Lanczos (pykrylov_amd.tools.cheb_filter, csrc/mk_chebfilt.hip): the time
of one filter step at degree 8, 16 and 32 against a plain product and against the byte model (the plain product of that
format plus 8 n bytes for y_{j-2}, none in the first step, at the bandwidth a plain device-to-device copy reaches in the same
run), and time, products, steps and cycles of solves to reltol = 1e-8 for nev = 4 with the automatic interval, the pilot run
shown separately, beside the unfiltered solve in the same process.  One JSON line per measurement.

    python tools/trlan_filter_bench.py [--quick] [--reps 10] [--matvec-max 20000] [--only 2d|3d]

The product and the applies are timed like the product of tools/trlan_bench.py: medians of `reps` batches behind two untimed
ones, a batch enqueued back to back and closed by one synchronisation.  Report, not a test: nothing is asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_us(enqueue, reps, inner):
    "tools/trlan_bench.py's timer: the median over `reps` batches of `inner` calls, two untimed batches first."
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


def step_lines(name, op, reps, degrees=(8, 16, 32)):
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    n = op.shape[0]
    rng = np.random.default_rng(0)
    dx, dy = _lib.DeviceArray.from_numpy(rng.standard_normal(n)), _lib.DeviceArray(n)
    spmv = median_us(lambda: op.spmv_device(dx.ptr, dy.ptr), reps, 20)
    copy = median_us(lambda: _lib.check(lib.mk_memcpy_d2d(dy.ptr, dx.ptr, 8 * n)), reps, 20)
    bw = 16.0 * n / (copy * 1e-6)                                # bytes per second of a plain copy: 8 n in, 8 n out
    fmt = _lib.c_i32()
    _lib.check(lib.mk_csr_format_info(op.handle, _lib.ctypes.byref(fmt), None, None, None, None))
    for d in degrees:
        # (an interval over the upper three quarters of a spectrum in [0, 12]: the time does not depend on it)
        F = tools.cheb_filter(op, degree=d, interval=(1.0, None), ref=-0.25)
        apply_us = median_us(lambda: F.apply_device(dx, dy), reps, 4)
        extra = 8.0 * n * (d - 1) / d                            # bytes per step beyond the plain product, averaged over the steps
        model = spmv + 1e6 * extra / bw
        print(json.dumps({"matrix": name, "rows": n, "format": fmt.value, "degree": d, "plain_product_us": round(spmv, 2),
                          "copy_TBps": round(bw / 1e12, 3), "apply_us": round(apply_us, 1), "step_us": round(apply_us / d, 2),
                          "step_over_product": round(apply_us / d / spmv, 3), "model_step_us": round(model, 2),
                          "ratio_to_model": round(apply_us / d / model, 3), "owned_bytes": F.info["bytes"]}), flush=True)
        F.free()
    for b in (dx, dy):
        b.free()


def solve_lines(name, op, matvec_max, reltol=1e-8, nev=4, ncvs=(20, 40), degrees=(8, 16, 32)):
    from pykrylov_amd import ThickRestartLanczos, _lib, tools
    lib = _lib.init()

    def timed(fn):
        _lib.check(lib.mk_sync())
        t0 = time.perf_counter()
        out = fn()
        _lib.check(lib.mk_sync())
        return out, time.perf_counter() - t0

    for ncv in ncvs:
        for which in ("SA", "LA"):
            s = ThickRestartLanczos(op, abstol=0.0, reltol=reltol)
            _, dt = timed(lambda: s.solve(nev, which=which, ncv=ncv, matvec_max=matvec_max))
            base = {"solve": name, "which": which, "nev": nev, "ncv": ncv, "reltol": reltol}
            print(json.dumps(dict(base, filter=None, products=int(s.nMatvec), steps=int(s.nIter), cycles=int(s.cycles),
                                  converged=bool(s.converged), residNorm=float(s.residNorm), threshold=float(s.threshold),
                                  w=[float(v) for v in s.w], solve_s=round(dt, 4))), flush=True)
            plain_s, plain_w = dt, s.w.copy()
            for d in degrees:
                F, pilot_s = timed(lambda: tools.cheb_filter_for(op, nev, which, degree=d))
                f = ThickRestartLanczos(op, abstol=0.0, reltol=reltol)
                _, dt = timed(lambda: f.solve(nev, which=which, ncv=ncv, filter=F))
                same = len(f.w) == len(plain_w) and float(np.max(np.abs(f.w - plain_w))) if len(f.w) == len(plain_w) else None
                print(json.dumps(dict(base, filter=d, degree_used=F.degree, interval=list(F.interval), ref=F.ref,
                                      products=int(f.nMatvec), pilot_products=int(f.pilotMatvec), steps=int(f.nIter),
                                      cycles=int(f.cycles), converged=bool(f.converged), outside=int(f.outside),
                                      residNorm=float(f.residNorm), threshold=float(f.threshold), w=[float(v) for v in f.w],
                                      max_w_difference_to_plain=same, solve_s=round(dt, 4), pilot_s=round(pilot_s, 4),
                                      speedup_with_pilot=round(plain_s / (dt + pilot_s), 3))), flush=True)
                F.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small matrix only")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--matvec-max", type=int, default=20000, help="the cap of the unfiltered solves")
    ap.add_argument("--only", choices=("2d", "3d"), default=None, help="one of the two full-size matrices")
    a = ap.parse_args()
    from pykrylov_amd import gallery
    sizes = [("poisson2d(100)", lambda: gallery.poisson2d(100))] if a.quick else \
        [(nm, mk) for key, nm, mk in (("2d", "poisson2d(1024), n = 2^20", lambda: gallery.poisson2d(1024)),
                                      ("3d", "poisson3d(256), n = 2^24", lambda: gallery.poisson3d(256)))
         if a.only in (None, key)]
    for name, make in sizes:
        op = make()
        step_lines(name, op, a.reps)
        solve_lines(name, op, a.matvec_max)
        op.free()


if __name__ == "__main__":
    main()
