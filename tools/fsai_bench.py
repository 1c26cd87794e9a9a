"""Device FSAI preconditioner (tools.fsai): set-up time and the median apply time for power 1 and 2, next to two plain
products of the matrix and to the IC(0) apply, and MINRES to rtol = 1e-8 with no preconditioner, with IC(0), with Chebyshev
of degree 4 and with FSAI of power 1 and 2 -- iterations and solve time -- on poisson2d(1000), poisson3d(64) and 1138bus.
One JSON line per matrix and one per MINRES run.

    python tools/fsai_bench.py [--quick] [--reps 30]

Times are medians over `reps` samples; a sample enqueues `inner` applies (products) back to back and waits for the stream
once, so it measures device time per apply and not the host's wait.  Report, not a test: nothing is asserted.
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

POWERS = (1, 2)


def bus1138():
    """tests/golden/1138bus.mtx (symmetric storage, expanded) as a device matrix."""
    from pykrylov_amd import CsrOperator
    rows, cols, vals = [], [], []
    with open(os.path.join(ROOT, "tests", "golden", "1138bus.mtx")) as fh:
        header = fh.readline()
        assert "symmetric" in header
        line = fh.readline()
        while line.startswith("%"):
            line = fh.readline()
        for line in fh:
            i, j, v = line.split()
            i, j, v = int(i) - 1, int(j) - 1, float(v)
            rows.append(i), cols.append(j), vals.append(v)
            if i != j:
                rows.append(j), cols.append(i), vals.append(v)
    rows, cols, vals = np.array(rows), np.array(cols), np.array(vals)
    n = int(max(rows.max(), cols.max())) + 1
    order = np.lexsort((cols, rows))
    ip = np.zeros(n + 1, dtype=np.int64)
    ip[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return CsrOperator(ip, cols[order], vals[order], (n, n), symmetric=True)


def matrix_line(name, make, reps):
    """Set-up and apply times of one matrix; the byte model of an apply: 2 (12 nnz(G) + 4 n) + 32 n."""
    from pykrylov_amd import _lib, tools
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    dx, dy = _lib.DeviceArray.from_numpy(np.random.default_rng(0).standard_normal(n)), _lib.DeviceArray(n)
    line = {"matrix": name, "rows": n, "nnz": op.nnz}
    spmv = median_us(lambda: op.spmv_device(dx.ptr, dy.ptr), reps, 20)
    line["format"] = fmt_of(op)
    line["plain_product_us"] = round(spmv, 2)
    for power in POWERS:
        setups = []
        for _ in range(3):                                       # (the first creation loads the code objects)
            _lib.check(lib.mk_sync())
            t0 = time.perf_counter()
            M = tools.fsai(op, power=power)
            _lib.check(lib.mk_sync())
            setups.append(1e6 * (time.perf_counter() - t0))
            last = M
            if len(setups) < 3:
                M.free()
        M = last
        us = median_us(lambda: _lib.check(lib.mk_fsai_apply(M.handle, dx.ptr, dy.ptr)), reps, 10)
        info = M.info
        model = 2 * (12 * info["nnz"] + 4 * n) + 32 * n
        line["fsai%d" % power] = {
            "setup_us_python": round(float(np.median(setups[1:])), 1), "setup_us_library": info["setup_us"],
            "apply_us": round(us, 2), "two_products_us": round(2 * spmv, 2), "ratio_to_two_products": round(us / (2 * spmv), 3),
            "nnz_g": info["nnz"], "longest_row": info["longest_row"], "formats": [info["format_g"], info["format_gt"]],
            "bytes": info["bytes"], "model_bytes": model, "model_gb_per_s": round(model / us / 1e3, 1)}
        M.free()
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


def minres_lines(name, make, rtol=1e-8):
    from pykrylov_amd import Minres, _lib, tools
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    dx, dy = _lib.DeviceArray.from_numpy(np.ones(n)), _lib.DeviceArray(n)
    op.spmv_device(dx.ptr, dy.ptr)
    rhs = dy.to_numpy()                                          # b = A ones
    for d in (dx, dy):
        d.free()
    cases = [("none", lambda: None), ("ic0", lambda: tools.ic0(op)), ("chebyshev4", lambda: tools.chebyshev(op, degree=4))]
    cases += [("fsai%d" % p, lambda p=p: tools.fsai(op, power=p)) for p in POWERS]
    for label, make_precon in cases:
        t0 = time.perf_counter()
        try:
            P = make_precon()
        except Exception as exc:                                 # (e.g. IC(0) breaks down: reported, not fatal)
            print(json.dumps({"minres": name, "precon": label, "error": str(exc)[:200]}), flush=True)
            continue
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
        print(json.dumps({"minres": name, "rtol": rtol, "precon": label, "itn": int(s.itn), "istop": int(s.istop),
                          "solve_s": round(best, 4), "precon_setup_s": round(t_setup, 4), "format": fmt_of(op)}), flush=True)
        if P is not None:
            P.free()
    op.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="poisson2d(100) and 1138bus only")
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    from pykrylov_amd import gallery
    cases = (("poisson2d(100)", lambda: gallery.poisson2d(100)), ("1138bus", bus1138)) if a.quick else \
        (("poisson2d(1000)", lambda: gallery.poisson2d(1000)), ("poisson3d(64)", lambda: gallery.poisson3d(64)), ("1138bus", bus1138))
    for name, make in cases:
        matrix_line(name, make, a.reps)
        minres_lines(name, make)


if __name__ == "__main__":
    main()
