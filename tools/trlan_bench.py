"""Device thick-restart Lanczos (pykrylov_amd.ThickRestartLanczos, csrc/mk_trlan.hip): time per Lanczos step at n = 2^20 and
2^24 for ncv 20 and 40 against the byte model of DESIGN.md 3.15 at the bandwidth a plain device-to-device copy reaches in the
same run; the rotation kernel against the same rotation composed of GmOpCombine launches; the host part of a cycle, also at
ncv = 128; and time and products to reltol = 1e-8 for nev = 4.  One JSON line per measurement.

    python tools/trlan_bench.py [--quick] [--reps 10] [--matvec-max 20000]

A sample is one whole cycle (ncv - keep steps, the download, the small eigenproblem on the host, the upload and the rotation)
enqueued by one `iterate` call and timed by the HIP events around it; the first cycle of a run, which takes ncv steps, is left
out.  The library reports the host part of each cycle (mk_solver_history2) and the device time of the last rotation
(mk_result.aux[7]); what remains of a cycle is its steps.  Report, not a test: nothing is asserted.
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
KT = 16                                                          # output columns per rotation launch (TR_KT)


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


def steps_model_bytes(n, m, keep):
    "Bytes of the steps keep + 1 .. m beyond their products: per step 2 (16 j + 24 ceil(j / G)) n + 16 n."
    return sum(2 * (16 * j + 24 * -(-j // GROUP)) * n + 16 * n for j in range(keep + 1, m + 1))


def rotation_model_bytes(n, m, kk):
    "8 n (m ceil(kk / KT) + kk), and 16 n per column copied down from the spare columns."
    g = -(-kk // KT)
    return 8 * n * (m * g + kk) + 16 * n * KT * (g - 1)


def composed_model_bytes(n, m, kk):
    "Per output column: m columns in, and per group of G the column itself out (and in again after the first); then the copy."
    g = -(-m // GROUP)
    return kk * (8 * n * m + 8 * n * (2 * g - 1)) + 16 * n * kk


def cycles(op, reps, nev, ncv, which, keep=0, window=0):
    """Medians over `reps` cycles behind the first: (cycle us, host part us, rotation us, keep, sweeps)."""
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    cyc, host, rot = [], [], []
    with DeviceRun(op, _lib.MK_TRLAN, None, abstol=0.0, reltol=0.0, matvec_max=1 << 40, window=window,
                   eig=(nev, ncv, which, keep, 1)) as run:
        run.setup()
        run.iterate(1)                                           # (code objects, the storage format, the full first cycle)
        for _ in range(reps):
            run.iterate(1)
            cyc.append(1e3 * run.timing()["iterate_ms"])
            res = run.finish()
            rot.append(1e3 * res.aux[7])
            host.append(1e3 * run.history2()[-1])
        keep, sweeps, halted = int(res.aux[2]), int(res.aux[6]), bool(res.halted)
    return float(np.median(cyc)), float(np.median(host)), float(np.median(rot)), keep, sweeps, halted


def step_lines(name, make, reps, ncvs=(20, 40), nev=4):
    from pykrylov_amd import _lib
    lib = _lib.init()
    op = make()
    n = op.shape[0]
    rng = np.random.default_rng(0)
    dx, dy = _lib.DeviceArray.from_numpy(rng.standard_normal(n)), _lib.DeviceArray(n)
    spmv = median_us(lambda: op.spmv_device(dx.ptr, dy.ptr), reps, 20)
    copy = median_us(lambda: _lib.check(lib.mk_memcpy_d2d(dy.ptr, dx.ptr, 8 * n)), reps, 20)
    bw = 16.0 * n / (copy * 1e-6)                                # bytes per second of a plain copy: 8 n in, 8 n out
    for d in (dx, dy):
        d.free()
    for m in ncvs:
        for which in (1, 0):
            cyc, host, rot, keep, sweeps, halted = cycles(op, reps, nev, m, which)
            steps = m - keep
            model = steps_model_bytes(n, m, keep)
            other = cyc - host - rot - steps * spmv
            print(json.dumps({"matrix": name, "rows": n, "ncv": m, "keep": keep, "which": "LA" if which else "SA",
                              "plain_product_us": round(spmv, 2), "copy_TBps": round(bw / 1e12, 3), "cycle_us": round(cyc, 1),
                              "host_part_us": round(host, 1), "rotation_us": round(rot, 1), "jacobi_sweeps": sweeps,
                              "step_us": round((cyc - host - rot) / steps, 2), "beyond_products_us": round(other, 1),
                              "model_us_at_copy_rate": round(1e6 * model / bw, 1),
                              "ratio_to_model": round(other / (1e6 * model / bw), 3), "halted": halted}), flush=True)
    # the rotation kernel against GmOpCombine launches, alternating, in this process
    for keep in (8, 16, 30):
        a, b = [], []
        for _ in range(2):
            a.append(cycles(op, reps, nev, 40, 1, keep=keep, window=0)[2])
            b.append(cycles(op, reps, nev, 40, 1, keep=keep, window=1)[2])
        ra, rb = min(a), min(b)
        ma, mb = 1e6 * rotation_model_bytes(n, 40, keep) / bw, 1e6 * composed_model_bytes(n, 40, keep) / bw
        print(json.dumps({"matrix": name, "rows": n, "rotation": "40 -> %d columns" % keep, "kernel_us": round(ra, 1),
                          "kernel_model_us": round(ma, 1), "composed_us": round(rb, 1), "composed_model_us": round(mb, 1),
                          "composed_over_kernel": round(rb / ra, 2) if ra else None}), flush=True)
    return op, spmv, bw


def host_line(name, op, reps):
    "The host part of a cycle at the largest basis: the Jacobi iteration grows with ncv^3."
    for m in (40, 128):
        cyc, host, rot, keep, sweeps, _ = cycles(op, max(3, reps // 3), 4, m, 1)
        print(json.dumps({"matrix": name, "ncv": m, "keep": keep, "host_part_ms": round(host / 1e3, 3), "jacobi_sweeps": sweeps,
                          "cycle_ms": round(cyc / 1e3, 3), "rotation_ms": round(rot / 1e3, 3)}), flush=True)


def solve_lines(name, op, matvec_max, reltol=1e-8, nev=4, ncv=40):
    from pykrylov_amd import ThickRestartLanczos, _lib
    lib = _lib.init()
    for which in ("LA", "SA"):
        s = ThickRestartLanczos(op, abstol=0.0, reltol=reltol)
        _lib.check(lib.mk_sync())
        t0 = time.perf_counter()
        s.solve(nev, which=which, ncv=ncv, matvec_max=matvec_max)
        _lib.check(lib.mk_sync())
        dt = time.perf_counter() - t0
        print(json.dumps({"solve": name, "which": which, "nev": nev, "ncv": ncv, "reltol": reltol, "products": int(s.nMatvec),
                          "cycles": int(s.cycles), "converged": bool(s.converged), "nconv": int(s.nconv),
                          "residNorm": float(s.residNorm), "threshold": float(s.threshold), "w": [float(v) for v in s.w],
                          "solve_s": round(dt, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small matrix only")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--matvec-max", type=int, default=20000, help="the cap of the solves to 1e-8")
    a = ap.parse_args()
    from pykrylov_amd import gallery
    sizes = [("poisson2d(100)", lambda: gallery.poisson2d(100))] if a.quick else \
        [("poisson2d(1024), n = 2^20", lambda: gallery.poisson2d(1024)), ("poisson3d(256), n = 2^24", lambda: gallery.poisson3d(256))]
    for name, make in sizes:
        op, _, _ = step_lines(name, make, a.reps)
        host_line(name, op, a.reps)
        solve_lines(name, op, a.matvec_max)
        op.free()


if __name__ == "__main__":
    main()
