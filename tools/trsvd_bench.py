"""Device thick-restart SVD (pykrylov_amd.ThickRestartSVD, csrc/mk_trsvd.hip): time per bidiagonalisation step in both
reorthogonalisation modes on tall random matrices (2^22 x 2^20 and 2^24 x 2^22, four entries per row, built on the host) and
on poisson2d(1024), against the byte model of DESIGN.md 3.17 at the bandwidth a plain device-to-device copy reaches in the
same run; the rotation of both bases; the host part of a cycle at ncv = 20, 40 and 128; and time and products to
reltol = 1e-8 for the 4 largest singular values.  One JSON line per measurement.

    python tools/trsvd_bench.py [--quick] [--reps 6] [--matvec-max 20000] [--skip-large]

A sample is one whole cycle (ncv - keep steps, the download, the small SVD on the host, the upload and the two rotations)
enqueued by one `iterate` call and timed by the HIP events around it; the first cycle of a run, which takes ncv steps, is left
out.  The library reports the host part of each cycle (mk_solver_history2) and the device time of the last rotation of both
bases (mk_result.aux[7]); what remains of a cycle is its steps.  Report, not a test: nothing is asserted.
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
KT = 16                                                          # output columns per rotation launch


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


def tall_random(R, C, per=4, seed=1):
    """R x C with `per` entries per row, one in each of `per` equal bands of columns (sorted, no duplicates), values in
    [-0.5, 0.5)."""
    from pykrylov_amd import CsrOperator
    rng = np.random.default_rng(seed)
    band = C // per
    cols = (rng.integers(0, band, size=(R, per), dtype=np.int64) + band * np.arange(per, dtype=np.int64)[None, :]).astype(np.int32)
    vals = rng.random((R, per)) - 0.5
    indptr = np.arange(0, (R + 1) * per, per, dtype=np.int64)
    return CsrOperator(indptr, cols.reshape(-1), vals.reshape(-1), (R, C))


def orth_bytes(j, n):
    "D, U, D, U against j columns of n entries: 2 (16 j + 24 ceil(j / G)) n."
    return 2 * (16 * j + 24 * -(-j // GROUP)) * n


def steps_model_bytes(R, C, m, keep, full):
    """Bytes of the steps keep + 1 .. m beyond their two plain products.  V side, step j: the orthogonalisation against j
    columns and the scaling (16 C).  U side: the scaling (16 R) and, full: the orthogonalisation against j - 1 columns;
    one-sided: 8 R for u_{j-1} in the product's epilogue, and in the first step the arrow over `keep` columns."""
    total = 0
    for j in range(keep + 1, m + 1):
        total += orth_bytes(j, C) + 16 * C + 16 * R
        if full:
            total += orth_bytes(j - 1, R)
        elif j == keep + 1:
            total += (8 * keep + 16 * -(-keep // GROUP)) * R
        else:
            total += 8 * R
    return total


def rotation_model_bytes(R, C, m, kk):
    "Per basis of n rows: 8 n (m ceil(kk / KT) + kk), and 16 n per column copied down from the spare columns."
    g = -(-kk // KT)
    return (R + C) * (8 * (m * g + kk) + 16 * KT * (g - 1))


def cycles(tall, wide, reps, nsv, ncv, full, keep=0):
    """Medians over `reps` cycles behind the first: (cycle us, host part us, rotation us, keep, sweeps, halted)."""
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    cyc, host, rot = [], [], []
    with DeviceRun(tall, _lib.MK_TRSVD, None, transpose=wide, abstol=0.0, reltol=0.0, matvec_max=1 << 40, reorth=int(full),
                   eig=(nsv, ncv, 1, keep, 1)) as run:
        run.setup()
        run.iterate(1)                                           # (code objects, the storage formats, the full first cycle)
        for _ in range(reps):
            run.iterate(1)
            cyc.append(1e3 * run.timing()["iterate_ms"])
            res = run.finish()
            rot.append(1e3 * res.aux[7])
            host.append(1e3 * run.history2()[-1])
        keep, sweeps, halted = int(res.aux[2]), int(res.istop), bool(res.halted)
    return float(np.median(cyc)), float(np.median(host)), float(np.median(rot)), keep, sweeps, halted


def step_lines(name, tall, wide, reps, ncvs=(20, 40), nsv=4):
    from pykrylov_amd import _lib
    lib = _lib.init()
    R, C = tall.shape
    rng = np.random.default_rng(0)
    dc, dr = _lib.DeviceArray.from_numpy(rng.standard_normal(C)), _lib.DeviceArray.from_numpy(rng.standard_normal(R))
    dr2 = _lib.DeviceArray(R)
    pa = median_us(lambda: tall.spmv_device(dc.ptr, dr2.ptr), reps, 20)
    pt = median_us(lambda: wide.spmv_device(dr.ptr, dc.ptr), reps, 20)
    copy = median_us(lambda: _lib.check(lib.mk_memcpy_d2d(dr2.ptr, dr.ptr, 8 * R)), reps, 20)
    bw = 16.0 * R / (copy * 1e-6)                                # bytes per second of a plain copy: 8 R in, 8 R out
    for d in (dc, dr, dr2):
        d.free()
    for m in ncvs:
        per_step = {}
        for full in (1, 0):
            cyc, host, rot, keep, sweeps, halted = cycles(tall, wide, reps, nsv, m, full)
            steps = m - keep
            model = steps_model_bytes(R, C, m, keep, full)
            other = cyc - host - rot - steps * (pa + pt)
            per_step[full] = (cyc - host - rot) / steps
            print(json.dumps({"matrix": name, "rows": R, "cols": C, "ncv": m, "keep": keep,
                              "reorth": "full" if full else "one-sided", "product_A_us": round(pa, 2),
                              "product_At_us": round(pt, 2), "copy_TBps": round(bw / 1e12, 3), "cycle_us": round(cyc, 1),
                              "host_part_us": round(host, 1), "rotation_us": round(rot, 1),
                              "rotation_model_us": round(1e6 * rotation_model_bytes(R, C, m, keep) / bw, 1),
                              "jacobi_sweeps": sweeps, "step_us": round(per_step[full], 2),
                              "beyond_products_us": round(other, 1), "model_us_at_copy_rate": round(1e6 * model / bw, 1),
                              "ratio_to_model": round(other / (1e6 * model / bw), 3), "halted": halted}), flush=True)
        print(json.dumps({"matrix": name, "ncv": m, "step_us_full": round(per_step[1], 2),
                          "step_us_one_sided": round(per_step[0], 2),
                          "one_sided_over_full": round(per_step[0] / per_step[1], 3)}), flush=True)


def host_lines(name, tall, wide, reps):
    "The host part of a cycle: the Jacobi iteration grows with ncv^3."
    for m in (20, 40, 128):
        if m >= tall.shape[1]:
            continue
        cyc, host, rot, keep, sweeps, _ = cycles(tall, wide, max(3, reps // 2), 4, m, 0)
        print(json.dumps({"matrix": name, "ncv": m, "keep": keep, "host_part_ms": round(host / 1e3, 3), "jacobi_sweeps": sweeps,
                          "cycle_ms": round(cyc / 1e3, 3), "rotation_ms": round(rot / 1e3, 3)}), flush=True)


def solve_lines(name, op, matvec_max, reltol=1e-8, nsv=4, ncv=40):
    from pykrylov_amd import ThickRestartSVD, _lib
    lib = _lib.init()
    for reorth in ("full", "one-sided"):
        s = ThickRestartSVD(op, abstol=0.0, reltol=reltol)
        _lib.check(lib.mk_sync())
        t0 = time.perf_counter()
        s.solve(nsv, which="LM", ncv=ncv, matvec_max=matvec_max, reorth=reorth)
        _lib.check(lib.mk_sync())
        dt = time.perf_counter() - t0
        print(json.dumps({"solve": name, "which": "LM", "reorth": reorth, "nsv": nsv, "ncv": ncv, "reltol": reltol,
                          "products": int(s.nMatvec), "cycles": int(s.cycles), "converged": bool(s.converged),
                          "nconv": int(s.nconv), "residNorm": float(s.residNorm), "threshold": float(s.threshold),
                          "s": [float(v) for v in s.s], "workspace_MB": round(s.workspace_bytes / 2 ** 20, 1),
                          "solve_s": round(dt, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small matrix only")
    ap.add_argument("--skip-large", action="store_true", help="leave the 2^24 x 2^22 matrix out")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--matvec-max", type=int, default=20000,
                    help="the cap of the solves to 1e-8 (at most 4000 on a matrix of more than 2^22 rows)")
    a = ap.parse_args()
    from pykrylov_amd import gallery
    if a.quick:
        sizes = [("random 4096 x 1024", lambda: tall_random(4096, 1024))]
    else:
        sizes = [("random 2^22 x 2^20", lambda: tall_random(1 << 22, 1 << 20))]
        if not a.skip_large:
            sizes.append(("random 2^24 x 2^22", lambda: tall_random(1 << 24, 1 << 22)))
        sizes.append(("poisson2d(1024), n = 2^20", lambda: gallery.poisson2d(1024)))
    for name, make in sizes:
        t0 = time.perf_counter()
        op = make()
        wide = op.T
        print(json.dumps({"matrix": name, "build_s": round(time.perf_counter() - t0, 2)}), flush=True)
        step_lines(name, op, wide, a.reps)
        host_lines(name, op, wide, a.reps)
        solve_lines(name, op, a.matvec_max if op.shape[0] <= 1 << 22 else min(a.matvec_max, 4000))
        if wide is not op:
            wide.free()
        op.free()


if __name__ == "__main__":
    main()
