"""Device LOBPCG (pykrylov_amd.LOBPCG, csrc/mk_lobpcg.hip): time per iteration at n = 2^20 and 2^24 for nev = 4, block = 8,
with and without `tools.amg`, split into products, preconditioner, Gram matrices, rotations and the host part, against the byte
model of DESIGN.md 3.16 at the bandwidth a plain device-to-device copy reaches in the same run; the Gram kernel against the same
Gram matrices composed of GmOpMultiDot launches; and time and products to reltol = 1e-8.  One JSON line per measurement.

    python tools/lobpcg_bench.py [--quick] [--reps 10] [--matvec-max 20000] [--matvec-max-large 4000]

A sample is one whole iteration enqueued by one `iterate` call and timed by the HIP events around it, with every column active
(reltol = 0: nothing is ever locked); the first two iterations of a run, which have no P yet or load code objects, are left out.
The library reports the device time of the phases of the last iteration (mk_result: Acond the two Gram matrices, Arnorm the
preconditioner, ynorm the products, xnorm the rotations with the scaling of P and the residuals) and the host part
(mk_solver_history2); what remains is the orthogonalisation of W and the two synchronisations.  Report, not a test: nothing is
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

GROUP = 8                                                        # columns of X per launch (GM_GROUP)
TILE = 8                                                         # the Gram kernel's tile at these column counts


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


def gram_model_bytes(n, m, tile=TILE):
    "Two Gram matrices: per tile on or above the diagonal 2 * tile columns read."
    nt = -(-m // tile)
    return 2 * (nt * (nt + 1) // 2) * 2 * tile * 8 * n


def composed_gram_model_bytes(n, m):
    "Two Gram matrices of GmOpMultiDot launches: column j against the columns 0 .. j, 1 + min(G, rest) columns per launch."
    cols = sum(-(-(j + 1) // GROUP) + (j + 1) for j in range(m))
    return 2 * cols * 8 * n


def iteration_model_bytes(n, nb, na, precon):
    """Beyond the products and the preconditioner, m = nb + 2 na: W (a copy: 2 na columns, none with a general
    preconditioner), O (per column and pass: nb + g reads of the dots, nb + 2 g of the updates; then the scaling), G, R
    (X and AX: m in, nb out, twice; P and AP: m - nb in, na out, twice), N (per column 1 + 4), E (2 nb in, nb out)."""
    m, g = nb + 2 * na, -(-nb // GROUP)
    cols = (0 if precon else 2 * na) + na * (2 * (2 * nb + 3 * g) + 2) + 2 * (m + nb) + 2 * (m - nb + na) + 5 * na + 3 * nb
    return cols * 8 * n + gram_model_bytes(n, m)


def iterations(op, reps, nev, nb, precon=None):
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun, resolve_precon
    payload = resolve_precon(precon, op.shape[0], 'precon', 'LOBPCG')[1]
    rows = []
    with DeviceRun(op, _lib.MK_LOBPCG, None, precon_diag=payload, abstol=0.0, reltol=0.0, matvec_max=1 << 40,
                   eig=(nev, nb, 0, 0, 1)) as run:
        run.setup()
        run.iterate(2)
        for _ in range(reps):
            run.iterate(1)
            res = run.finish()
            rows.append((1e3 * run.timing()["iterate_ms"], 1e3 * run.history2()[-1], 1e3 * res.Acond, 1e3 * res.Arnorm,
                         1e3 * res.ynorm, 1e3 * res.xnorm, res.aux[2], res.aux[6]))
        halted = bool(res.halted)
    med = [float(np.median([r[k] for r in rows])) for k in range(8)]
    return med, halted


def iteration_lines(name, make, reps, nev=4, nb=8):
    from pykrylov_amd import _lib, tools
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
    t0 = time.perf_counter()
    M = tools.amg(op)
    _lib.check(lib.mk_sync())
    amg_s = time.perf_counter() - t0
    for label, precon in (("none", None), ("amg", M)):
        (it, host, gram, pre, prod, rot, na, sweeps), halted = iterations(op, reps, nev, nb, precon)
        na = int(na)
        model = iteration_model_bytes(n, nb, na, precon is not None)
        gmodel = gram_model_bytes(n, nb + 2 * na)
        beyond = it - prod - pre - host
        print(json.dumps({"matrix": name, "rows": n, "nev": nev, "block": nb, "active": na, "precon": label,
                          "plain_product_us": round(spmv, 2), "copy_TBps": round(bw / 1e12, 3), "iteration_us": round(it, 1),
                          "products_us": round(prod, 1), "preconditioner_us": round(pre, 1), "gram_us": round(gram, 1),
                          "gram_model_us": round(1e6 * gmodel / bw, 1), "rotation_scale_residual_us": round(rot, 1),
                          "host_part_us": round(host, 1), "jacobi_sweeps": int(sweeps),
                          "orthogonalisation_and_syncs_us": round(it - prod - pre - host - gram - rot, 1),
                          "beyond_products_precon_host_us": round(beyond, 1), "model_us_at_copy_rate": round(1e6 * model / bw, 1),
                          "ratio_to_model": round(beyond / (1e6 * model / bw), 3), "halted": halted}), flush=True)
    return op, M, bw, amg_s


def gram_lines(name, op, bw, reps):
    "The Gram kernel (8 x 8 and 4 x 4 tiles) against GmOpMultiDot launches: the probe of the solver kind, alternating."
    from pykrylov_amd import _lib
    from pykrylov_amd.generic import DeviceRun
    n = op.shape[0]
    for m in (16, 24, 48):
        us = {8: [], 4: [], 1: []}
        for _ in range(max(3, reps // 2)):
            for window in (8, 4, 1):
                with DeviceRun(op, _lib.MK_LOBPCG, None, abstol=0.0, reltol=0.0, matvec_max=1, restart=1, window=window,
                               eig=(1, m, 0, 0, 1)) as run:
                    run.setup()
                    run.setup()                                  # (the second: the code objects are loaded)
                    us[window].append(1e3 * run.finish().aux[7])
        k8, k4, comp = (float(np.median(us[w])) for w in (8, 4, 1))
        print(json.dumps({"matrix": name, "rows": n, "gram": "2 matrices of %d x %d" % (m, m), "tile8_us": round(k8, 1),
                          "tile8_model_us": round(1e6 * gram_model_bytes(n, m, 8) / bw, 1), "tile4_us": round(k4, 1),
                          "tile4_model_us": round(1e6 * gram_model_bytes(n, m, 4) / bw, 1), "composed_us": round(comp, 1),
                          "composed_model_us": round(1e6 * composed_gram_model_bytes(n, m) / bw, 1),
                          "composed_over_tile8": round(comp / k8, 2) if k8 else None}), flush=True)


def solve_lines(name, op, M, amg_s, matvec_max, reltol=1e-8, nev=4, nb=8):
    from pykrylov_amd import LOBPCG, _lib
    lib = _lib.init()
    for label, precon in (("amg", M), ("none", None)):
        s = LOBPCG(op, abstol=0.0, reltol=reltol, precon=precon)
        _lib.check(lib.mk_sync())
        t0 = time.perf_counter()
        s.solve(nev, which="SA", block=nb, matvec_max=matvec_max)
        _lib.check(lib.mk_sync())
        dt = time.perf_counter() - t0
        print(json.dumps({"solve": name, "which": "SA", "nev": nev, "block": nb, "precon": label, "reltol": reltol,
                          "products": int(s.nMatvec), "iterations": int(s.nIter), "converged": bool(s.converged),
                          "nconv": int(s.nconv), "restarts": int(s.restarts), "residNorm": float(s.residNorm),
                          "threshold": float(s.threshold), "anorm": float(s.anorm), "w": [float(v) for v in s.w],
                          "solve_s": round(dt, 4), "amg_setup_s": round(amg_s, 3) if precon is not None else 0.0}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small matrix only")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--matvec-max", type=int, default=20000, help="the cap of the solves to 1e-8 at n = 2^20")
    ap.add_argument("--matvec-max-large", type=int, default=4000, help="... and at n = 2^24")
    a = ap.parse_args()
    from pykrylov_amd import gallery
    sizes = [("poisson2d(100)", lambda: gallery.poisson2d(100), a.matvec_max)] if a.quick else \
        [("poisson2d(1024), n = 2^20", lambda: gallery.poisson2d(1024), a.matvec_max),
         ("poisson3d(256), n = 2^24", lambda: gallery.poisson3d(256), a.matvec_max_large)]
    for name, make, cap in sizes:
        op, M, bw, amg_s = iteration_lines(name, make, a.reps)
        gram_lines(name, op, bw, a.reps)
        solve_lines(name, op, M, amg_s, cap)
        M.free()
        op.free()


if __name__ == "__main__":
    main()
