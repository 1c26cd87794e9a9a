#!/usr/bin/env python3
"""Timings of the device L-BFGS operator (DESIGN.md, section on L-BFGS):

  * one apply (npairs = 5, full ring, scaling on) at n = 10^6 and n = 2^24, device vectors in and out: median over `reps`
    batches of back-to-back applies, host clock around stream synchronisations, and the implied bytes per second against
    the byte model of the chain as built, (64 p + 8) n bytes out of place;
  * the same apply through the host route (``H * v`` on a NumPy vector: upload, chain, download), per application;
  * one CG solve on poisson2d(1000) with ``precon=H`` on the device against ``precon=Shell(H)`` (host callback).

    python tools/lbfgs_bench.py [--reps 20] [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Shell(object):
    def __init__(self, H):
        self.H, self.calls = H, 0

    def __mul__(self, x):
        self.calls += 1
        return self.H * x


def median_ms(fn, sync, reps, batch):
    for _ in range(3):
        fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(batch):
            fn()
        sync()
        out.append(1e3 * (time.perf_counter() - t0) / batch)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    import pykrylov_amd
    from pykrylov_amd import _lib, gallery
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    lib = _lib.init()
    sync = lambda: _lib.check(lib.mk_sync())     # noqa: E731
    rows, p = [], 5
    for n in (10 ** 6, 2 ** 24):
        rng = np.random.default_rng(1)
        H = pykrylov_amd.InverseLBFGSOperator(n, p, scaling=True)
        for _ in range(p):
            s = rng.standard_normal(n)
            assert H.store(s, s * (1.0 + rng.random(n)) + 0.01 * rng.standard_normal(n))
        v = rng.standard_normal(n)
        d_in, d_out = _lib.DeviceArray.from_numpy(v), _lib.DeviceArray(n)
        batch = 10 if n <= 10 ** 6 else 4
        med, lo, hi = median_ms(lambda: H.apply_device(d_in, d_out), sync, reps, batch)
        model = (64 * p + 8) * n
        host = median_ms(lambda: H * v, sync, reps, 1)
        rows.append({"what": "apply", "n": n, "npairs": p, "launches": H.info["launches_last_apply"], "reps": reps,
                     "batch": batch, "ms_median": med, "ms_min": lo, "ms_max": hi, "model_bytes": model,
                     "model_TBps": model / (med * 1e-3) / 1e12, "host_route_ms_median": host[0]})
        print(json.dumps(rows[-1]), flush=True)
        d_in.free()
        d_out.free()
        H.free()
    op = gallery.poisson2d(1000)
    n = op.shape[0]
    rng = np.random.default_rng(8)
    H = pykrylov_amd.InverseLBFGSOperator(n, p, scaling=True)
    for _ in range(p):
        s = rng.standard_normal(n)
        assert H.store(s, op * s)
    rhs = op * np.ones(n)
    for name, precon in (("device", H), ("host callback", Shell(H)), ("device", H), ("host callback", Shell(H))):
        solver = pykrylov_amd.CG(op, precon=precon, reltol=1e-8)
        sync()
        t0 = time.perf_counter()
        solver.solve(rhs, matvec_max=400)
        sync()
        rows.append({"what": "cg poisson2d(1000)", "precon": name, "seconds": time.perf_counter() - t0,
                     "nMatvec": int(solver.nMatvec), "residNorm": float(solver.residNorm),
                     "callbacks": getattr(precon, "calls", 0)})
        print(json.dumps(rows[-1]), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
