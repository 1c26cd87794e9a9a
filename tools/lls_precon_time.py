#!/usr/bin/env python3
"""Milliseconds per pass of LSQR and LSMR with a device-resident N, on the device route against the same object forced
through the host callback:

  * the seeded 4e6 x 1e6 matrix of tests/test_gpu_lls_full_size.py (`--size full`) and the seeded 1537 x 1025 matrix of
    tests/test_gpu_lls_device_precon.py (`--size small`);
  * N = InverseLBFGSOperator(n, 5) with a full ring (`--precon lbfgs`) and N = ic0 of an SPD tridiagonal (`--precon ic0`).

A pass is timed as the difference of two whole solves stopped by their iteration budgets (`--passes k1,k2`, every tolerance
zero) over the difference of their pass counts: set-up, the matrix's transpose and the first launches cancel.  Host clock around solves that end in a
device synchronise (they download x).  One warm-up pair per configuration, then `--reps` repeats with the two routes
alternating; median, minimum and maximum of the per-pass time are reported, and the ratio of the medians.

    python tools/lls_precon_time.py [--size small|full|both] [--precon lbfgs|ic0|both] [--reps 5] [--passes 5,25] [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def small_matrix():
    m, n, per_row = 1537, 1025, 5
    rng = np.random.default_rng(7)
    rows = np.concatenate([np.repeat(np.arange(m), per_row), np.arange(n)])
    cols = np.concatenate([rng.integers(0, n, m * per_row), np.arange(n)])
    vals = np.concatenate([0.2 * rng.standard_normal(m * per_row), np.ones(n)])
    from oracle import csr_ref
    A = csr_ref.from_coo(rows, cols, vals, (m, n))
    return A.indptr, A.indices, A.data, (m, n)


def full_matrix():
    import bench
    m, n = 4000000, 1000000
    return bench.random_tall_csr(m, n) + ((m, n),)


def tridiagonal(n, seed):
    from pykrylov_amd import CsrOperator
    d = 2.0 + np.random.default_rng(seed).random(n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.full(n, 3) - (np.arange(n) == 0) - (np.arange(n) == n - 1))
    cols = np.stack([np.arange(n) - 1, np.arange(n), np.arange(n) + 1], axis=1).reshape(-1)
    vals = np.stack([np.full(n, -0.5), d, np.full(n, -0.5)], axis=1).reshape(-1)
    keep = (cols >= 0) & (cols < n)
    return CsrOperator(indptr, cols[keep], vals[keep], (n, n), symmetric=True)


def make_n(kind, n):
    import pykrylov_amd
    from pykrylov_amd import tools
    if kind == "lbfgs":
        rng = np.random.default_rng(1)
        H = pykrylov_amd.InverseLBFGSOperator(n, 5)
        for _ in range(5):
            s = rng.standard_normal(n)
            assert H.store(s, s * (1.0 + rng.random(n)) + 0.01 * rng.standard_normal(n))
        return H, [H]
    T = tridiagonal(n, 2)
    return tools.ic0(T), [T]


def solve_seconds(cls, op, b, N, passes):
    s = cls(op)
    t0 = time.perf_counter()
    ret = s.solve(b, itnlim=passes, atol=0.0, btol=0.0, conlim=0.0, etol=0.0, N=N)
    dt = time.perf_counter() - t0
    itn = s.itn if ret is None else ret[2]                   # (LSMR returns its results, like the reference)
    return dt, int(itn), s.precon_route["N"]


def main():
    from pykrylov_amd import CsrOperator, lls
    sizes = {"small": ["small"], "full": ["full"], "both": ["small", "full"]}[arg("--size", "both")]
    kinds = {"lbfgs": ["lbfgs"], "ic0": ["ic0"], "both": ["lbfgs", "ic0"]}[arg("--precon", "both")]
    reps = int(arg("--reps", "5"))
    k1, k2 = (int(t) for t in arg("--passes", "5,25").split(","))
    rows = []
    for size in sizes:
        indptr, indices, data, shape = small_matrix() if size == "small" else full_matrix()
        op = CsrOperator(indptr, indices, data, shape)
        b = op * np.ones(shape[1])
        for kind in kinds:
            N, owned = make_n(kind, shape[1])
            routes = (("device", N), ("host", lambda v, N=N: N * v))
            for name, cls in (("lsqr", lls.LSQRFramework), ("lsmr", lls.LSMRFramework)):
                per_pass = {"device": [], "host": []}
                for rep in range(reps + 1):                  # (the first pair warms every shape and both routes up)
                    for route, P in routes:
                        t1, n1, r1 = solve_seconds(cls, op, b, P, k1)
                        t2, n2, r2 = solve_seconds(cls, op, b, P, k2)
                        want = route if route == "host" else {"lbfgs": "lbfgs", "ic0": "ilu"}[kind]
                        assert r1 == r2 == want, (r1, r2, want)
                        assert n2 > n1, (n1, n2)             # (passes actually run: a solve may converge before k2)
                        if rep:
                            per_pass[route].append(1e3 * (t2 - t1) / (n2 - n1))
                row = {"solver": name, "shape": list(shape), "N": kind, "passes": [k1, k2], "reps": reps}
                for route in ("device", "host"):
                    v = per_pass[route]
                    row[route + "_ms_per_pass"] = {"median": float(np.median(v)), "min": float(np.min(v)),
                                                   "max": float(np.max(v))}
                row["host_over_device"] = row["host_ms_per_pass"]["median"] / row["device_ms_per_pass"]["median"]
                rows.append(row)
                print(json.dumps(row), flush=True)
            for o in [N] + owned:
                o.free()
        op.free()
    out = arg("--out", None)
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
