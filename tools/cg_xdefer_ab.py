"""A/B of CG's deferred x update (MK_CG_XDEFER = m, csrc/mk_cg.hip) through the C ABI, ONE matrix in ONE process: for every m a
solver object of its own (the knob is read at set-up), visited round robin; per m the median pass time over the rounds, the
pass's TRUE physical bytes and what fraction of 8 TB/s that is, and the device memory the ring holds.

    python tools/cg_xdefer_ab.py [const|varcoef] [side] [rounds] [passes]        (defaults: const 512 5 96)

Physical bytes per pass (n rows, 8-byte entries): product kernel = matrix + p_old, r in + p, Ap out (32 n; with m = 1 also x
in and out: 48 n), r update 24 n, x sweep 8 n + 16 n / m (with m = 1: inside the product kernel).  Matrix: format 9 one byte
per row (+ a dictionary), format 11 one byte + 32 bytes per row."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pykrylov_amd import _lib, gallery
from pykrylov_amd.generic import DeviceRun

lib = _lib.init(0)
wl = sys.argv[1] if len(sys.argv) > 1 else "const"
side = int(sys.argv[2]) if len(sys.argv) > 2 else 512
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
passes = int(sys.argv[4]) if len(sys.argv) > 4 else 96          # a multiple of every m below: whole rings inside a timing
ms_list = [int(v) for v in os.environ.get("AB_MS", "1,2,4,8,16,32").split(",")]

op = gallery.poisson3d(side) if wl == "const" else gallery.poisson3d_varcoef(side)
n = op.shape[0]
ones = _lib.DeviceArray.from_numpy(np.ones(n))
rhs = _lib.DeviceArray(n)
op.spmv_device(ones.ptr, rhs.ptr)
matrix_bytes = n * (1 if wl == "const" else 33)

# the deepest ring first: every ring takes at most an eighth of the memory that is free at ITS set-up (csrc/mk_ringdepth.h), and
# 31 GiB beyond the pair (m = 32 at 512^3) is an eighth of nearly the whole device; `got`: the depth each object was given
runs, got = {}, {}
for m in sorted(ms_list, reverse=True):
    os.environ["MK_CG_XDEFER"] = str(m)
    os.environ["MK_PLACEMENT_DRAWS"] = "1"                       # (one object per m: the A/B is between them)
    run = DeviceRun(op, _lib.MK_CG, rhs, None, abstol=0.0, reltol=0.0, matvec_max=1 << 60, check_curvature=1)
    run.setup()
    run.iterate(16)
    runs[m], got[m] = run, int(run.finish().aux[1])

t = {m: [] for m in ms_list}
for r in range(rounds):
    for m in ms_list:
        _lib.check(lib.mk_sync())
        t0 = time.perf_counter()
        done = runs[m].iterate(passes)
        _lib.check(lib.mk_sync())
        assert done == passes and (m == 1 or runs[m].unapplied() == 0)
        t[m].append(1e3 * (time.perf_counter() - t0) / passes)

print("workload %s %d^3, n = %d, %d rounds of %d passes; medians (min .. max)" % (wl, side, n, rounds, passes))
print("%3s  %21s  %8s  %10s  %9s  %s" % ("m", "ms per pass", "it/s", "GB / pass", "of 8 TB/s", "ring memory"))
for want in ms_list:
    a = np.array(t[want])
    m = got[want]
    if m != want:
        print("(m = %d asked for, %d served: no memory for a deeper ring)" % (want, m))
    byts = matrix_bytes + (32 + 24) * n + (16 * n if m == 1 else 8 * n + 16 * n / m)
    med = float(np.median(a))
    print("%3d  %6.3f (%6.3f .. %6.3f)  %8.1f  %10.3f  %9.3f  %.2f GB" % (m, med, a.min(), a.max(), 1e3 / med, byts / 1e9,
                                                                        byts / (med * 1e-3) / 8e12, (m + 1) * 8 * n / 1e9))
