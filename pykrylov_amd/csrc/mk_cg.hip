// mk_cg.hip -- conjugate gradients, device resident.   Reference: pykrylov/cg/cg.py:46-165.
//
// One pass of the reference loop (cg.py:113-158) = three kernels:
//   K1  Ap = A p ; partial sums of <p, Ap>                          (cg.py:115-117)
//   K2  alpha = ry / pAp ; r += alpha Ap ; partial sums of <r, r>                  (cg.py:119-127,131,146)
//   K3  x += alpha p ; beta = ry' / ry ; p = beta p - r ; residNorm, history, loop test
//                                                                                  (cg.py:130,149-158, :113)
// The x update rides in K3 because K3 streams p anyway (x is not read by anything in between and K3 always
// runs when K2 did), which saves one pass over p.  Same operations on the same values: results are unchanged.
// Algorithmic traffic per pass: B_spmv + (16n read + 8n write) + (24n read + 16n write)
//   = B_spmv + 64n bytes (the reference's op count gives B_spmv + 104n).
//
// FUSED passes (round 5; storage format 9, one GPU): K3's vector work moves into the NEXT pass's product kernel --
//   K1f  x += alpha p_old ; p = beta p_old - r ; Ap = A p ; partial sums of <p, Ap>   (cg.py:130,150-151 of the pass before,
//        then cg.py:115-117): the brick march of mk_spmv_fmt9.h loads the own rows of p_old, r and x once, forms p and x,
//        writes p to the OTHER p buffer (neighbouring bricks still read p_old for their halo rows) and x in place
//   K2   unchanged
//   K3s  one workgroup: beta, residNorm, history, loop test (the prologue of K3, nothing else); marks the update pending
// -- same operations on the same values in the same order per element, so every bit of x, p, r and of the history is
// the bit of the three-kernel pass.  Traffic per pass: (48n read/write in K1f) + 24n instead of 16n + 24n + 40n: one
// sweep over p less.  The update of the LAST pass is applied when the loop has halted (mk_solver_x / _vector / finish:
// `materialize`); a caller that looks at x between passes gets x + alpha p formed into a scratch vector.
//
// DEFERRED x (MK_CG_XDEFER = m > 1): x is an accumulator that nothing in the loop reads, so K1f leaves it alone (p_old, r in;
// p, Ap out) and the directions stay where the products wrote them, in a ring of m + 1 buffers (pass k writes slot
// k % (m + 1)); K2 keeps alpha_k in a ring of the scalar file.  After every m-th pass -- and at the end of every
// mk_solver_iterate call, before its closing event, so that a timed call contains the applications of its own passes --
// `cg_xapply` sweeps x once: x = fl(x + fl(alpha_k p_k)) for the pending k in order, in registers, each step rounded on its
// own: the bits of m sweeps.  x costs 16 n / m + 8 n bytes per pass instead of 16 n.
#include "mk_solver.h"
#include "mk_cg_epi.h"
#include "mk_ringdepth.h"

namespace {

enum { S_RY0 = 0, S_RY1 = 1, S_THRESH = 2, S_RESID = 3, S_RESID0 = 4, S_PAP = 5, S_ALPHA = 6, S_BETA = 7, S_PENDING = 8,
       S_ARING = 32 };                                     // alpha of pass k at S_ARING + k % (m + 1) (deferred x)
static_assert(S_ARING + MK_XD_MAX + 1 <= MK_NSCAL, "the alpha ring lives in the scalar file");

// K1: the product epilogue CgSpmvEpiT<NTY> lives in mk_cg_epi.h (PCG, mk_pcg.hip, launches the same product kernels)

// K1f: the brick march's "fuse" hooks (mk_spmv_fmt9.h).  Only ever launched on a plain march matrix (formats 9 / 10 / 11):
// MARCH_ONLY keeps the generic launcher from compiling any other kernel for them.
constexpr int MK_FUSE_NT_ALL = 7;                            // 1 nt loads of x, 2 nt stores of x, 4 nt stores of the new p (profiles/r05_fuse_nt_ab.txt: all three)
template <bool NTY, bool FX = true>
struct CgFusedEpiT {
    static constexpr int NACC = 1, SLOT0 = 0;
    static constexpr bool SYM_MARCH = true;
    static constexpr bool FUSE_X = FX;                       // false: x stays out of the kernel (deferred, cg_xapply)
    static constexpr bool MARCH_ONLY = true;                 // only the march kernels are compiled for it (mk_device.h)
    static constexpr int FUSE_NT = NTY ? MK_FUSE_NT_ALL : 0;  // vectors beyond the Infinity Cache: x / the new p past the caches too
    double *Ap;
    const double *fuse_r;
    double *fuse_x, *fuse_p, *fuse_dump;
    double *scal;
    double fa, fb;
    __device__ void prologue(double *) {
        fa = scal[S_ALPHA];                                // alpha and beta of the pass before (K2 / K3s)
        fb = scal[S_BETA];
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[S_PENDING] = 0.0;     // this kernel applies the pending update
    }
    __device__ double xin(double v) const { return v; }
    __device__ double fuse_pnew(double po, double rv) const { return fb * po - rv; }       // cg.py:150-151
    __device__ double fuse_xnew(double xv, double po) const { return xv + fa * po; }       // cg.py:130
    __device__ void row(int64_t r, double s, double *) { Ap[r] = s; }                      // (never run: see above)
    __device__ void row_x(int64_t r, double s, double xr, double *acc) {
        if constexpr (NTY) __builtin_nontemporal_store(s, Ap + r);
        else Ap[r] = s;
        acc[0] += xr * s;
    }
    __device__ void row2_m(int64_t r, mk_d2 s, mk_d2 xr, bool oka, bool okb, double *dump, double *acc) {   // (as CgSpmvEpiT's)
        mk_d2u *d = reinterpret_cast<mk_d2u *>(okb ? Ap + r : dump);
        if constexpr (NTY) __builtin_nontemporal_store(s, d);
        else *d = s;
        if (oka && !okb) Ap[r] = s.x;
        const double ta = xr.x * s.x, tb = xr.y * s.y;
        acc[0] += oka ? ta : 0.0;
        acc[0] += okb ? tb : 0.0;
    }
};

// K3s: the scalar part of K3 (CgUpdateXP::prologue), one workgroup
__global__ __launch_bounds__(MK_BLOCK) void cg_beta_kernel(const double *part, int np, double *scal, MkStatus *st, double *hist,
                                                           int par, int64_t matvec_max, MkHalt halt) {
    __shared__ double s4[4];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double ry_next = mk_total(part + MK_MAXP, np, s4);
    if (threadIdx.x == 0) {
        const double ry = scal[S_RY0 + par];
        const double beta = ry_next / ry;                 // cg.py:149
        const double resid = fabs(__dsqrt_rn(ry_next));   // cg.py:154
        const bool go = (resid > scal[S_THRESH]) && (st->nMatvec < matvec_max);   // cg.py:113
        scal[S_RY0 + (par ^ 1)] = ry_next;                // cg.py:153
        scal[S_RESID] = resid;
        scal[S_BETA] = beta;
        scal[S_PENDING] = 1.0;                            // x += alpha p ; p = beta p - r of this pass are still to be applied
        hist[st->hist_len % MK_HIST_RING] = resid;        // cg.py:155
        st->hist_len += 1;
        st->itn += 1;
        halt.out(!go);
    }
}

// the pending update of the last pass, outside the halt protocol: in place once the loop has halted, into scratch
// vectors for a caller that looks at the iterate between passes
__global__ __launch_bounds__(MK_BLOCK) void cg_flush_kernel(int64_t n, const double *scal, const double *r, const double *p,
                                                            const double *x, double *p_out, double *x_out) {
    const bool pend = scal[S_PENDING] != 0.0;
    const double alpha = scal[S_ALPHA], beta = scal[S_BETA];
    for (int64_t i = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MK_BLOCK) {
        const double pv = p[i];
        if (x_out) {                                      // (null: x is deferred, cg_xapply has it)
            const double xv = x[i];
            x_out[i] = pend ? xv + alpha * pv : xv;       // cg.py:130
        }
        p_out[i] = pend ? beta * pv - r[i] : pv;          // cg.py:150-151
    }
}

// Deferred x: x += alpha_k p_k (cg.py:130) for the passes k in [lo, hi) in order, one sweep over x, 16 bytes per lane.  `hi` is
// what the host enqueued; the passes the DEVICE completed decide (st->itn: a pass stopped by the curvature test applies
// nothing, cg.py:119-124, and passes enqueued behind a halt never ran).  Outside the halt protocol: it reads only what no
// concurrent workgroup writes, and a range that was applied is never asked for again (the host's `x_applied`).
struct CgXRing {
    const double *p[MK_XD_MAX + 1];
};
template <bool NT>
__device__ __forceinline__ mk_d2 cg_ld2(const double *v, int64_t i) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const mk_d2 *>(v + i));
    else return *reinterpret_cast<const mk_d2 *>(v + i);
}
template <bool NT>
__global__ __launch_bounds__(MK_BLOCK) void cg_xapply_kernel(int64_t n, const double *scal, const MkStatus *st, CgXRing ring, int R,
                                                             int64_t lo, int64_t hi, double *x) {
    const int64_t done = st->itn;
    if (hi > done) hi = done;
    if (lo >= hi) return;
    const int64_t S = (int64_t)gridDim.x * MK_BLOCK, g = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x, npair = n >> 1;
    for (int64_t q = g; q < npair; q += S) {
        mk_d2 xv = cg_ld2<NT>(x, 2 * q);
        int64_t k = lo;
        for (; k + 4 <= hi; k += 4) {                     // four directions in flight (uniform trip counts)
            mk_d2 pv[4];
            double a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int s = (int)((k + u) % R);
                pv[u] = cg_ld2<NT>(ring.p[s], 2 * q);
                a[u] = scal[S_ARING + s];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                xv.x = xv.x + a[u] * pv[u].x;
                xv.y = xv.y + a[u] * pv[u].y;
            }
        }
        for (; k < hi; ++k) {
            const int s = (int)(k % R);
            const mk_d2 pv = cg_ld2<NT>(ring.p[s], 2 * q);
            const double a = scal[S_ARING + s];
            xv.x = xv.x + a * pv.x;
            xv.y = xv.y + a * pv.y;
        }
        if constexpr (NT) __builtin_nontemporal_store(xv, reinterpret_cast<mk_d2 *>(x + 2 * q));
        else *reinterpret_cast<mk_d2 *>(x + 2 * q) = xv;
    }
    if ((n & 1) && g == (npair % S)) {
        double xv = x[n - 1];
        for (int64_t k = lo; k < hi; ++k) xv = xv + scal[S_ARING + (int)(k % R)] * ring.p[(int)(k % R)][n - 1];
        x[n - 1] = xv;
    }
}

struct CgUpdateR {
    static constexpr int NACC = 1, SLOT0 = 1;
    const double *part;
    int np;
    double *scal;
    MkStatus *st;
    int par, check_curv;
    const double *Ap;
    double *r;
    const double *dg;                                     // preconditioner diagonal or null
    double alpha;
    bool bad;
    MkTotalRegs tr;
    double ry_in;
    double *aslot = nullptr;                              // deferred x: where alpha of this pass is kept for cg_xapply
    __device__ void early() {
        mk_total_issue(part, np, tr);
        ry_in = scal[S_RY0 + par];
    }
    __device__ bool prologue(double *s4, bool lead) {
        const double pAp = mk_total_finish(tr, np, s4);
        const double ry = ry_in;
        bad = check_curv && (pAp <= 0.0);                 // cg.py:119-124
        alpha = ry / pAp;                                 // cg.py:127
        if (lead) {
            st->nMatvec += 1;                             // cg.py:116
            scal[S_PAP] = pAp;
            scal[S_ALPHA] = alpha;
            if (aslot) *aslot = alpha;
            if (bad) st->definite = 0;
        }
        return bad;
    }
    __device__ bool skip() const { return bad; }
    struct Regs {
        double2 av, rv, dv;
    };
    __device__ void load2(int64_t i, Regs &g) const {
        g.av = mk_ld2(Ap, i);
        g.rv = mk_ld2(r, i);
        if (dg) g.dv = mk_ld2(dg, i);
    }
    __device__ void apply2(Regs &g, double *acc) const {
        g.rv.x = g.rv.x + alpha * g.av.x;                 // cg.py:131
        g.rv.y = g.rv.y + alpha * g.av.y;
        if (dg) {                                         // y = precon * r ; <r, y>   cg.py:137-138,146
            acc[0] += g.rv.x * (g.dv.x * g.rv.x);
            acc[0] += g.rv.y * (g.dv.y * g.rv.y);
        } else {
            acc[0] += g.rv.x * g.rv.x;                    // cg.py:146
            acc[0] += g.rv.y * g.rv.y;
        }
    }
    __device__ void store2(int64_t i, const Regs &g) const { mk_st2(r, i, g.rv); }
    __device__ void one(int64_t i, double *acc) {
        const double rv = r[i] + alpha * Ap[i];
        r[i] = rv;
        acc[0] += dg ? rv * (dg[i] * rv) : rv * rv;
    }
};

struct CgUpdateXP {
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *part;
    int np;
    double *scal;
    MkStatus *st;
    double *hist;
    int par;
    int64_t matvec_max;
    const double *r;
    double *p, *x;
    double alpha, beta;
    MkTotalRegs tr;
    double ry_in, thresh_in;
    int64_t nmv_in;
    __device__ void early() {
        mk_total_issue(part + MK_MAXP, np, tr);
        ry_in = scal[S_RY0 + par];
        alpha = scal[S_ALPHA];                            // written by K2 of this pass
        thresh_in = scal[S_THRESH];
        nmv_in = st->nMatvec;
    }
    __device__ bool prologue(double *s4, bool lead) {
        const double ry_next = mk_total_finish(tr, np, s4);
        const double ry = ry_in;
        beta = ry_next / ry;                              // cg.py:149
        const double resid = fabs(__dsqrt_rn(ry_next));   // cg.py:154
        const bool go = (resid > thresh_in) && (nmv_in < matvec_max);   // cg.py:113
        if (lead) {
            scal[S_RY0 + (par ^ 1)] = ry_next;            // cg.py:153
            scal[S_RESID] = resid;
            hist[st->hist_len % MK_HIST_RING] = resid;    // cg.py:155
            st->hist_len += 1;
            st->itn += 1;
        }
        return !go;
    }
    __device__ bool skip() const { return false; }
    struct Regs {
        double2 rv, pv, xv;
    };
    __device__ void load2(int64_t i, Regs &g) const {
        g.rv = mk_ld2(r, i);
        g.pv = mk_ld2(p, i);
        g.xv = mk_ld2(x, i);
    }
    __device__ void apply2(Regs &g, double *) const {
        g.xv.x = g.xv.x + alpha * g.pv.x;                 // cg.py:130 (with the p of this pass)
        g.xv.y = g.xv.y + alpha * g.pv.y;
        g.pv.x = beta * g.pv.x - g.rv.x;                  // cg.py:150-151 (p *= beta; p -= r)
        g.pv.y = beta * g.pv.y - g.rv.y;
    }
    __device__ void store2(int64_t i, const Regs &g) const {
        mk_st2(x, i, g.xv);
        mk_st2(p, i, g.pv);
    }
    __device__ void one(int64_t i, double *) {
        const double pv = p[i];
        x[i] = x[i] + alpha * pv;
        p[i] = beta * pv - r[i];
    }
};

// everything between the initial <r, y> and the loop header (cg.py:99-113)
__global__ __launch_bounds__(MK_BLOCK) void cg_init_kernel(const double *part, int np, double *scal, MkStatus *st,
                                                           double *hist, MkHalt halt, double abstol, double reltol,
                                                           int64_t matvec_max, int64_t nmv0) {
    __shared__ double s4[4];
    const double ry = mk_total(part + MK_MAXP, np, s4);
    if (threadIdx.x == 0) {
        const double resid0 = fabs(__dsqrt_rn(ry));
        const double rel = reltol * resid0;
        const double thresh = (rel > abstol) ? rel : abstol;   // max(abstol, reltol*residNorm0)
        scal[S_RY0] = ry;
        scal[S_THRESH] = thresh;
        scal[S_RESID] = resid0;
        scal[S_RESID0] = resid0;
        hist[0] = resid0;
        st->hist_len = 1;
        st->nMatvec = nmv0;
        st->itn = 0;
        st->definite = 1;
        scal[S_PENDING] = 0.0;
        halt.out(!((resid0 > thresh) && (nmv0 < matvec_max)));
    }
}

struct CgSolver : mk_solver {
    double *d_x = nullptr, *d_r = nullptr, *d_p = nullptr, *d_Ap = nullptr;
    // fused passes (see the top of the file)
    bool fused = false;
    double *d_dump = nullptr;                             // the dump rows of the brick march
    // the direction buffers: ring[0] = d_p; fused passes use the first m + 1 (m = xdefer; 1: the pair that alternates).  Each has
    // nx entries: a slab keeps the neighbours' planes of the direction behind the own rows
    std::vector<double *> ring;
    int xdefer = 1;                                       // m of this solve: x is swept once per m passes (1: inside K1f)
    int setups_done = 0;                                  // set-ups that chose a depth so far (mk_params_ring: a bound for the first k)
    mutable int64_t x_applied = 0;                        // deferred x: directions [0, x_applied) have been asked to be applied
    mutable double *d_xv = nullptr, *d_pv = nullptr;      // the iterate / direction as a caller sees them between passes
    mutable bool flushed = false;
    int64_t nmv0 = 0;                                     // products before the loop (the initial guess's)
    double *pbuf(int64_t k) const { return fused ? ring[(size_t)(k % (xdefer + 1))] : d_p; }     // p of pass k
    // the buffer of the direction in use: product k WROTE pbuf(k), and the passes the host enqueued behind a halt never ran,
    // so the products the DEVICE counted decide (K2 counts one per product, cg.py:116), not the host's pass counter
    double *pcur() const {
        CgSolver *me = const_cast<CgSolver *>(this);
        if (!fused || !is_setup) return d_p;
        if (hipMemcpyAsync(me->h_status, d_status, sizeof(MkStatus), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return d_p;
        const int64_t done = h_status->nMatvec - nmv0;
        return done > 0 ? pbuf(done - 1) : d_p;
    }

    static bool want_fuse() {
        return mk_switch_int<MK_SW_CG_FUSE>() != 0;        // (read at every setup: tests switch it between solves)
    }
    // MK_CG_XDEFER = m (read at every setup like MK_CG_FUSE).  Unset: the rule of mk_ringdepth.h -- 1 where the vectors stay in the
    // Infinity Cache (the deferral saves HBM traffic and costs one kernel boundary per m passes, so a problem whose x stays in
    // the cache has nothing to gain from it), beyond that the deepest ring the memory rule serves.  The caller's
    // bound (mk_params_ring: a placement search holds several solvers at once and probes them at one depth) caps either.
    int want_xdefer() const {
        static_assert(mk_switch_table[MK_SW_CG_XDEFER].hi == MK_XD_MAX, "the ring holds at most MK_XD_MAX + 1 directions");
        const MkSwitchVal m = mk_switch<MK_SW_CG_XDEFER>();
        const int cap = (ring_cap > 0 && (ring_cap_setups == 0 || setups_done < ring_cap_setups)) ? ring_cap : MK_XD_MAX;
        if (m.set) return (int)m.v < cap ? (int)m.v : cap;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
            (void)hipGetLastError();
            fr = 0;
        }
        return mk_ring_depth(sizeof(double) * (size_t)n, fr, (int)ring.size(), cap);
    }
    // grow the ring towards m + 1 buffers; returns the m it can serve (0: not even the pair of today's fused pass).  The buffers
    // beyond the pair may take an eighth of the device memory that is free (mk_ring_fit): a placement search holds several
    // solvers at once.  Only ever called from setup(): pbuf() ties the slot of the current direction to m.
    int ring_reserve(int m) {
        const size_t bytes = sizeof(double) * (size_t)nx;
        if ((int)ring.size() < m + 1 && m > 1) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
                (void)hipGetLastError();
                fr = 0;
            }
            const int fit = mk_ring_fit(bytes, fr, (int)ring.size());
            const int have = (int)ring.size() - 1;
            m = m < fit ? m : (fit > have ? fit : have);     // (what the ring holds already is never given up)
        }
        while ((int)ring.size() < m + 1) {
            double *v = nullptr;
            if (alloc_vec(&v, nx) != MK_OK) {
                (void)hipGetLastError();                     // (reported by the fall-back, not by the next launch check)
                break;
            }
            ring.push_back(v);
        }
        const int got = (int)ring.size() - 1;
        return got < m ? got : m;
    }
    // deferred x: enqueue the application of the directions [x_applied, hi) -- clamped on the device to the passes it completed
    void enqueue_xapply(int64_t hi) const {
        if (hi <= x_applied) return;
        CgXRing rg{};
        const int R = xdefer + 1;
        for (int k = 0; k < R; ++k) rg.p[k] = ring[(size_t)k];
        const int grid = mk_grid_stream(n);
        if (mk_store_nt(A))
            hipLaunchKernelGGL(cg_xapply_kernel<true>, dim3(grid), dim3(MK_BLOCK), 0, stream, n, d_scal, d_status, rg, R, x_applied, hi, d_x);
        else
            hipLaunchKernelGGL(cg_xapply_kernel<false>, dim3(grid), dim3(MK_BLOCK), 0, stream, n, d_scal, d_status, rg, R, x_applied, hi, d_x);
        x_applied = hi;
    }
    // apply (halted) or form (running) the pending x / p update; returns the vectors a caller may read
    void materialize(const double **xo, const double **po) const {
        CgSolver *me = const_cast<CgSolver *>(this);
        *xo = d_x;
        double *pc = pcur();
        *po = pc;
        if (!fused || it == 0 || !is_setup) return;
        const int grid = (int)((n + MK_BLOCK - 1) / MK_BLOCK > 2048 ? 2048 : (n + MK_BLOCK - 1) / MK_BLOCK);
        // deferred x: whatever is still to be applied goes into x itself, running or halted -- x is an accumulator the loop never
        // reads, and every direction is applied once, in order (after an iterate call nothing is left: `drain`)
        const bool defer = xdefer > 1;
        if (defer) enqueue_xapply(it);
        if (halted) {
            if (!flushed) {
                hipLaunchKernelGGL(cg_flush_kernel, dim3(grid), dim3(MK_BLOCK), 0, stream, n, d_scal, d_r, pc, d_x, pc, defer ? nullptr : d_x);
                hipMemsetAsync(d_scal + S_PENDING, 0, sizeof(double), stream);
                me->flushed = true;
            }
            return;
        }
        if (!d_pv && me->alloc_vec(&me->d_pv, n) != MK_OK) return;
        if (!defer && !d_xv && me->alloc_vec(&me->d_xv, n) != MK_OK) return;
        hipLaunchKernelGGL(cg_flush_kernel, dim3(grid), dim3(MK_BLOCK), 0, stream, n, d_scal, d_r, pc, d_x, d_pv, defer ? nullptr : d_xv);
        if (!defer) *xo = d_xv;
        *po = d_pv;
    }
    int drain() override {                                  // end of an iterate call: the applications of its own passes
        if (fused && xdefer > 1) enqueue_xapply(it);
        return MK_OK;
    }
    int64_t unapplied() const override {                    // completed passes (as of the last poll) whose direction is not in x yet
        if (!fused || !is_setup) return 0;
        if (xdefer > 1) return h_status->itn > x_applied ? h_status->itn - x_applied : 0;
        return (h_scal[S_PENDING] != 0.0 && !flushed) ? 1 : 0;
    }

    int setup(const double *rhs, const double *guess) override {
        int rc_alloc = MK_OK;
        // (r with room for received entries too: fused passes on a slab exchange r's boundary planes, not p's; each vector is
        //  allocated where it is still missing: a set-up that failed half way is repeated from where it stopped)
        if (!d_x) rc_alloc = alloc_vec(&d_x, nx);
        if (rc_alloc == MK_OK && !d_r) rc_alloc = alloc_vec(&d_r, nx);
        if (rc_alloc == MK_OK && !d_p && (rc_alloc = alloc_vec(&d_p, nx)) == MK_OK) ring.assign(1, d_p);
        if (rc_alloc == MK_OK && !d_Ap) rc_alloc = alloc_vec(&d_Ap, n);
        if (rc_alloc != MK_OK) {
            // the other ranks are on their way into the veto all-reduce below: vote before leaving
            if (mk_comm_active()) {
                double veto = 1.0;
                mk_comm_allreduce_host(&veto, 1);
            }
            return rc_alloc;
        }
        const MkPlan *plan = A ? mk_csr_plan(A) : nullptr;
        // one device, or one rank's slab under a halo exchange (the march takes the neighbours' planes from the received entries)
        const bool slab = plan && A->ex.mode == 0 && nx == n + A->ex.n_halo && (plan->pen_xlo >= 0 || plan->pen_xhi >= 0);
        fused = want_fuse() && plan && mk_fmt_march(plan->fmt) && !general_precon() && A->nops == 0 && !A->comp_kind &&
                ((!mk_comm_active() && A->ex.mode < 0 && nx == n) || slab);
        flushed = false;
        x_applied = 0;
        xdefer = 1;
        if (fused && !d_dump && alloc_vec(&d_dump, (int64_t)MK_MAXP * 1024) != MK_OK) {
            (void)hipGetLastError();
            d_dump = nullptr;
            fused = false;
        }
        if (fused) {
            xdefer = ring_reserve(want_xdefer());           // (a ring that cannot be had: a smaller m, down to today's pair)
            if (xdefer < 1) {
                xdefer = 1;
                fused = false;
            }
        }
        setups_done += 1;
        if (mk_comm_active()) {
            // The choice changes what travels: fused ranks exchange r's boundary planes and form the neighbours' p themselves,
            // the others exchange p -- messages of the same size, so a disagreement would neither hang nor fail, it would
            // multiply by the wrong vector.  (Ranks can differ: a slab one plane thinner falls below the march's row
            // threshold, an allocation fails on one of them.)  So all ranks fuse, or none does.
            double veto = fused ? 0.0 : 1.0;
            int rc = mk_comm_allreduce_host(&veto, 1);
            if (rc != MK_OK) return rc;
            if (veto != 0.0) fused = false;
        }
        nmv0 = 0;
        mk_launch_stream(this, MkOpNegCopy{rhs, d_r}, n);                   // r = -rhs          cg.py:85
        if (guess) {
            MK_HIP(hipMemcpyAsync(d_x, guess, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
            int rc = exchange(d_x);
            if (rc != MK_OK) return rc;
            mk_launch_spmv(this, d_x, MkPlainEpi{d_Ap}, false);             // r += A x          cg.py:86-88
            mk_launch_stream(this, MkOpAddTo<1>{d_Ap, d_r}, n);
            nmv0 = 1;
        } else {
            MK_HIP(hipMemsetAsync(d_x, 0, sizeof(double) * (size_t)nx, stream));
        }
        if (d_prec()) {
            mk_launch_stream(this, MkOpMul{d_prec(), d_r, d_Ap}, n);          // y = precon * r    cg.py:91-92
            if (general_precon() && apply_precon(d_r, d_Ap) != MK_OK) return MK_ERR_STATE;
            mk_launch_stream(this, MkOpDot<1>{d_r, d_Ap}, n);               // ry = <r, y>       cg.py:99
        } else {
            mk_launch_stream(this, MkOpDot<1>{d_r, d_r}, n);                // ry = <r, r>       cg.py:99
        }
        int rc = allreduce(1, 1);
        if (rc != MK_OK) return rc;
        hipLaunchKernelGGL(cg_init_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, d_part, np_stream, d_scal, d_status,
                           d_hist, next_halt(), prm.abstol, prm.reltol, prm.matvec_max, nmv0);
        mk_launch_stream(this, MkOpNegCopy{d_r, d_p}, n);                   // p = -r            cg.py:104
        return MK_OK;
    }

    int enqueue_spmv_only(int which) override {
        if (which != 0) return mk_fail(MK_ERR_ARG, "CG has one product per pass");
        if (fused && it > 0) {
            // the fused kernel exactly as a pass launches it (same streams: p_old, r in; p, Ap out; with m = 1 x in and out too,
            // updated again with the same alpha), except that p goes to the ring slot behind the one it came from -- after an
            // iterate call every direction has been applied (`drain`), so no slot holds one that x still needs -- timing
            // only, after the run
            double *pc = pcur(), *po = ring[0];
            for (int k = 0; k <= xdefer; ++k)
                if (ring[(size_t)k] == pc) po = ring[(size_t)((k + 1) % (xdefer + 1))];
            launch_fused(pc, po, false);
            return MK_OK;
        }
        if (A && mk_store_nt(A)) mk_launch_spmv(this, d_p, CgSpmvEpiT<true>{d_p, d_Ap, 0.0}, false);
        else mk_launch_spmv(this, d_p, CgSpmvEpi{d_p, d_Ap, 0.0}, false);
        return MK_OK;
    }

    // K1f on p_old = `po`, the new p into `pn`: with x (m = 1) or without (deferred)
    void launch_fused(const double *po, double *pn, bool timed) {
        const bool nt = mk_store_nt(A);
        if (xdefer > 1) {
            if (nt) mk_launch_spmv(this, po, CgFusedEpiT<true, false>{d_Ap, d_r, d_x, pn, d_dump, d_scal, 0.0, 0.0}, timed);
            else mk_launch_spmv(this, po, CgFusedEpiT<false, false>{d_Ap, d_r, d_x, pn, d_dump, d_scal, 0.0, 0.0}, timed);
        } else {
            if (nt) mk_launch_spmv(this, po, CgFusedEpiT<true>{d_Ap, d_r, d_x, pn, d_dump, d_scal, 0.0, 0.0}, timed);
            else mk_launch_spmv(this, po, CgFusedEpiT<false>{d_Ap, d_r, d_x, pn, d_dump, d_scal, 0.0, 0.0}, timed);
        }
    }

    int enqueue_pass() override {
        const int par = (int)(it & 1);
        int rc;
        if (fused) {
            const bool nt = mk_store_nt(A);
            if (it == 0) {                                  // nothing pending yet: the plain product on p = -r
                if ((rc = exchange(d_p)) != MK_OK) return rc;
                if (nt) mk_launch_spmv(this, d_p, CgSpmvEpiT<true>{d_p, d_Ap, 0.0});
                else mk_launch_spmv(this, d_p, CgSpmvEpi{d_p, d_Ap, 0.0});
            } else {                                        // K1f: p_old = the other buffer
                // a slab: the neighbours' planes of p are FORMED here like the own ones, from their p_old (kept behind the own rows
                // of the p buffers since the pass before) and their r -- so it is r whose boundary planes travel, as soon as K2 of
                // the pass before has written them; the interior planes' launch overlaps the messages as everywhere
                if ((rc = exchange(d_r)) != MK_OK) return rc;
                launch_fused(pbuf(it - 1), pbuf(it), true);
            }
            if ((rc = allreduce(0, 1)) != MK_OK) return rc;
            CgUpdateR k2{d_part, np_spmv, d_scal, d_status, par, prm.check_curvature, d_Ap, d_r, d_prec(), 0.0, false};
            if (xdefer > 1) k2.aslot = d_scal + S_ARING + (int)(it % (xdefer + 1));
            mk_launch_stream(this, k2, n);
            if ((rc = allreduce(1, 1)) != MK_OK) return rc;
            hipLaunchKernelGGL(cg_beta_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, d_part, np_stream, d_scal, d_status, d_hist,
                               par, prm.matvec_max, next_halt());
            // deferred x: pass `it` has put the m-th direction into the ring -- one sweep over x applies them, before pass
            // it + 1 writes the slot of the oldest
            if (xdefer > 1 && it + 1 - x_applied >= xdefer) enqueue_xapply(it + 1);
            return MK_OK;
        }
        rc = exchange(d_p);
        if (rc != MK_OK) return rc;
        if (A && mk_store_nt(A)) mk_launch_spmv(this, d_p, CgSpmvEpiT<true>{d_p, d_Ap, 0.0});
        else mk_launch_spmv(this, d_p, CgSpmvEpi{d_p, d_Ap, 0.0});
        if ((rc = allreduce(0, 1)) != MK_OK) return rc;
        mk_launch_stream(this, CgUpdateR{d_part, np_spmv, d_scal, d_status, par, prm.check_curvature, d_Ap, d_r,
                                         d_prec(), 0.0, false}, n);
        if (general_precon()) {                             // y = precon * r ; <r, y> re-formed   cg.py:137-138,146
            if ((rc = apply_precon(d_r, d_Ap)) != MK_OK) return rc;
            mk_launch_stream(this, MkOpDot<1>{d_r, d_Ap}, n);
        }
        if ((rc = allreduce(1, 1)) != MK_OK) return rc;
        mk_launch_stream(this, CgUpdateXP{d_part, np_stream, d_scal, d_status, d_hist, par, prm.matvec_max, d_r, d_p,
                                          d_x, 0.0, 0.0}, n);
        return MK_OK;
    }

    int finish(mk_result *res) override {
        int rc = poll();
        if (rc != MK_OK) return rc;
        fill_result(res);
        res->residNorm = h_scal[S_RESID];
        res->residNorm0 = h_scal[S_RESID0];
        res->threshold = h_scal[S_THRESH];
        res->converged = (h_scal[S_RESID] <= h_scal[S_THRESH]) ? 1 : 0;     // cg.py:161
        res->aux[0] = h_scal[S_PAP];
        res->aux[1] = fused ? (double)xdefer : 0.0;          // the ring depth m this set-up chose (0: three-kernel passes)
        return MK_OK;
    }

    const double *x() const override {
        const double *xo, *po;
        materialize(&xo, &po);
        return xo;
    }
    const double *vector(int i) const override {
        if (i == 0) return d_r;
        if (i != 1) return nullptr;
        const double *xo, *po;
        materialize(&xo, &po);
        return po;
    }
    bool is_fused() const override { return fused; }
    // The search direction is built from r, not from y = precon*r, exactly as cg.py:104,150-151 do.
    bool takes_precon() const override { return true; }
};

}  // namespace

mk_solver *mk_make_cg() { return new CgSolver(); }
