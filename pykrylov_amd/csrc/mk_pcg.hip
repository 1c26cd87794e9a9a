// mk_pcg.hip -- preconditioned conjugate gradients, device resident (solver kind MK_PCG; no reference module).
//
// CG (mk_cg.hip) reproduces the reference's recurrence, whose search direction is built from r and not from precon * r.  This
// is the textbook loop beside it: p = z + beta p with z = M r, beta = <r,z>' / <r,z> (standard) or, for a preconditioner
// that changes from call to call, beta = -alpha <q,z'> / <r,z> (flexible; = <z', r' - r> / <r,z> without storing the old r).
// The history holds 2-norms of the recurrence residual r of x itself.  Without a preconditioner every bit of x, of the
// history and of the counts is CG's: the two loops differ by the sign of r, and negation is exact.
//
// One pass, routes `none` and `diag` (M = a diagonal d, multiplied inside the kernels) -- CG's split into three kernels:
//   K1  q = A p ; partial sums of <p, q>                              (CG's product kernels, mk_cg_epi.h)
//   K2  alpha = rz / pq ; curvature test ; r -= alpha q ; partial sums of <r,r> [, <r, d r>] [, <q, d r> or <q, r>]
//   K3  ||r||, history, stop test ; rz' > 0 ? ; beta ; x += alpha p ; p = d r + beta p
// z is never stored: d r is formed in K2 and again in K3, with the same bits.  K3's x update also runs in the pass that halts.
// Traffic beyond the product: (16 n read + 8 n write) + (24 n read + 16 n write) = 64 n bytes, + 16 n for the diagonal.
//
// One pass, general routes (device matrix, ILU / IC, L-BFGS, Chebyshev, FSAI, AMG, host callback):
//   K1   as above
//   K2g  alpha ; curvature test ; x += alpha p ; r -= alpha q ; partial sums of <r,r>          32 n read + 16 n write
//   Kn   one workgroup: ||r||, history, stop test
//   M    z = M r by the preconditioner's own launches (no-ops once halted; the host callback is skipped by the halt word)
//   Kd   partial sums of <r,z> [and <q,z>]                                                    16 n [24 n] read
//   K3g  rz' > 0 ? ; beta ; p = z + beta p                                                    16 n read + 8 n write
// = 88 n bytes (flexible: 96 n) beside the product and the preconditioner.
#include "mk_solver.h"
#include "mk_cg_epi.h"

namespace {

enum { S_RZ0 = 0, S_RZ1 = 1, S_THRESH = 2, S_RESID = 3, S_RESID0 = 4, S_PQ = 5, S_ALPHA = 6, S_BETA = 7, S_BREAK = 8, S_FLEX = 9 };
// partial-sum slots: 0 <p,q> (the product kernel's), 1 <r,r>, 2 <r,z>, 3 <q,z>; without a preconditioner <r,z> is <r,r> and
// <q,z> = <q,r> takes slot 2
static_assert(MK_NDOT >= 4, "PCG keeps <p,q>, <r,r>, <r,z> and <q,z> in the solver's partial-sum slots");

__device__ __forceinline__ bool pcg_bad_rz(double rz) { return !(rz > 0.0) || !isfinite(rz); }

// alpha and the curvature test from the product's partial sums: the prologue of K2 and of K2g
struct PcgAlpha {
    const double *part;
    int np;
    double *scal;
    MkStatus *st;
    int par, check_curv;
    double alpha;
    bool bad;
    MkTotalRegs tr;
    double rz_in;
    __device__ void early() {
        mk_total_issue(part, np, tr);
        rz_in = scal[S_RZ0 + par];
    }
    __device__ bool prologue(double *s4, bool lead) {
        const double pq = mk_total_finish(tr, np, s4);
        bad = check_curv && !(pq > 0.0);
        alpha = rz_in / pq;
        if (lead) {
            st->nMatvec += 1;
            scal[S_PQ] = pq;
            scal[S_ALPHA] = alpha;
            if (bad) {                                    // x untouched, no history entry; p is the direction of no descent
                st->definite = 0;
                scal[S_BREAK] = 1.0;
            }
        }
        return bad;
    }
    __device__ bool skip() const { return bad; }
};

// K2: r -= alpha q with the sums the next direction needs.  DIAG: z = d r; FLEX: <q, z> too (z = r without a diagonal).
template <bool DIAG, bool FLEX>
struct PcgUpdateR : PcgAlpha {
    static constexpr int NACC = 1 + (DIAG ? 1 : 0) + (FLEX ? 1 : 0), SLOT0 = 1;
    const double *q;
    double *r;
    const double *dg;
    struct Regs {
        double2 qv, rv, dv;
    };
    __device__ void load2(int64_t i, Regs &g) const {
        g.qv = mk_ld2(q, i);
        g.rv = mk_ld2(r, i);
        if constexpr (DIAG) g.dv = mk_ld2(dg, i);
    }
    __device__ void apply2(Regs &g, double *acc) const {
        g.rv.x = g.rv.x - alpha * g.qv.x;
        g.rv.y = g.rv.y - alpha * g.qv.y;
        acc[0] += g.rv.x * g.rv.x;
        acc[0] += g.rv.y * g.rv.y;
        double2 zv = g.rv;
        if constexpr (DIAG) {
            zv.x = g.dv.x * g.rv.x;
            zv.y = g.dv.y * g.rv.y;
            acc[1] += g.rv.x * zv.x;
            acc[1] += g.rv.y * zv.y;
        }
        if constexpr (FLEX) {
            acc[NACC - 1] += g.qv.x * zv.x;
            acc[NACC - 1] += g.qv.y * zv.y;
        }
    }
    __device__ void store2(int64_t i, const Regs &g) const { mk_st2(r, i, g.rv); }
    __device__ void one(int64_t i, double *acc) {
        const double qv = q[i];
        const double rv = r[i] - alpha * qv;
        r[i] = rv;
        acc[0] += rv * rv;
        double zv = rv;
        if constexpr (DIAG) {
            zv = dg[i] * rv;
            acc[1] += rv * zv;
        }
        if constexpr (FLEX) acc[NACC - 1] += qv * zv;
    }
};

// what the stop test and the new direction share: everything a lane needs from the scalar file, read before the sums arrive
struct PcgStopIn {
    double rz, alpha, thresh;
    int64_t nmv;
};

// ||r||, history and the stop test from <r,r>; `lead` writes.  Returns true when the loop ends here.
__device__ __forceinline__ bool pcg_stop(double rr, const PcgStopIn &in, int64_t matvec_max, double *scal, MkStatus *st, double *hist,
                                         bool lead) {
    const double resid = __dsqrt_rn(rr);
    const bool stop = (resid <= in.thresh) || (in.nmv >= matvec_max);
    if (lead) {
        scal[S_RESID] = resid;
        hist[st->hist_len % MK_HIST_RING] = resid;
        st->hist_len += 1;
        st->itn += 1;
    }
    return stop;
}

// beta from <r,z>' (and <q,z>'); a <r,z>' that is not positive and finite ends the run with breakdown 2
__device__ __forceinline__ bool pcg_beta(double rz_new, double qz, bool flex, const PcgStopIn &in, int par, double *scal, bool lead,
                                         double *beta) {
    if (pcg_bad_rz(rz_new)) {
        if (lead) scal[S_BREAK] = 2.0;
        return true;
    }
    *beta = flex ? -(in.alpha * qz) / in.rz : rz_new / in.rz;
    if (lead) {
        scal[S_RZ0 + (par ^ 1)] = rz_new;
        scal[S_BETA] = *beta;
    }
    return false;
}

// K3: x += alpha p (also in the pass that halts) ; p = d r + beta p (only when the loop goes on)
template <bool DIAG, bool FLEX>
struct PcgUpdateXP {
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
    const double *dg;
    double alpha, beta;
    bool go;
    MkTotalRegs t_rr, t_rz, t_qz;
    PcgStopIn in;
    __device__ void early() {
        mk_total_issue(part + MK_MAXP, np, t_rr);
        if constexpr (DIAG) mk_total_issue(part + 2 * MK_MAXP, np, t_rz);
        if constexpr (FLEX) mk_total_issue(part + (DIAG ? 3 : 2) * MK_MAXP, np, t_qz);
        in.rz = scal[S_RZ0 + par];
        in.alpha = scal[S_ALPHA];                         // written by K2 of this pass
        in.thresh = scal[S_THRESH];
        in.nmv = st->nMatvec;
    }
    __device__ bool prologue(double *s4, bool lead) {
        const double rr = mk_total_finish(t_rr, np, s4);
        double rz_new = rr, qz = 0.0;
        if constexpr (DIAG) rz_new = mk_total_finish(t_rz, np, s4);
        if constexpr (FLEX) qz = mk_total_finish(t_qz, np, s4);
        alpha = in.alpha;
        beta = 0.0;
        bool stop = pcg_stop(rr, in, matvec_max, scal, st, hist, lead);
        if (!stop) stop = pcg_beta(rz_new, qz, FLEX, in, par, scal, lead, &beta);
        go = !stop;
        return stop;
    }
    __device__ bool skip() const { return false; }
    struct Regs {
        double2 rv, pv, xv, dv;
    };
    __device__ void load2(int64_t i, Regs &g) const {
        g.rv = mk_ld2(r, i);
        g.pv = mk_ld2(p, i);
        g.xv = mk_ld2(x, i);
        if constexpr (DIAG) g.dv = mk_ld2(dg, i);
    }
    __device__ void apply2(Regs &g, double *) const {
        g.xv.x = g.xv.x + alpha * g.pv.x;
        g.xv.y = g.xv.y + alpha * g.pv.y;
        double2 zv = g.rv;
        if constexpr (DIAG) {
            zv.x = g.dv.x * g.rv.x;
            zv.y = g.dv.y * g.rv.y;
        }
        g.pv.x = zv.x + beta * g.pv.x;
        g.pv.y = zv.y + beta * g.pv.y;
    }
    __device__ void store2(int64_t i, const Regs &g) const {
        mk_st2(x, i, g.xv);
        if (go) mk_st2(p, i, g.pv);
    }
    __device__ void one(int64_t i, double *) {
        const double pv = p[i];
        x[i] = x[i] + alpha * pv;
        if (go) {
            double zv = r[i];
            if constexpr (DIAG) zv = dg[i] * zv;
            p[i] = zv + beta * pv;
        }
    }
};

// K2g: x += alpha p ; r -= alpha q ; partial sums of <r,r>
struct PcgUpdateXR : PcgAlpha {
    static constexpr int NACC = 1, SLOT0 = 1;
    const double *q, *p;
    double *r, *x;
    struct Regs {
        double2 qv, rv, pv, xv;
    };
    __device__ void load2(int64_t i, Regs &g) const {
        g.qv = mk_ld2(q, i);
        g.rv = mk_ld2(r, i);
        g.pv = mk_ld2(p, i);
        g.xv = mk_ld2(x, i);
    }
    __device__ void apply2(Regs &g, double *acc) const {
        g.xv.x = g.xv.x + alpha * g.pv.x;
        g.xv.y = g.xv.y + alpha * g.pv.y;
        g.rv.x = g.rv.x - alpha * g.qv.x;
        g.rv.y = g.rv.y - alpha * g.qv.y;
        acc[0] += g.rv.x * g.rv.x;
        acc[0] += g.rv.y * g.rv.y;
    }
    __device__ void store2(int64_t i, const Regs &g) const {
        mk_st2(x, i, g.xv);
        mk_st2(r, i, g.rv);
    }
    __device__ void one(int64_t i, double *acc) {
        x[i] = x[i] + alpha * p[i];
        const double rv = r[i] - alpha * q[i];
        r[i] = rv;
        acc[0] += rv * rv;
    }
};

// Kd: partial sums of <r,z> into slot 2 and, FLEX, of <q,z> into slot 3
template <bool FLEX>
struct PcgDotZ {
    static constexpr int NACC = FLEX ? 2 : 1, SLOT0 = 2;
    const double *r, *z, *q;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        const double2 rv = mk_ld2(r, i), zv = mk_ld2(z, i);
        acc[0] += rv.x * zv.x;
        acc[0] += rv.y * zv.y;
        if constexpr (FLEX) {
            const double2 qv = mk_ld2(q, i);
            acc[1] += qv.x * zv.x;
            acc[1] += qv.y * zv.y;
        }
    }
    __device__ void one(int64_t i, double *acc) {
        acc[0] += r[i] * z[i];
        if constexpr (FLEX) acc[1] += q[i] * z[i];
    }
};

// K3g: rz' > 0 ? ; beta ; p = z + beta p
struct PcgUpdateP {
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *part;
    int np;
    double *scal;
    int par, flex;
    const double *z;
    double *p;
    double beta;
    bool bad;
    MkTotalRegs t_rz, t_qz;
    PcgStopIn in;
    __device__ void early() {
        mk_total_issue(part + 2 * MK_MAXP, np, t_rz);
        if (flex) mk_total_issue(part + 3 * MK_MAXP, np, t_qz);
        in.rz = scal[S_RZ0 + par];
        in.alpha = scal[S_ALPHA];
    }
    __device__ bool prologue(double *s4, bool lead) {
        const double rz_new = mk_total_finish(t_rz, np, s4);
        const double qz = flex ? mk_total_finish(t_qz, np, s4) : 0.0;
        beta = 0.0;
        bad = pcg_beta(rz_new, qz, flex != 0, in, par, scal, lead, &beta);
        return bad;
    }
    __device__ bool skip() const { return bad; }
    struct Regs {
        double2 zv, pv;
    };
    __device__ void load2(int64_t i, Regs &g) const {
        g.zv = mk_ld2(z, i);
        g.pv = mk_ld2(p, i);
    }
    __device__ void apply2(Regs &g, double *) const {
        g.pv.x = g.zv.x + beta * g.pv.x;
        g.pv.y = g.zv.y + beta * g.pv.y;
    }
    __device__ void store2(int64_t i, const Regs &g) const { mk_st2(p, i, g.pv); }
    __device__ void one(int64_t i, double *) { p[i] = z[i] + beta * p[i]; }
};

// Kn: ||r|| from <r,r> (slot 1), one workgroup.  first: the set-up (threshold, history[0], the status record); otherwise the
// stop test of a pass of the general routes.
__global__ __launch_bounds__(MK_BLOCK) void pcg_norm_kernel(const double *part, int np, double *scal, MkStatus *st, double *hist,
                                                            MkHalt halt, int first, int rz_is_rr, int flex, double abstol,
                                                            double reltol, int64_t matvec_max, int64_t nmv0) {
    __shared__ double s4[4];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double rr = mk_total(part + MK_MAXP, np, s4);
    if (threadIdx.x != 0) return;
    if (!first) {
        PcgStopIn in{};
        in.thresh = scal[S_THRESH];
        in.nmv = st->nMatvec;
        halt.out(pcg_stop(rr, in, matvec_max, scal, st, hist, true));
        return;
    }
    const double resid0 = __dsqrt_rn(rr);
    const double rel = reltol * resid0;
    const double thresh = (rel > abstol) ? rel : abstol;
    scal[S_THRESH] = thresh;
    scal[S_RESID] = resid0;
    scal[S_RESID0] = resid0;
    scal[S_FLEX] = (double)flex;
    hist[0] = resid0;
    st->hist_len = 1;
    st->nMatvec = nmv0;
    st->itn = 0;
    st->definite = 1;
    bool stop = (resid0 <= thresh) || (nmv0 >= matvec_max);
    if (!stop && rz_is_rr) {                              // no preconditioner: z = r, <r,z> = <r,r>, no second dot
        stop = pcg_bad_rz(rr);
        if (stop) scal[S_BREAK] = 2.0;
        else scal[S_RZ0] = rr;
    }
    halt.out(stop);
}

// the set-up's <r,z> (slot 2) with a preconditioner, one workgroup
__global__ __launch_bounds__(MK_BLOCK) void pcg_rz0_kernel(const double *part, int np, double *scal, MkHalt halt) {
    __shared__ double s4[4];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double rz = mk_total(part + 2 * MK_MAXP, np, s4);
    if (threadIdx.x != 0) return;
    const bool bad = pcg_bad_rz(rz);
    if (bad) scal[S_BREAK] = 2.0;
    else scal[S_RZ0] = rz;
    halt.out(bad);
}

struct PcgSolver : mk_solver {
    double *d_x = nullptr, *d_r = nullptr, *d_p = nullptr, *d_q = nullptr, *d_z = nullptr;
    int flexible = 0;
    bool allocated = false;
    int64_t nmv0 = 0;
    bool takes_precon() const override { return true; }

    template <class Op>
    void launch_product(const Op &epi, bool timed) { mk_launch_spmv(this, d_p, epi, timed); }
    void product(bool timed) {                              // K1, with CG's choice of the non-temporal variant
        if (A && mk_store_nt(A)) launch_product(CgSpmvEpiT<true>{d_p, d_q, 0.0}, timed);
        else launch_product(CgSpmvEpi{d_p, d_q, 0.0}, timed);
    }

    PcgAlpha alpha_in(int par) const {
        PcgAlpha a{};
        a.part = d_part;
        a.np = np_spmv;
        a.scal = d_scal;
        a.st = d_status;
        a.par = par;
        a.check_curv = prm.check_curvature;
        return a;
    }
    template <bool DIAG, bool FLEX>
    void launch_k23(int par) {
        PcgUpdateR<DIAG, FLEX> k2{};
        static_cast<PcgAlpha &>(k2) = alpha_in(par);
        k2.q = d_q;
        k2.r = d_r;
        k2.dg = d_prec();
        mk_launch_stream(this, k2, n);
        PcgUpdateXP<DIAG, FLEX> k3{};
        k3.part = d_part;
        k3.np = np_stream;
        k3.scal = d_scal;
        k3.st = d_status;
        k3.hist = d_hist;
        k3.par = par;
        k3.matvec_max = prm.matvec_max;
        k3.r = d_r;
        k3.p = d_p;
        k3.x = d_x;
        k3.dg = d_prec();
        mk_launch_stream(this, k3, n);
    }
    void launch_norm(int first) {
        hipLaunchKernelGGL(pcg_norm_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, d_part, np_stream, d_scal, d_status, d_hist,
                           next_halt(), first, slot[0].kind == MK_PRECON_NONE ? 1 : 0, flexible, prm.abstol, prm.reltol,
                           prm.matvec_max, nmv0);
    }

    int setup(const double *rhs, const double *guess) override {
        int rc;
        if (!allocated) {
            if ((rc = alloc_vec(&d_x, nx)) || (rc = alloc_vec(&d_r, nx)) || (rc = alloc_vec(&d_p, nx)) || (rc = alloc_vec(&d_q, n)))
                return rc;
            allocated = true;
        }
        if (general_precon() && !d_z && (rc = alloc_vec(&d_z, n)) != MK_OK) return rc;
        nmv0 = 0;
        if (guess) {
            MK_HIP(hipMemcpyAsync(d_x, guess, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
            mk_launch_spmv(this, d_x, MkPlainEpi{d_q}, false);                 // r = b - A x, the product counted
            mk_launch_stream(this, MkOpSub{rhs, d_q, d_r}, n);
            nmv0 = 1;
        } else {
            MK_HIP(hipMemsetAsync(d_x, 0, sizeof(double) * (size_t)nx, stream));
            MK_HIP(hipMemcpyAsync(d_r, rhs, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
        }
        mk_launch_stream(this, MkOpDot<1>{d_r, d_r}, n);
        launch_norm(1);
        // z = M r, once, and only if the loop is going to run: from here on everything obeys the halt word the kernel above
        // wrote (a device preconditioner's launches are no-ops, the host callback is not called)
        const double *z = d_r;
        if (slot[0].kind != MK_PRECON_NONE) {
            if (general_precon()) {
                if ((rc = apply_precon(d_r, d_z)) != MK_OK) return rc;
                z = d_z;
            } else {
                mk_launch_stream(this, MkOpMul{d_prec(), d_r, d_q}, n);           // (q is free until the first product)
                z = d_q;
            }
            mk_launch_stream(this, MkOpDot<2>{d_r, z}, n);
            hipLaunchKernelGGL(pcg_rz0_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, d_part, np_stream, d_scal, next_halt());
        }
        mk_launch_stream(this, MkOpCopy{z, d_p}, n);                           // p = z
        return MK_OK;
    }

    int enqueue_spmv_only(int which) override {
        if (which != 0) return mk_fail(MK_ERR_ARG, "PCG has one product per pass");
        product(false);
        return MK_OK;
    }

    int enqueue_pass() override {
        const int par = (int)(it & 1);
        product(true);
        if (general_precon()) {
            int rc;
            PcgUpdateXR k2{};
            static_cast<PcgAlpha &>(k2) = alpha_in(par);
            k2.q = d_q;
            k2.p = d_p;
            k2.r = d_r;
            k2.x = d_x;
            mk_launch_stream(this, k2, n);
            launch_norm(0);
            if ((rc = apply_precon(d_r, d_z)) != MK_OK) return rc;
            if (flexible) mk_launch_stream(this, PcgDotZ<true>{d_r, d_z, d_q}, n);
            else mk_launch_stream(this, PcgDotZ<false>{d_r, d_z, d_q}, n);
            PcgUpdateP k3{};
            k3.part = d_part;
            k3.np = np_stream;
            k3.scal = d_scal;
            k3.par = par;
            k3.flex = flexible;
            k3.z = d_z;
            k3.p = d_p;
            mk_launch_stream(this, k3, n);
            return MK_OK;
        }
        const bool diag = d_prec() != nullptr;
        if (diag && flexible) launch_k23<true, true>(par);
        else if (diag) launch_k23<true, false>(par);
        else if (flexible) launch_k23<false, true>(par);
        else launch_k23<false, false>(par);
        return MK_OK;
    }

    int finish(mk_result *res) override {
        int rc = poll();
        if (rc != MK_OK) return rc;
        fill_result(res);
        res->residNorm = h_scal[S_RESID];
        res->residNorm0 = h_scal[S_RESID0];
        res->threshold = h_scal[S_THRESH];
        res->converged = (h_scal[S_RESID] <= h_scal[S_THRESH]) ? 1 : 0;
        res->aux[0] = h_scal[S_FLEX];
        res->aux[1] = h_scal[S_BREAK];
        return MK_OK;
    }

    const double *x() const override { return d_x; }
    const double *vector(int i) const override { return i == 0 ? d_r : (i == 1 ? d_p : nullptr); }
};

}  // namespace

mk_solver *mk_make_pcg() { return new PcgSolver(); }

extern "C" int mk_solver_set_pcg(mk_solver *s, int32_t flexible) {
    MK_ARG(s);
    if (s->prm.kind != MK_PCG) return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_set_pcg: not a PCG solver");
    if (flexible != 0 && flexible != 1) return mk_fail(MK_ERR_ARG, "mk_solver_set_pcg: flexible = %d, must be 0 or 1", (int)flexible);
    PcgSolver *d = static_cast<PcgSolver *>(s);
    if (d->is_setup || d->allocated)
        return mk_fail(MK_ERR_STATE, "mk_solver_set_pcg after mk_solver_setup: the recurrence of a run is fixed at its set-up");
    d->flexible = flexible;
    return MK_OK;
}
