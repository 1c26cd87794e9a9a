// mk_mscg.hip -- multi-shift conjugate gradients, device resident (solver kind MK_MSCG; no reference module).
//
// (A + sigma_k I) x_k = b for up to MK_MSCG_MAX_SHIFTS shifts in the Krylov space of one (Frommer and Maass; Jegerlehner,
// hep-lat/9612014).  CG runs on A itself (x_0 = 0, r = p = b, PCG's loop without a preconditioner); the residual of system k
// stays collinear with it, r_k = zeta_k r, so that a shift costs two scalars' recurrences and two vectors, x_k and p_k, and no
// product and no inner product of its own.  Its residual norm is |zeta_k| ||r||.  A shift whose norm has reached the
// threshold is FROZEN after the updates of that pass: its x_k has the pass's update, its p_k has not, and from then on
// neither its vectors nor its scalars are touched (left running, zeta_k underflows to 0 / 0).  With sigma_k = 0 every factor
// is exactly 1 and x_k is PCG's x bit for bit.  No preconditioner and no initial guess: both destroy the collinearity.
//
// One pass:
//   K1  q = A p ; partial sums of <p, q>                                (CG's product kernels, mk_cg_epi.h, as PCG's K1)
//   K2  alpha = rr / pq ; curvature test ; per active shift zeta_k', alpha_k and their breakdown test (every workgroup, one
//       lane per shift; the lead workgroup writes) ; r -= alpha q ; partial sums of <r, r>
//   Ks  one workgroup: ||r||, both histories, the freeze decisions (one lane per shift), the stop test, beta, beta_k, and
//       per shift what K3 is to do (x_k, p_k or nothing) in the coefficient table
//   K3  ceil(nsigma / GM_GROUP) group launches: r read once, per column that entered the pass active x_k += alpha_k p_k and,
//       if it is still active and the loop goes on, p_k = zeta_k' r + beta_k p_k ; the first group also p = r + beta p.  A
//       frozen column costs no load and no store, a launch with nothing to do returns from its prologue.
// In the pass that halts the x_k updates still run and no p is written (PCG's K3 rule).  Ks therefore does not raise the
// halt word itself: it leaves the stop flag in the scalar file, and the LAST group launch of K3 hands it to the halt word, so that
// every group of the halting pass still runs.  A breakdown in K2 raises the word at once: nothing is updated in that pass.
//
// Traffic of a pass beside the product: 24 n (K2: q, r read, r written) + 16 n (base p) + per group launch 8 n (r) + per
// ACTIVE shift 32 n (x_k and p_k read and written) bytes; Ks and the scalar work move O(nsigma) bytes.
#include "mk_solver.h"
#include "mk_cg_epi.h"
#include "mk_multicol.h"      // GM_GROUP

namespace {

constexpr int NS = MK_MSCG_MAX_SHIFTS;
static_assert(NS <= MK_WAVE, "one lane per shift in the prologues");

enum { S_RR = 0, S_THRESH = 1, S_RESID = 2, S_RESID0 = 3, S_PQ = 4, S_ALPHA = 5, S_BETA = 6, S_BREAK = 7, S_APREV = 8, S_BPREV = 9,
       S_GO = 10, S_NFROZEN = 11, S_MAXRES = 12 };
// partial-sum slots: 0 <p,q> (the product kernel's), 1 <r,r>

// the coefficient table: rows of NS doubles, then the per-shift record of mk_solver_vector (3 per shift)
enum { T_SIGMA = 0, T_ZPREV, T_ZCUR, T_ZNEW, T_ALPHAK, T_BETAK, T_ACTIVE, T_DO, T_ROWS };
constexpr int T_REC = T_ROWS * NS;
constexpr int T_LEN = T_REC + 3 * NS;
// T_DO: 0 nothing (the shift entered the pass frozen), 1 x_k only, 3 x_k and p_k

__device__ __forceinline__ bool mscg_bad(double v) { return v == 0.0 || !isfinite(v); }

// K2: alpha, the curvature test and the shifts' scalars in the prologue; r -= alpha q with the partial sums of <r, r>
struct MscgUpdateR {
    static constexpr int NACC = 1, SLOT0 = 1;
    const double *part;
    int np;
    double *scal;
    MkStatus *st;
    double *tab;
    int nsigma, check_curv;
    const double *q;
    double *r;
    double alpha;
    bool bad;
    MkTotalRegs tr;
    double rr_in, aprev, bprev, sg, zp, zc, act;
    __device__ void early() {
        mk_total_issue(part, np, tr);
        rr_in = scal[S_RR];
        aprev = scal[S_APREV];
        bprev = scal[S_BPREV];
        const int k = (int)threadIdx.x < nsigma ? (int)threadIdx.x : 0;
        sg = tab[T_SIGMA * NS + k];
        zp = tab[T_ZPREV * NS + k];
        zc = tab[T_ZCUR * NS + k];
        act = tab[T_ACTIVE * NS + k];
    }
    __device__ bool prologue(double *s4, bool lead) {
        const double pq = mk_total_finish(tr, np, s4);
        const bool curv = check_curv && !(pq > 0.0);
        alpha = rr_in / pq;
        // lane k < nsigma of every workgroup: zeta_k' and alpha_k of an active shift
        const bool mine = (int)threadIdx.x < nsigma && act != 0.0 && !curv;
        double zn = zc, ak = 0.0;
        int broke = 0;
        if (mine) {
            const double den = (zp * aprev) * (1.0 + sg * alpha) + (alpha * bprev) * (zp - zc);
            zn = ((zc * zp) * aprev) / den;
            ak = (alpha * zn) / zc;
            broke = (mscg_bad(den) || mscg_bad(zn)) ? 1 : 0;
        }
        const bool bad2 = __syncthreads_or(broke) != 0;
        bad = curv || bad2;
        if (blockIdx.x == 0 && mine && !bad2) {
            tab[T_ZNEW * NS + threadIdx.x] = zn;
            tab[T_ALPHAK * NS + threadIdx.x] = ak;
        }
        if (lead) {
            st->nMatvec += 1;
            scal[S_PQ] = pq;
            scal[S_ALPHA] = alpha;
            if (curv) {                                   // nothing is updated; p is the direction of no descent
                st->definite = 0;
                scal[S_BREAK] = 1.0;
            } else if (bad2) {                            // nothing is updated: every x_k is its last iterate
                scal[S_BREAK] = 2.0;
            }
        }
        return bad;
    }
    __device__ bool skip() const { return bad; }
    struct Regs {
        double2 qv, rv;
    };
    __device__ void load2(int64_t i, Regs &g) const {
        g.qv = mk_ld2(q, i);
        g.rv = mk_ld2(r, i);
    }
    __device__ void apply2(Regs &g, double *acc) const {
        g.rv.x = g.rv.x - alpha * g.qv.x;
        g.rv.y = g.rv.y - alpha * g.qv.y;
        acc[0] += g.rv.x * g.rv.x;
        acc[0] += g.rv.y * g.rv.y;
    }
    __device__ void store2(int64_t i, const Regs &g) const { mk_st2(r, i, g.rv); }
    __device__ void one(int64_t i, double *acc) {
        const double rv = r[i] - alpha * q[i];
        r[i] = rv;
        acc[0] += rv * rv;
    }
};

// Ks (first = 0) and the set-up's norm kernel (first = 1): one workgroup, lane k < nsigma owns shift k
__global__ __launch_bounds__(MK_BLOCK) void mscg_scalar_kernel(const double *part, int np, double *scal, MkStatus *st, double *hist,
                                                               double *tab, int nsigma, MkHalt halt, int first, double abstol,
                                                               double reltol, int64_t matvec_max) {
    __shared__ double s4[4];
    __shared__ double s_res[NS];
    __shared__ int s_ent[NS], s_live[NS];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double rr = mk_total(part + MK_MAXP, np, s4);
    const double resid = __dsqrt_rn(rr);
    const int k = (int)threadIdx.x;
    const bool lane = k < nsigma;
    if (first) {
        const double rel = reltol * resid;
        const double thresh = (rel > abstol) ? rel : abstol;
        const bool conv = resid <= thresh;                  // (a zero right-hand side: every x_k = 0 solves its system)
        if (lane) {
            tab[T_ACTIVE * NS + k] = conv ? 0.0 : 1.0;
            tab[T_REC + 3 * k + 1] = resid;
            tab[T_REC + 3 * k + 2] = conv ? 0.0 : -1.0;
        }
        if (k != 0) return;
        scal[S_THRESH] = thresh;
        scal[S_RESID] = resid;
        scal[S_RESID0] = resid;
        scal[S_MAXRES] = resid;
        scal[S_NFROZEN] = conv ? (double)nsigma : 0.0;
        scal[S_APREV] = 1.0;
        scal[S_BPREV] = 0.0;
        hist[0] = resid;
        hist[MK_HIST_RING] = resid;
        st->hist_len = 1;
        st->nMatvec = 0;
        st->itn = 0;
        st->definite = 1;
        bool stop = conv || (0 >= matvec_max);
        if (!stop) {
            stop = !(rr > 0.0) || !isfinite(rr);
            if (stop) scal[S_BREAK] = 2.0;
            else scal[S_RR] = rr;
        }
        halt.out(stop);
        return;
    }
    const double thresh = scal[S_THRESH];
    const double rr_old = scal[S_RR];
    const int64_t pass = st->itn + 1;
    // the freeze decisions: |zeta_k'| ||r|| of every shift that entered the pass active
    bool entered = false, live = false;
    double zn = 1.0, zc = 1.0;
    if (lane) {
        entered = tab[T_ACTIVE * NS + k] != 0.0;
        double res = tab[T_REC + 3 * k + 1];
        if (entered) {
            zn = tab[T_ZNEW * NS + k];
            zc = tab[T_ZCUR * NS + k];
            res = fabs(zn) * resid;
            live = !(res <= thresh);
            tab[T_ZPREV * NS + k] = zc;
            tab[T_ZCUR * NS + k] = zn;
            tab[T_REC + 3 * k] = zn;
            tab[T_REC + 3 * k + 1] = res;
            if (!live) {
                tab[T_ACTIVE * NS + k] = 0.0;
                tab[T_REC + 3 * k + 2] = (double)pass;
            }
        }
        s_res[k] = res;
        s_ent[k] = entered ? 1 : 0;
        s_live[k] = live ? 1 : 0;
    }
    __syncthreads();
    int nlive = 0;
    for (int j = 0; j < nsigma; ++j) nlive += s_live[j];
    const bool stop = (nlive == 0) || (st->nMatvec >= matvec_max);
    const bool broke = !stop && (!(rr > 0.0) || !isfinite(rr));
    const bool go = !stop && !broke;
    const double beta = rr / rr_old;
    if (lane) {
        double what = 0.0;
        if (entered) {
            what = 1.0;
            if (live && go) {
                const double ratio = zn / zc;
                tab[T_BETAK * NS + k] = beta * (ratio * ratio);
                what = 3.0;
            }
        }
        tab[T_DO * NS + k] = what;
    }
    if (k != 0) return;
    double pass_max = 0.0, all_max = 0.0;
    for (int j = 0; j < nsigma; ++j) {
        if (s_ent[j] && s_res[j] > pass_max) pass_max = s_res[j];
        if (s_res[j] > all_max) all_max = s_res[j];
    }
    scal[S_RESID] = resid;
    scal[S_MAXRES] = all_max;
    scal[S_NFROZEN] = (double)(nsigma - nlive);
    scal[S_GO] = go ? 1.0 : 0.0;
    const int64_t at = st->hist_len % MK_HIST_RING;
    hist[at] = resid;
    hist[MK_HIST_RING + at] = pass_max;
    st->hist_len += 1;
    st->itn += 1;
    if (broke) scal[S_BREAK] = 2.0;
    if (go) {
        scal[S_BETA] = beta;
        scal[S_RR] = rr;
        scal[S_APREV] = scal[S_ALPHA];
        scal[S_BPREV] = beta;
    }
    halt.out(false);                                        // (K3's last group launch raises the word: see the header)
}

struct MscgCols {
    double *x[GM_GROUP], *p[GM_GROUP];
};

// K3: one group of columns.  BASE: the first group, which also forms p = r + beta p.
template <bool BASE>
struct MscgUpdateXP {
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *scal;
    const double *tab;           // at the group's first column
    int ncol, last;
    const double *r;
    double *p;
    MscgCols c;
    double ak[GM_GROUP], zk[GM_GROUP], bk[GM_GROUP], what[GM_GROUP];
    double beta, gof;
    unsigned mx, mp;             // columns whose x_k / p_k this pass updates (wave uniform)
    bool go;
    __device__ void early() {
        gof = scal[S_GO];
        beta = scal[S_BETA];
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k) {
            const int j = k < ncol ? k : 0;
            what[k] = tab[T_DO * NS + j];
            ak[k] = tab[T_ALPHAK * NS + j];
            zk[k] = tab[T_ZCUR * NS + j];
            bk[k] = tab[T_BETAK * NS + j];
        }
    }
    __device__ bool prologue(double *, bool) {
        go = gof != 0.0;
        mx = mp = 0u;
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (k < ncol) {
                if (what[k] != 0.0) mx |= 1u << k;
                if (what[k] == 3.0) mp |= 1u << k;
            }
        return last && !go;
    }
    __device__ bool skip() const { return mx == 0u && !(BASE && go); }
    __device__ void pair(int64_t i, double *) {
        double2 rv{0.0, 0.0}, pv{0.0, 0.0};
        if (go) rv = mk_ld2(r, i);
        if (BASE && go) pv = mk_ld2(p, i);
        double2 xv[GM_GROUP], cv[GM_GROUP];
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (mx >> k & 1u) {
                xv[k] = mk_ld2(c.x[k], i);
                cv[k] = mk_ld2(c.p[k], i);
            }
        if (BASE && go) {
            pv.x = rv.x + beta * pv.x;
            pv.y = rv.y + beta * pv.y;
            mk_st2(p, i, pv);
        }
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (mx >> k & 1u) {
                xv[k].x = xv[k].x + ak[k] * cv[k].x;
                xv[k].y = xv[k].y + ak[k] * cv[k].y;
                mk_st2(c.x[k], i, xv[k]);
                if (mp >> k & 1u) {
                    cv[k].x = zk[k] * rv.x + bk[k] * cv[k].x;
                    cv[k].y = zk[k] * rv.y + bk[k] * cv[k].y;
                    mk_st2(c.p[k], i, cv[k]);
                }
            }
    }
    __device__ void one(int64_t i, double *) {
        const double rv = go ? r[i] : 0.0;
        if (BASE && go) p[i] = rv + beta * p[i];
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (mx >> k & 1u) {
                const double cv = c.p[k][i];
                c.x[k][i] = c.x[k][i] + ak[k] * cv;
                if (mp >> k & 1u) c.p[k][i] = zk[k] * rv + bk[k] * cv;
            }
    }
};

struct MscgSolver : mk_solver {
    double *d_r = nullptr, *d_p = nullptr, *d_q = nullptr, *d_tab = nullptr;
    double *d_xk[NS] = {}, *d_pk[NS] = {};
    std::vector<double> h_tab;          // the table of a set-up, uploaded in stream order

    void product(bool timed) {                              // K1, with CG's choice of the non-temporal variant
        if (A && mk_store_nt(A)) mk_launch_spmv(this, d_p, CgSpmvEpiT<true>{d_p, d_q, 0.0}, timed);
        else mk_launch_spmv(this, d_p, CgSpmvEpi{d_p, d_q, 0.0}, timed);
    }
    void launch_scalar(int first) {
        hipLaunchKernelGGL(mscg_scalar_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, d_part, np_stream, d_scal, d_status, d_hist,
                           d_tab, nsigma, next_halt(), first, prm.abstol, prm.reltol, prm.matvec_max);
    }
    template <bool BASE>
    void launch_group(int c0) {
        MscgUpdateXP<BASE> k3{};
        k3.scal = d_scal;
        k3.tab = d_tab + c0;
        k3.ncol = nsigma - c0 < GM_GROUP ? nsigma - c0 : GM_GROUP;
        k3.last = c0 + GM_GROUP >= nsigma ? 1 : 0;
        k3.r = d_r;
        k3.p = d_p;
        for (int k = 0; k < GM_GROUP; ++k) {
            k3.c.x[k] = d_xk[c0 + (k < k3.ncol ? k : 0)];
            k3.c.p[k] = d_pk[c0 + (k < k3.ncol ? k : 0)];
        }
        mk_launch_stream(this, k3, n);
    }

    // every vector is allocated where it is still missing: a set-up that ran out of memory leaves nothing half done, and
    // a later one goes on from what this one got
    int allocate() {
        int rc;
        if (!d_tab) {
            MK_HIP(hipMalloc((void **)&d_tab, sizeof(double) * T_LEN));
            vecs.push_back(d_tab);
        }
        if (!d_r && (rc = alloc_vec(&d_r, nx)) != MK_OK) return rc;
        if (!d_p && (rc = alloc_vec(&d_p, nx)) != MK_OK) return rc;
        if (!d_q && (rc = alloc_vec(&d_q, n)) != MK_OK) return rc;
        for (int k = 0; k < nsigma; ++k) {
            if (!d_xk[k] && (rc = alloc_vec(&d_xk[k], n)) != MK_OK) return rc;
            if (!d_pk[k] && (rc = alloc_vec(&d_pk[k], n)) != MK_OK) return rc;
        }
        return MK_OK;
    }
    double workspace_bytes() const { return 8.0 * (double)(2 * nx + n + 2 * (int64_t)nsigma * n); }

    int setup(const double *rhs, const double *guess) override {
        if (guess)
            return mk_fail(MK_ERR_ARG, "mk_solver_setup: multi-shift CG takes no initial guess (the residuals of the shifted "
                           "systems would no longer be collinear)");
        int rc = allocate();
        if (rc != MK_OK) return rc;
        use_hist2 = true;
        h_tab.assign(T_LEN, 0.0);
        for (int k = 0; k < nsigma; ++k) {
            h_tab[T_SIGMA * NS + k] = sigma[k];
            h_tab[T_ZPREV * NS + k] = h_tab[T_ZCUR * NS + k] = h_tab[T_ZNEW * NS + k] = 1.0;
            h_tab[T_REC + 3 * k] = 1.0;
            h_tab[T_REC + 3 * k + 2] = -1.0;
        }
        MK_HIP(hipMemcpyAsync(d_tab, h_tab.data(), sizeof(double) * T_LEN, hipMemcpyHostToDevice, stream));
        const size_t bytes = sizeof(double) * (size_t)n;
        MK_HIP(hipMemcpyAsync(d_r, rhs, bytes, hipMemcpyDeviceToDevice, stream));
        MK_HIP(hipMemcpyAsync(d_p, rhs, bytes, hipMemcpyDeviceToDevice, stream));
        for (int k = 0; k < nsigma; ++k) {
            MK_HIP(hipMemsetAsync(d_xk[k], 0, bytes, stream));
            MK_HIP(hipMemcpyAsync(d_pk[k], rhs, bytes, hipMemcpyDeviceToDevice, stream));
        }
        mk_launch_stream(this, MkOpDot<1>{d_r, d_r}, n);
        launch_scalar(1);
        return MK_OK;
    }

    int enqueue_spmv_only(int which) override {
        if (which != 0) return mk_fail(MK_ERR_ARG, "multi-shift CG has one product per pass");
        product(false);
        return MK_OK;
    }

    int enqueue_pass() override {
        product(true);
        MscgUpdateR k2{};
        k2.part = d_part;
        k2.np = np_spmv;
        k2.scal = d_scal;
        k2.st = d_status;
        k2.tab = d_tab;
        k2.nsigma = nsigma;
        k2.check_curv = prm.check_curvature;
        k2.q = d_q;
        k2.r = d_r;
        mk_launch_stream(this, k2, n);
        launch_scalar(0);
        launch_group<true>(0);
        for (int c0 = GM_GROUP; c0 < nsigma; c0 += GM_GROUP) launch_group<false>(c0);
        return MK_OK;
    }

    int finish(mk_result *res) override {
        int rc = poll();
        if (rc != MK_OK) return rc;
        fill_result(res);
        res->residNorm = h_scal[S_MAXRES];
        res->residNorm0 = h_scal[S_RESID0];
        res->threshold = h_scal[S_THRESH];
        res->converged = ((int)h_scal[S_NFROZEN] == nsigma) ? 1 : 0;
        res->aux[0] = (double)nsigma;
        res->aux[1] = h_scal[S_BREAK];
        res->aux[2] = h_scal[S_NFROZEN];
        res->aux[3] = workspace_bytes();
        return MK_OK;
    }

    const double *x() const override { return d_xk[0]; }
    const double *vector(int i) const override {
        if (i == 0) return d_r;
        if (i == 1) return d_p;
        const int ns = nsigma;
        if (i >= 2 && i < 2 + ns) return d_xk[i - 2];
        if (i >= 2 + ns && i < 2 + 2 * ns) return d_pk[i - 2 - ns];
        if (i == 2 + 2 * ns && d_tab) return d_tab + T_REC;
        return nullptr;
    }
    int64_t vector_len(int i) const override { return i == 2 + 2 * nsigma ? 3 * (int64_t)nsigma : n; }
};

}  // namespace

mk_solver *mk_make_mscg() { return new MscgSolver(); }
