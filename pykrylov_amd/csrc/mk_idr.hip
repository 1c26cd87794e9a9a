// mk_idr.hip -- IDR(s) with right preconditioning, device resident.  No reference module: the NumPy
// restatement is tests/_idr_ref.py.
//
// The biorthogonal form of van Gijzen and Sonneveld (ACM TOMS 38, 2011), with the new g made orthogonal to the earlier shadow
// vectors by ONE batch of s dots and a triangular solve instead of k dependent dots.  P (shadow vectors), G and U are s rows
// of `ld` doubles each, in one allocation; M (s x s, lower triangular once a cycle is through), f, c and a live in IDR's own
// scalar block, om and beta in the solver's.  One pass of the driver = one inner step k of the current cycle:
//   C   v = r - sum_{i>=k} c_i G_i and t = sum_{i>=k} c_i U_i, i ascending, GM_GROUP columns of G and of U per launch; the
//       last launch forms u = t + om v straight into U_k.  With a preconditioner it writes v instead, v = precon * v goes
//       through the solver's slot, and one more pass forms u                                        [ceil((s-k) / GM_GROUP) launches]
//   P   G_k = A U_k                                                                                 [product, in A's format]
//   D   m_i = <p_i, G_k> for all s rows, GM_GROUP rows per launch with one read of G_k             [ceil(s / GM_GROUP) launches]
//   K   one workgroup: the totals, a of M[:k,:k] a = m[:k], the new column M[k:,k] = m[k:] - M[k:,:k] a, the pivot test,
//       beta = f_k / M_kk, f[k+1:] -= beta M[k+1:,k], and the next step's c of M[k+1:,k+1:] c = f[k+1:].  Wave 0 runs the
//       substitutions as column sweeps (lane i owns row i, so every row subtracts its terms in ascending column order)
//   F   G_k -= a_i G_i, U_k -= a_i U_i (i < k, ascending), GM_GROUP columns per launch; the last launch goes on with
//       r -= beta G_k, x += beta U_k and the partials of <r, r>                                     [max(1, ceil(k / GM_GROUP)) launches]
//   N   one workgroup: ||r||, the history ring, the status record, the stop tests
// The pass of step s - 1 goes on with the dimension-reduction step -- v = precon * r; t = A v; one stream kernel for <t,t> and
// <t,r>; O: om in one workgroup; r -= om t, x += om v with <r,r>; N -- and with f = P r of the next cycle (D, then K0: the
// totals and c of M c = f).  x is complete after every step, so a halted run needs no drain.
//
// Bytes per inner step k without a preconditioner, s <= GM_GROUP: the product + (16 (s - k) + 16) n [C] + (8 s + 8) n [D] +
// (16 k + 48 [+ 16 if k > 0]) n [F], together (24 s + 72 [+ 16]) n whatever k is.  The step index and the number of products
// are host knowledge, every scalar stays on the device.  Every operation rounds on its own (-ffp-contract=off); every dot
// has the lanes, the grid and the tree of mk_stream_kernel<MkOpDot>, then mk_total.
#include <cmath>
#include <vector>

#include "mk_multicol.h"
#include "mk_solver.h"

namespace {

constexpr int ID_MAXS = MK_IDR_MAX_S;
constexpr double ID_KAPPA = 0.7;

// the shared scalar file (poll() brings it to the host)
enum { S_THRESH = 0, S_RESID = 1, S_RESID0 = 2, S_OM = 3, S_BETA = 4, S_S = 5, S_CYCLES = 6, S_BREAK = 7 };

// IDR's own scalar block: M row by row, f, c (the combination of step k, entries k ..), a (the coefficients of F, entries .. k - 1)
struct IdScal {
    double *M, *f, *c, *a;
    int s;
};

struct IdOpHashRow {            // p[i] = mk_cell_field(i, seed) - 1.0, in [-0.5, 0.5)
    static constexpr int NACC = 0, SLOT0 = 0;
    double *p;
    uint64_t seed;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 v;
        v.x = mk_cell_field(i, seed) - 1.0;
        v.y = mk_cell_field(i + 1, seed) - 1.0;
        mk_st2(p, i, v);
    }
    __device__ void one(int64_t i, double *) { p[i] = mk_cell_field(i, seed) - 1.0; }
};

struct IdOpResid {              // r = b - t ; partial <r, r>
    static constexpr int NACC = 1, SLOT0 = 0;
    const double *b, *t;
    double *r;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        double2 u = mk_ld2(b, i);
        const double2 v = mk_ld2(t, i);
        u.x -= v.x;
        u.y -= v.y;
        mk_st2(r, i, u);
        acc[0] += u.x * u.x;
        acc[0] += u.y * u.y;
    }
    __device__ void one(int64_t i, double *acc) {
        const double u = b[i] - t[i];
        r[i] = u;
        acc[0] += u * u;
    }
};

// C: one group of columns.  v = vin - c_i G_i and t = tin + c_i U_i, i ascending (`first`: vin is r and t starts from
// zero; otherwise both are the earlier groups' results in `v` and `u`).  FUSE (the last group, no preconditioner):
// u = t + om v is written and v is not; otherwise v and t are.  `u` is U_k, which the first group also reads as a column:
// a lane loads every column before it stores.
template <bool FUSE>
struct IdOpCombine {
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *c;             // at the group's first coefficient
    const double *om;
    const double *vin;
    double *v, *u;
    GmCols G, U;
    int ncol, first;
    double coef[GM_GROUP], omv;
    __device__ bool prologue(double *, bool) {
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k) coef[k] = k < ncol ? c[k] : 0.0;
        omv = om[0];
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 vv = mk_ld2(vin, i);
        double2 tv{0.0, 0.0};
        if (!first) tv = mk_ld2(u, i);
        double2 gv[GM_GROUP], uv[GM_GROUP];
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (k < ncol) {
                gv[k] = mk_ld2(G.col[k], i);
                uv[k] = mk_ld2(U.col[k], i);
            }
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (k < ncol) {
                vv.x = vv.x - coef[k] * gv[k].x;
                vv.y = vv.y - coef[k] * gv[k].y;
                tv.x = tv.x + coef[k] * uv[k].x;
                tv.y = tv.y + coef[k] * uv[k].y;
            }
        if constexpr (FUSE) {
            tv.x = tv.x + omv * vv.x;
            tv.y = tv.y + omv * vv.y;
        } else {
            mk_st2(v, i, vv);
        }
        mk_st2(u, i, tv);
    }
    __device__ void one(int64_t i, double *) {
        double vv = vin[i];
        double tv = first ? 0.0 : u[i];
        double gv[GM_GROUP], uv[GM_GROUP];
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (k < ncol) {
                gv[k] = G.col[k][i];
                uv[k] = U.col[k][i];
            }
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (k < ncol) {
                vv = vv - coef[k] * gv[k];
                tv = tv + coef[k] * uv[k];
            }
        if constexpr (FUSE) tv = tv + omv * vv;
        else v[i] = vv;
        u[i] = tv;
    }
};

struct IdOpAxpy {               // u = u + om z      (C's last operation after a preconditioner)
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *om, *z;
    double *u;
    double omv;
    __device__ bool prologue(double *, bool) {
        omv = om[0];
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 uv = mk_ld2(u, i);
        const double2 zv = mk_ld2(z, i);
        uv.x = uv.x + omv * zv.x;
        uv.y = uv.y + omv * zv.y;
        mk_st2(u, i, uv);
    }
    __device__ void one(int64_t i, double *) { u[i] = u[i] + omv * z[i]; }
};

// F: one group of columns.  g = g - a_i G_i and u = u - a_i U_i, i ascending (ncol = 0 at step 0: nothing to subtract,
// nothing stored).  LAST: r = r - beta g, x = x + beta u and the partials of <r, r>.
template <bool LAST>
struct IdOpUpdate {
    static constexpr int NACC = LAST ? 1 : 0, SLOT0 = 0;
    const double *a;             // at the group's first coefficient
    const double *beta;
    double *g, *u, *r, *x;
    GmCols G, U;
    int ncol;
    double coef[GM_GROUP], bt;
    __device__ bool prologue(double *, bool) {
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k) coef[k] = k < ncol ? a[k] : 0.0;
        bt = LAST ? beta[0] : 0.0;
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        double2 gw = mk_ld2(g, i), uw = mk_ld2(u, i);
        double2 gv[GM_GROUP], uv[GM_GROUP];
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (k < ncol) {
                gv[k] = mk_ld2(G.col[k], i);
                uv[k] = mk_ld2(U.col[k], i);
            }
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (k < ncol) {
                gw.x = gw.x - coef[k] * gv[k].x;
                gw.y = gw.y - coef[k] * gv[k].y;
                uw.x = uw.x - coef[k] * uv[k].x;
                uw.y = uw.y - coef[k] * uv[k].y;
            }
        if (ncol > 0) {
            mk_st2(g, i, gw);
            mk_st2(u, i, uw);
        }
        if constexpr (LAST) {
            double2 rv = mk_ld2(r, i), xv = mk_ld2(x, i);
            rv.x = rv.x - bt * gw.x;
            rv.y = rv.y - bt * gw.y;
            xv.x = xv.x + bt * uw.x;
            xv.y = xv.y + bt * uw.y;
            mk_st2(r, i, rv);
            mk_st2(x, i, xv);
            acc[0] += rv.x * rv.x;
            acc[0] += rv.y * rv.y;
        }
    }
    __device__ void one(int64_t i, double *acc) {
        double gw = g[i], uw = u[i];
#pragma unroll
        for (int k = 0; k < GM_GROUP; ++k)
            if (k < ncol) {
                gw = gw - coef[k] * G.col[k][i];
                uw = uw - coef[k] * U.col[k][i];
            }
        if (ncol > 0) {
            g[i] = gw;
            u[i] = uw;
        }
        if constexpr (LAST) {
            const double rv = r[i] - bt * gw;
            r[i] = rv;
            x[i] = x[i] + bt * uw;
            acc[0] += rv * rv;
        }
    }
};

struct IdOpDot2 {               // partials of <t, t> (slot 0) and <t, r> (slot 1), one read of t
    static constexpr int NACC = 2, SLOT0 = 0;
    const double *t, *r;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        const double2 tv = mk_ld2(t, i), rv = mk_ld2(r, i);
        acc[0] += tv.x * tv.x;
        acc[0] += tv.y * tv.y;
        acc[1] += tv.x * rv.x;
        acc[1] += tv.y * rv.y;
    }
    __device__ void one(int64_t i, double *acc) {
        acc[0] += t[i] * t[i];
        acc[1] += t[i] * r[i];
    }
};

struct IdOpDrUpdate {           // r = r - om t ; x = x + om v ; partial <r, r>
    static constexpr int NACC = 1, SLOT0 = 0;
    const double *om, *t, *v;
    double *r, *x;
    double omv;
    __device__ bool prologue(double *, bool) {
        omv = om[0];
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        const double2 tv = mk_ld2(t, i), vv = mk_ld2(v, i);
        double2 rv = mk_ld2(r, i), xv = mk_ld2(x, i);
        rv.x = rv.x - omv * tv.x;
        rv.y = rv.y - omv * tv.y;
        xv.x = xv.x + omv * vv.x;
        xv.y = xv.y + omv * vv.y;
        mk_st2(r, i, rv);
        mk_st2(x, i, xv);
        acc[0] += rv.x * rv.x;
        acc[0] += rv.y * rv.y;
    }
    __device__ void one(int64_t i, double *acc) {
        const double vv = v[i];
        const double rv = r[i] - omv * t[i];
        r[i] = rv;
        x[i] = x[i] + omv * vv;
        acc[0] += rv * rv;
    }
};

// y of Ms[lo:hi, lo:hi] y = rhs[lo:hi] (Ms: the s x s matrix in LDS) by a column sweep over wave 0: lane i brings rhs_i and
// leaves with y_i; in sweep j lane j's quotient goes round and every later row subtracts its term -- row i thus runs
// t = rhs_i ; t = t - M_ij y_j, j ascending ; y_i = t / M_ii.  All 64 lanes call it.
__device__ __forceinline__ double id_lower_solve(const double *Ms, int s, int lo, int hi, int lane, double t) {
    const bool mine = lane >= lo && lane < hi;
    const double d = mine ? Ms[lane * s + lane] : 1.0;
    double y = 0.0;
    for (int j = lo; j < hi; ++j) {
        const double yj = __shfl(t / d, j, 64);
        if (lane == j) y = yj;
        if (mine && lane > j) t = t - Ms[lane * s + j] * yj;
    }
    return y;
}

// the totals of the s slots of a bank into LDS (every lane of the workgroup takes part) and M into LDS
__device__ __forceinline__ void id_stage(const double *bank, int np, const IdScal &sc, double *tot, double *Ms, double *s4) {
    const int t = (int)threadIdx.x;
    for (int i = 0; i < sc.s; ++i) {
        const double v = mk_total(bank + (size_t)i * MK_MAXP, np, s4);
        if (t == 0) tot[i] = v;
    }
    for (int e = t; e < sc.s * sc.s; e += MK_BLOCK) Ms[e] = sc.M[e];
    __syncthreads();
}

// K0: f = the totals of D on r, and c of M c = f for step 0 of the cycle
__global__ __launch_bounds__(MK_BLOCK) void id_cycle_kernel(const double *bank, int np, IdScal sc, MkHalt halt) {
    __shared__ double s4[4];
    __shared__ double Ms[ID_MAXS * ID_MAXS], fs[ID_MAXS];
    const int t = (int)threadIdx.x;
    if (halt.in()) {
        if (t == 0) halt.out(true);
        return;
    }
    id_stage(bank, np, sc, fs, Ms, s4);
    if (t < MK_WAVE) {
        const int s = sc.s;
        const double y = id_lower_solve(Ms, s, 0, s, t, t < s ? fs[t] : 0.0);
        if (t < s) {
            sc.f[t] = fs[t];
            sc.c[t] = y;
        }
    }
    if (t == 0) halt.out(false);
}

// K: the small work of step k, whose product was the run's product number nmv
__global__ __launch_bounds__(MK_BLOCK) void id_step_kernel(const double *bank, int np, double *scal, IdScal sc, MkStatus *st,
                                                           double *hist, MkHalt halt, int k, int64_t nmv) {
    __shared__ double s4[4];
    __shared__ double Ms[ID_MAXS * ID_MAXS], ms[ID_MAXS];
    const int t = (int)threadIdx.x;
    if (halt.in()) {
        if (t == 0) halt.out(true);
        return;
    }
    id_stage(bank, np, sc, ms, Ms, s4);
    if (t >= MK_WAVE) return;
    const int s = sc.s;
    const bool row = t < s;
    const double a = id_lower_solve(Ms, s, 0, k, t, t < k ? ms[t] : 0.0);          // lane i < k: a_i
    double col = row ? ms[t] : 0.0;                                               // lane i >= k: M_ik
    for (int j = 0; j < k; ++j) {
        const double aj = __shfl(a, j, 64);
        if (row && t >= k) col = col - Ms[t * s + j] * aj;
    }
    const double piv = __shfl(col, k, 64);
    if (row && t >= k) sc.M[t * s + k] = col;
    if (piv == 0.0 || !isfinite(piv)) {                     // breakdown: x stays the last iterate
        if (t == 0) {
            hist[st->hist_len % MK_HIST_RING] = scal[S_RESID];
            st->hist_len += 1;
            st->itn += 1;
            st->nMatvec = nmv;
            st->converged = 0;
            scal[S_BREAK] = 1.0;
            halt.out(true);
        }
        return;
    }
    const double beta = sc.f[k] / piv;
    double fi = row ? sc.f[t] : 0.0;
    if (row && t > k) {
        fi = fi - beta * col;
        sc.f[t] = fi;
    }
    if (k + 1 < s) {                                        // (the columns from k + 1 on are the earlier cycle's)
        const double y = id_lower_solve(Ms, s, k + 1, s, t, fi);
        if (row && t > k) sc.c[t] = y;
    }
    if (t < k) sc.a[t] = a;
    if (t == 0) {
        scal[S_BETA] = beta;
        st->nMatvec = nmv;
        halt.out(false);
    }
}

// O: om of the dimension-reduction step from <t,t> (slot 0) and <t,r> (slot 1)
__global__ __launch_bounds__(MK_BLOCK) void id_omega_kernel(const double *part, int np, double *scal, MkStatus *st, double *hist,
                                                            MkHalt halt, int64_t nmv) {
    __shared__ double s4[4];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double tt = mk_total(part, np, s4);
    const double tr = mk_total(part + MK_MAXP, np, s4);
    if (threadIdx.x == 0) {
        double om = tr / tt;
        const double rho = fabs(tr) / (__dsqrt_rn(tt) * scal[S_RESID]);
        if (rho < ID_KAPPA) om = om * (ID_KAPPA / rho);
        const bool bad = tt == 0.0 || om == 0.0 || !isfinite(om);
        st->nMatvec = nmv;
        if (bad) {
            hist[st->hist_len % MK_HIST_RING] = scal[S_RESID];
            st->hist_len += 1;
            st->itn += 1;
            st->converged = 0;
            scal[S_BREAK] = 2.0;
        } else {
            scal[S_OM] = om;
        }
        halt.out(bad);
    }
}

// N: ||r|| = sqrt<r, r> and the loop tests on it.  first: the set-up (threshold, history[0]); otherwise the end of a step
// (`cycle`: of a dimension-reduction step) whose product was the run's product number `nmv`.
__global__ __launch_bounds__(MK_BLOCK) void id_norm_kernel(const double *rr_part, int np, double *scal, MkStatus *st, double *hist,
                                                           MkHalt halt, int first, int cycle, int s, double abstol, double reltol,
                                                           int64_t matvec_max, int64_t nmv) {
    __shared__ double s4[4];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double nr = __dsqrt_rn(mk_total(rr_part, np, s4));
    if (threadIdx.x == 0) {
        double thresh = scal[S_THRESH];
        if (first) {
            const double rel = reltol * nr;
            thresh = (rel > abstol) ? rel : abstol;
            scal[S_THRESH] = thresh;
            scal[S_RESID0] = nr;
            scal[S_OM] = 1.0;
            scal[S_S] = (double)s;
            hist[0] = nr;
            st->hist_len = 1;
            st->itn = 0;
        } else {
            hist[st->hist_len % MK_HIST_RING] = nr;
            st->hist_len += 1;
            st->itn += 1;
            if (cycle) scal[S_CYCLES] = scal[S_CYCLES] + 1.0;
        }
        scal[S_RESID] = nr;
        st->nMatvec = nmv;
        st->converged = (nr <= thresh) ? 1 : 0;
        halt.out(!(nr > thresh) || nmv >= matvec_max);
    }
}

struct IdrSolver : mk_solver {
    double *d_x = nullptr, *d_r = nullptr, *d_v = nullptr, *d_t = nullptr;
    double *d_blk = nullptr;         // P, G and U: 3 s rows of ld doubles
    double *d_iscal = nullptr;       // IdScal's storage
    double *d_ipart = nullptr;       // `nslot` slots for D, then <r,r>, <t,t>, <t,r>
    IdScal sc{};
    std::vector<double> h_iscal;     // the block's initial state (M = I)
    int want_s = 4, s = 0, nslot = 0;
    uint64_t seed = 1;
    const double *shadow = nullptr;  // borrowed: the caller's P, want_s rows of n doubles
    int64_t ld = 0;
    size_t blk_bytes = 0;
    int k = 0;                       // steps of the current cycle enqueued so far
    int64_t nmv = 0;                 // products enqueued so far
    bool allocated = false;
    bool takes_precon() const override { return true; }

    ~IdrSolver() override {
        if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
        hipFree(d_blk);
        hipFree(d_iscal);
        hipFree(d_ipart);
    }

    double *P(int i) const { return d_blk + (size_t)i * (size_t)ld; }
    double *G(int i) const { return d_blk + (size_t)(s + i) * (size_t)ld; }
    double *U(int i) const { return d_blk + (size_t)(2 * s + i) * (size_t)ld; }
    double *rr_part() const { return d_ipart + (size_t)nslot * MK_MAXP; }
    double *tt_part() const { return rr_part() + MK_MAXP; }
    size_t nscal() const { return (size_t)s * s + (size_t)3 * s; }

    template <class Op>
    void launch(const Op &op, double *partials, bool force = false) {
        hipLaunchKernelGGL(mk_stream_kernel<Op>, dim3(mk_grid_stream(n)), dim3(MK_BLOCK), 0, stream, op, n,
                           force ? MkHalt{d_nohalt, 0, 0} : next_halt(), partials);
    }

    GmCols cols(const double *first, int nc) const {        // nc rows from `first` on (the unused entries repeat the first)
        GmCols v;
        for (int c = 0; c < GM_GROUP; ++c) v.col[c] = first + (size_t)(c < nc ? c : 0) * (size_t)ld;
        return v;
    }

    int allocate() {
        if (shadow && (int64_t)want_s > n)
            return mk_fail(MK_ERR_ARG, "IDR: %d shadow vectors were given for %lld rows; at most n make sense", want_s, (long long)n);
        s = (int)((int64_t)want_s < n ? (int64_t)want_s : n);
        if (s < 1) s = 1;
        nslot = (s + GM_GROUP - 1) / GM_GROUP * GM_GROUP;
        ld = ((n + 1) & ~(int64_t)1) + 2;    // n rounded up to even, and the 16 bytes of zeroed slack a product's input needs
        blk_bytes = sizeof(double) * (size_t)3 * (size_t)s * (size_t)ld;
        if (d_blk) return mk_fail(MK_ERR_STATE, "IDR: an earlier set-up of this solver ran out of device memory");
        if (hipMalloc((void **)&d_blk, blk_bytes) != hipSuccess) {
            (void)hipGetLastError();
            d_blk = nullptr;
            return mk_fail(MK_ERR_HIP, "IDR: out of device memory for P, G and U: 3 x %d vectors of %lld rows need %zu bytes; "
                           "a smaller s needs less", s, (long long)n, blk_bytes);
        }
        MK_HIP(hipMemsetAsync(d_blk, 0, blk_bytes, stream));
        if (shadow) {
            MK_HIP(hipMemcpy2DAsync(P(0), sizeof(double) * (size_t)ld, shadow, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n,
                                    (size_t)s, hipMemcpyDeviceToDevice, stream));
        } else {
            for (int i = 0; i < s; ++i) launch(IdOpHashRow{P(i), seed + (uint64_t)i}, d_part, true);
        }
        MK_HIP(hipMalloc((void **)&d_iscal, sizeof(double) * nscal()));
        sc.M = d_iscal;
        sc.f = sc.M + (size_t)s * s;
        sc.c = sc.f + s;
        sc.a = sc.c + s;
        sc.s = s;
        h_iscal.assign(nscal(), 0.0);
        for (int i = 0; i < s; ++i) h_iscal[(size_t)i * s + i] = 1.0;
        const size_t pbytes = sizeof(double) * ((size_t)nslot + 3) * MK_MAXP;
        MK_HIP(hipMalloc((void **)&d_ipart, pbytes));
        MK_HIP(hipMemsetAsync(d_ipart, 0, pbytes, stream));
        int rc;
        if ((rc = alloc_vec(&d_x, nx)) || (rc = alloc_vec(&d_r, nx)) || (rc = alloc_vec(&d_v, nx)) || (rc = alloc_vec(&d_t, n)))
            return rc;
        allocated = true;
        return MK_OK;
    }

    // f = P r of a cycle's start, and c of its step 0
    void enqueue_cycle_start() {
        for (int c0 = 0; c0 < s; c0 += GM_GROUP) {
            const int nc = s - c0 < GM_GROUP ? s - c0 : GM_GROUP;
            launch(GmOpMultiDot{d_r, cols(P(c0), nc), nc}, d_ipart + (size_t)c0 * MK_MAXP);
        }
        hipLaunchKernelGGL(id_cycle_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, d_ipart, np_stream, sc, next_halt());
    }

    void enqueue_norm(int first, int cycle) {
        hipLaunchKernelGGL(id_norm_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, rr_part(), np_stream, d_scal, d_status, d_hist,
                           next_halt(), first, cycle, s, prm.abstol, prm.reltol, prm.matvec_max, nmv);
    }

    int setup(const double *rhs, const double *guess) override {
        int rc;
        if (!allocated && (rc = allocate()) != MK_OK) return rc;
        MK_HIP(hipMemcpyAsync(d_iscal, h_iscal.data(), sizeof(double) * nscal(), hipMemcpyHostToDevice, stream));
        MK_HIP(hipMemsetAsync(G(0), 0, sizeof(double) * (size_t)2 * (size_t)s * (size_t)ld, stream));    // G and U
        k = 0;
        nmv = 0;
        if (guess) {
            MK_HIP(hipMemcpyAsync(d_x, guess, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
            mk_launch_spmv(this, d_x, MkPlainEpi{d_t}, false);                 // r = b - A x0, the product counted
            launch(IdOpResid{rhs, d_t, d_r}, rr_part());
            nmv = 1;
        } else {
            MK_HIP(hipMemsetAsync(d_x, 0, sizeof(double) * (size_t)nx, stream));
            MK_HIP(hipMemcpyAsync(d_r, rhs, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
            launch(MkOpDot<0>{d_r, d_r}, rr_part());
        }
        enqueue_norm(1, 0);
        enqueue_cycle_start();
        return MK_OK;
    }

    // z = precon * v for the one slot: a diagonal by MkOpMul, a general kind through apply_precon (in == out allowed)
    int precondition(const double *v, double *z) {
        if (slot[0].general()) return apply_precon(v, z, false);
        launch(MkOpMul{d_prec(), v, z}, rr_part());
        return MK_OK;
    }

    int enqueue_pass() override {
        int rc;
        const bool pre = slot[0].kind != MK_PRECON_NONE;
        const double *om = d_scal + S_OM;
        // C
        for (int c0 = k; c0 < s; c0 += GM_GROUP) {
            const int nc = s - c0 < GM_GROUP ? s - c0 : GM_GROUP;
            const int first = c0 == k ? 1 : 0;
            const double *vin = first ? d_r : d_v;
            if (c0 + GM_GROUP >= s && !pre)
                launch(IdOpCombine<true>{sc.c + c0, om, vin, d_v, U(k), cols(G(c0), nc), cols(U(c0), nc), nc, first, {}, 0.0}, rr_part());
            else
                launch(IdOpCombine<false>{sc.c + c0, om, vin, d_v, U(k), cols(G(c0), nc), cols(U(c0), nc), nc, first, {}, 0.0}, rr_part());
        }
        if (pre) {
            if ((rc = precondition(d_v, d_v)) != MK_OK) return rc;
            launch(IdOpAxpy{om, d_v, U(k), 0.0}, rr_part());
        }
        // P, D, K
        mk_launch_spmv(this, U(k), MkPlainEpi{G(k)});
        nmv += 1;
        for (int c0 = 0; c0 < s; c0 += GM_GROUP) {
            const int nc = s - c0 < GM_GROUP ? s - c0 : GM_GROUP;
            launch(GmOpMultiDot{G(k), cols(P(c0), nc), nc}, d_ipart + (size_t)c0 * MK_MAXP);
        }
        hipLaunchKernelGGL(id_step_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, d_ipart, np_stream, d_scal, sc, d_status, d_hist,
                           next_halt(), k, nmv);
        // F, N
        const double *beta = d_scal + S_BETA;
        if (k == 0)
            launch(IdOpUpdate<true>{sc.a, beta, G(k), U(k), d_r, d_x, cols(G(0), 0), cols(U(0), 0), 0, {}, 0.0}, rr_part());
        for (int c0 = 0; c0 < k; c0 += GM_GROUP) {
            const int nc = k - c0 < GM_GROUP ? k - c0 : GM_GROUP;
            if (c0 + GM_GROUP >= k)
                launch(IdOpUpdate<true>{sc.a + c0, beta, G(k), U(k), d_r, d_x, cols(G(c0), nc), cols(U(c0), nc), nc, {}, 0.0}, rr_part());
            else
                launch(IdOpUpdate<false>{sc.a + c0, beta, G(k), U(k), d_r, d_x, cols(G(c0), nc), cols(U(c0), nc), nc, {}, 0.0}, rr_part());
        }
        enqueue_norm(0, 0);
        k += 1;
        if (k < s) return MK_OK;
        // the dimension-reduction step (a run that stopped in this step does none of this: the halt word is up)
        const double *v = d_r;
        if (pre) {
            if ((rc = precondition(d_r, d_v)) != MK_OK) return rc;
            v = d_v;
        }
        mk_launch_spmv(this, v, MkPlainEpi{d_t});
        nmv += 1;
        launch(IdOpDot2{d_t, d_r}, tt_part());
        hipLaunchKernelGGL(id_omega_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, tt_part(), np_stream, d_scal, d_status, d_hist,
                           next_halt(), nmv);
        launch(IdOpDrUpdate{om, d_t, v, d_r, d_x, 0.0}, rr_part());
        enqueue_norm(0, 1);
        enqueue_cycle_start();
        k = 0;
        return MK_OK;
    }

    int finish(mk_result *res) override {
        int rc = poll();
        if (rc != MK_OK) return rc;
        fill_result(res);
        res->residNorm = h_scal[S_RESID];
        res->residNorm0 = h_scal[S_RESID0];
        res->threshold = h_scal[S_THRESH];
        res->aux[0] = h_scal[S_S];
        res->aux[1] = h_scal[S_CYCLES];
        res->aux[2] = (double)blk_bytes;
        res->aux[3] = h_scal[S_BREAK];
        return MK_OK;
    }

    const double *x() const override { return d_x; }
    const double *vector(int i) const override { return i == 0 ? d_r : nullptr; }
};

}  // namespace

mk_solver *mk_make_idr() { return new IdrSolver(); }

extern "C" int mk_solver_set_idr(mk_solver *s, int32_t shadow_dim, uint64_t seed, const double *shadow) {
    MK_ARG(s);
    if (s->prm.kind != MK_IDR) return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_set_idr: not an IDR solver");
    if (shadow_dim < 1 || shadow_dim > MK_IDR_MAX_S)
        return mk_fail(MK_ERR_ARG, "mk_solver_set_idr: s = %d, must be 1 .. %d", (int)shadow_dim, MK_IDR_MAX_S);
    IdrSolver *d = static_cast<IdrSolver *>(s);
    if (d->allocated || d->d_blk)
        return mk_fail(MK_ERR_STATE, "mk_solver_set_idr after mk_solver_setup: P, G and U are sized at the first set-up");
    d->want_s = shadow_dim;
    d->seed = seed;
    d->shadow = shadow;
    return MK_OK;
}
