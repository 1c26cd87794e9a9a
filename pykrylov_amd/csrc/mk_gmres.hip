// mk_gmres.hip -- restarted GMRES(m) with right preconditioning, device resident.  No reference module: the
// NumPy restatement is tests/_gmres_ref.py.
//
// One pass of the driver = one Arnoldi step j (1-based) of the current cycle; V = [v_1 .. v_m, u] lives in one allocation:
//   P   z = precon * v_j (none: the column itself)  ;  w = A z                                  [product, in A's format]
//   D   h_i = <v_i, w>, i = 1..j: GM_GROUP columns per launch with one read of w               [ceil(j / GM_GROUP) launches]
//   U   w = w - h_i v_i, i ascending, GM_GROUP columns per launch; the coefficients are totalled in the prologue; the last
//       group of the last orthogonalisation accumulates <w, w> in the same sweep                [ceil(j / GM_GROUP) launches]
//       (reorth: D and U once more on the new w; the lead lane adds the second coefficients to the first)
//   E   one workgroup: hn = sqrt<w,w>, the j - 1 earlier rotations on the column (staged through LDS, lane 0 runs the
//       recurrences), the new rotation, the estimate |g_{j+1}| into the history ring, the status record, the stop tests
//   S   v_{j+1} = (1 / hn) w                                                                    [stream; not after step m]
// The pass of step m goes on with the cycle end -- B: back substitution R y = g in one workgroup; C: u = sum y_i v_i in
// groups; u = precon * u; x += u -- the residual r = b - A x with <r, r> fused into the subtraction, R: the loop test on
// beta = sqrt<r, r>, and v_1 = (1 / beta) r.  A run that halts inside a cycle (converged, out of products, breakdown) leaves
// its cycle end to `drain`, which runs it once under the never-raised halt words, sized by the step count the device kept.
//
// Launches per step: 1 + (1 + reorth) * 2 * ceil(j / GM_GROUP) + 2 plus the preconditioner's.  Bytes per step: the product +
// (1 + reorth) * (16 j + 24 ceil(j / GM_GROUP)) n + 16 n.  The step index within the cycle and the number of products are
// host knowledge (like GateB::nmv in mk_bicgstab.hip); every scalar stays on the device.  Every operation rounds on its own
// (-ffp-contract=off); every dot has the lanes, the grid and the tree of mk_stream_kernel<MkOpDot>, then mk_total.
#include <cmath>

#include "mk_multicol.h"      // GM_GROUP, GmCols and D, U and C: the many-column dot, update and combination
#include "mk_solver.h"

namespace {

constexpr int GM_MAXR = MK_GMRES_MAX_RESTART;

// the shared scalar file (poll() brings it to the host)
enum { S_THRESH = 0, S_RESID = 1, S_RESID0 = 2, S_BETA = 3, S_HN = 4, S_J = 5, S_RESTARTS = 6, S_LASTJ = 7 };

// GMRES' own scalar file: the column being orthogonalised, R (column k at r + k * m), the rotations, g and y
struct GmScal {
    double *h, *r, *c, *s, *g, *y;
    int m;
};

struct GmOpScale {              // out = (1 / *d) * in
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *d;
    const double *in;
    double *out;
    double s;
    __device__ bool prologue(double *, bool) {
        s = 1.0 / d[0];
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 v = mk_ld2(in, i);
        v.x = s * v.x;
        v.y = s * v.y;
        mk_st2(out, i, v);
    }
    __device__ void one(int64_t i, double *) { out[i] = s * in[i]; }
};

struct GmOpResid {              // r = b - t ; partial <r, r>
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

// beta = sqrt<r, r> of a cycle's start and the loop test on it.  first: the set-up (threshold, history[0]); otherwise the
// restart after a cycle end, whose residual product is the run's product number `nmv`.
__global__ __launch_bounds__(MK_BLOCK) void gm_start_kernel(const double *rr_part, int np, double *scal, GmScal gs, MkStatus *st,
                                                            double *hist, MkHalt halt, int first, double abstol, double reltol,
                                                            int64_t matvec_max, int64_t nmv) {
    __shared__ double s4[4];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double beta = __dsqrt_rn(mk_total(rr_part, np, s4));
    if (threadIdx.x == 0) {
        double thresh = scal[S_THRESH];
        if (first) {
            const double rel = reltol * beta;
            thresh = (rel > abstol) ? rel : abstol;
            scal[S_THRESH] = thresh;
            scal[S_RESID0] = beta;
            hist[0] = beta;
            st->hist_len = 1;
            st->itn = 0;
        } else {
            scal[S_RESTARTS] = scal[S_RESTARTS] + 1.0;
        }
        scal[S_BETA] = beta;
        scal[S_RESID] = beta;
        scal[S_J] = 0.0;
        gs.g[0] = beta;
        st->nMatvec = nmv;
        st->converged = (beta <= thresh) ? 1 : 0;
        halt.out(!(beta > thresh) || nmv >= matvec_max);
    }
}

// E: the end of step jc + 1 (jc steps of the cycle are behind it), whose product was the run's product number nmv
__global__ __launch_bounds__(MK_BLOCK) void gm_step_kernel(const double *ww_part, int np, double *scal, GmScal gs, MkStatus *st,
                                                           double *hist, MkHalt halt, int jc, int64_t matvec_max, int64_t nmv) {
    __shared__ double s4[4];
    __shared__ double a[GM_MAXR + 1], rc[GM_MAXR], rs[GM_MAXR];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double hn = __dsqrt_rn(mk_total(ww_part, np, s4));
    const int t = (int)threadIdx.x;
    if (t <= jc) a[t] = gs.h[t];
    if (t < jc) {
        rc[t] = gs.c[t];
        rs[t] = gs.s[t];
    }
    __syncthreads();
    if (t == 0) {
        for (int i = 0; i < jc; ++i) {
            const double u = rc[i] * a[i] + rs[i] * a[i + 1];
            a[i + 1] = rc[i] * a[i + 1] - rs[i] * a[i];
            a[i] = u;
        }
        const double aj = a[jc];
        const double rr = __dsqrt_rn(aj * aj + hn * hn);
        const double c = aj / rr, s = hn / rr;
        const double gj = gs.g[jc];
        const double gnext = -s * gj;
        const double est = fabs(gnext);
        const bool bad = !isfinite(hn) || !isfinite(rr) || !isfinite(est) || rr == 0.0;
        const double thresh = scal[S_THRESH];
        hist[st->hist_len % MK_HIST_RING] = est;
        st->hist_len += 1;
        st->itn += 1;
        st->nMatvec = nmv;
        scal[S_RESID] = est;
        scal[S_HN] = hn;
        if (!bad) {                                            // (a discarded step leaves the cycle where it was)
            for (int i = 0; i < jc; ++i) gs.r[(size_t)jc * gs.m + i] = a[i];
            gs.r[(size_t)jc * gs.m + jc] = rr;
            gs.c[jc] = c;
            gs.s[jc] = s;
            gs.g[jc + 1] = gnext;
            gs.g[jc] = c * gj;
            scal[S_J] = (double)(jc + 1);
            scal[S_LASTJ] = (double)(jc + 1);
        } else {
            scal[S_LASTJ] = (double)jc;
        }
        st->converged = (!bad && est <= thresh) ? 1 : 0;
        halt.out(bad || est <= thresh || !(hn > 0.0) || nmv >= matvec_max);
    }
}

// B: y of R y = g for the j leading rows; row i's entries are staged through LDS by one lane each (the next row's are in
// flight meanwhile), lane 0 runs the substitution in the order t = g_i ; t = t - R_ik y_k, k ascending ; y_i = t / R_ii
__global__ __launch_bounds__(MK_BLOCK) void gm_back_kernel(GmScal gs, MkHalt halt, int j) {
    __shared__ double row[GM_MAXR], y[GM_MAXR];
    const int t = (int)threadIdx.x;
    if (halt.in()) {
        if (t == 0) halt.out(true);
        return;
    }
    if (t == 0) halt.out(false);
    const int m = gs.m;
    double nxt = 0.0;
    if (j > 0 && t >= j - 1 && t < j) nxt = gs.r[(size_t)t * m + (j - 1)];
    for (int i = j - 1; i >= 0; --i) {
        if (t >= i && t < j) row[t] = nxt;
        __syncthreads();
        if (i > 0 && t >= i - 1 && t < j) nxt = gs.r[(size_t)t * m + (i - 1)];
        if (t == 0) {
            double v = gs.g[i];
            for (int k = i + 1; k < j; ++k) v = v - row[k] * y[k];
            y[i] = v / row[i];
        }
        __syncthreads();
    }
    if (t < j) gs.y[t] = y[t];
}

struct GmresSolver : mk_solver {
    double *d_x = nullptr, *d_w = nullptr, *d_z = nullptr, *d_b = nullptr;
    double *d_V = nullptr;           // m + 1 columns of ld doubles: v_1 .. v_m and u of the cycle end
    double *d_gscal = nullptr;       // GmScal's storage
    double *d_gpart = nullptr;       // two banks of `nslot` coefficient slots, then <w,w> and <r,r>
    GmScal gs{};
    int m = 0, nslot = 0;
    int64_t ld = 0;
    size_t basis_bytes = 0;
    int jc = 0;                      // steps of the current cycle enqueued so far
    int64_t nmv = 0;                 // products enqueued so far
    bool end_applied = false;        // the cycle end of a halted run has been enqueued
    bool allocated = false;
    bool takes_precon() const override { return true; }

    ~GmresSolver() override {
        if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
        hipFree(d_V);
        hipFree(d_gscal);
        hipFree(d_gpart);
    }

    double *col(int k) const { return d_V + (size_t)k * (size_t)ld; }
    double *bank(int b) const { return d_gpart + (size_t)b * nslot * MK_MAXP; }
    double *ww_part() const { return d_gpart + (size_t)2 * nslot * MK_MAXP; }
    double *rr_part() const { return ww_part() + MK_MAXP; }
    MkHalt halt_for(bool force) { return force ? MkHalt{d_nohalt, 0, 0} : next_halt(); }

    template <class Op>
    void launch(const Op &op, double *partials, bool force = false) {
        hipLaunchKernelGGL(mk_stream_kernel<Op>, dim3(mk_grid_stream(n)), dim3(MK_BLOCK), 0, stream, op, n, halt_for(force),
                           partials);
    }

    GmCols cols(int c0, int nc) const {
        GmCols v;
        for (int c = 0; c < GM_GROUP; ++c) v.col[c] = col(c0 + (c < nc ? c : 0));
        return v;
    }

    int allocate() {
        m = (int)((int64_t)prm.restart < n ? (int64_t)prm.restart : n);
        if (m < 1) m = 1;
        nslot = (m + GM_GROUP - 1) / GM_GROUP * GM_GROUP;
        ld = ((n + 1) & ~(int64_t)1) + 2;    // n rounded up to even, and the 16 bytes of zeroed slack a product's input needs
        basis_bytes = sizeof(double) * (size_t)(m + 1) * (size_t)ld;
        if (d_V) return mk_fail(MK_ERR_STATE, "GMRES: an earlier set-up of this solver ran out of device memory");
        if (hipMalloc((void **)&d_V, basis_bytes) != hipSuccess) {
            (void)hipGetLastError();
            d_V = nullptr;
            return mk_fail(MK_ERR_HIP, "GMRES: out of device memory for the basis: %d + 1 columns of %lld rows need %zu bytes; "
                           "a smaller restart needs less", m, (long long)n, basis_bytes);
        }
        MK_HIP(hipMemsetAsync(d_V, 0, basis_bytes, stream));
        const size_t nscal = (size_t)m * m + (size_t)5 * m + 2;
        MK_HIP(hipMalloc((void **)&d_gscal, sizeof(double) * nscal));
        double *p = d_gscal;
        gs.h = p, p += m + 1;
        gs.r = p, p += (size_t)m * m;
        gs.c = p, p += m;
        gs.s = p, p += m;
        gs.g = p, p += m + 1;
        gs.y = p;
        gs.m = m;
        const size_t pbytes = sizeof(double) * ((size_t)2 * nslot + 2) * MK_MAXP;
        MK_HIP(hipMalloc((void **)&d_gpart, pbytes));
        MK_HIP(hipMemsetAsync(d_gpart, 0, pbytes, stream));
        int rc;
        if ((rc = alloc_vec(&d_x, nx)) || (rc = alloc_vec(&d_w, n)) || (rc = alloc_vec(&d_b, n))) return rc;
        allocated = true;
        return MK_OK;
    }

    int setup(const double *rhs, const double *guess) override {
        int rc;
        if (!allocated && (rc = allocate()) != MK_OK) return rc;
        if (slot[0].kind != MK_PRECON_NONE && !d_z && (rc = alloc_vec(&d_z, nx)) != MK_OK) return rc;
        MK_HIP(hipMemsetAsync(d_gscal, 0, sizeof(double) * ((size_t)m * m + (size_t)5 * m + 2), stream));
        jc = 0;
        nmv = 0;
        end_applied = false;
        MK_HIP(hipMemcpyAsync(d_b, rhs, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
        if (guess) {
            MK_HIP(hipMemcpyAsync(d_x, guess, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
            mk_launch_spmv(this, d_x, MkPlainEpi{d_w}, false);                 // r = b - A x0, the product counted
            launch(GmOpResid{d_b, d_w, col(0)}, rr_part());
            nmv = 1;
        } else {
            MK_HIP(hipMemsetAsync(d_x, 0, sizeof(double) * (size_t)nx, stream));
            launch(MkOpCopy{d_b, col(0)}, rr_part());                          // r = b
            launch(MkOpDot<0>{col(0), col(0)}, rr_part());
        }
        hipLaunchKernelGGL(gm_start_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, rr_part(), np_stream, d_scal, gs, d_status,
                           d_hist, next_halt(), 1, prm.abstol, prm.reltol, prm.matvec_max, nmv);
        launch(GmOpScale{d_scal + S_BETA, col(0), col(0), 0.0}, rr_part());    // v_1 = (1 / beta) r
        return MK_OK;
    }

    // z = precon * v for the one slot: a diagonal by MkOpMul, a general kind through apply_precon (in == out allowed)
    int precondition(const double *v, double *z, bool force) {
        if (slot[0].general()) return apply_precon(v, z, force);
        launch(MkOpMul{d_prec(), v, z}, rr_part(), force);
        return MK_OK;
    }

    // B, C, u = precon * u, x += u for a cycle of j steps
    int enqueue_cycle_end(int j, bool force) {
        double *u = col(m);
        hipLaunchKernelGGL(gm_back_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, gs, halt_for(force), j);
        for (int c0 = 0; c0 < j; c0 += GM_GROUP) {
            const int nc = j - c0 < GM_GROUP ? j - c0 : GM_GROUP;
            launch(GmOpCombine{gs.y + c0, u, cols(c0, nc), nc, c0 == 0 ? 1 : 0, {}}, rr_part(), force);
        }
        int rc;
        if (slot[0].kind != MK_PRECON_NONE && (rc = precondition(u, u, force)) != MK_OK) return rc;
        launch(MkOpAddTo<1>{u, d_x}, rr_part(), force);
        return MK_OK;
    }

    int enqueue_pass() override {
        int rc;
        const double *zin = col(jc);
        if (slot[0].kind != MK_PRECON_NONE) {
            if ((rc = precondition(col(jc), d_z, false)) != MK_OK) return rc;
            zin = d_z;
        }
        mk_launch_spmv(this, zin, MkPlainEpi{d_w});
        nmv += 1;
        const int ncol = jc + 1, passes = prm.reorth ? 2 : 1;
        for (int p = 0; p < passes; ++p) {
            for (int c0 = 0; c0 < ncol; c0 += GM_GROUP) {
                const int nc = ncol - c0 < GM_GROUP ? ncol - c0 : GM_GROUP;
                launch(GmOpMultiDot{d_w, cols(c0, nc), nc}, bank(p) + (size_t)c0 * MK_MAXP);
            }
            for (int c0 = 0; c0 < ncol; c0 += GM_GROUP) {
                const int nc = ncol - c0 < GM_GROUP ? ncol - c0 : GM_GROUP;
                const bool last = p + 1 == passes && c0 + GM_GROUP >= ncol;
                if (last)
                    launch(GmOpUpdate<true>{bank(p) + (size_t)c0 * MK_MAXP, np_stream, gs.h + c0, p, d_w, cols(c0, nc), nc, {}},
                           ww_part());
                else
                    launch(GmOpUpdate<false>{bank(p) + (size_t)c0 * MK_MAXP, np_stream, gs.h + c0, p, d_w, cols(c0, nc), nc, {}},
                           ww_part());
            }
        }
        hipLaunchKernelGGL(gm_step_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, ww_part(), np_stream, d_scal, gs, d_status,
                           d_hist, next_halt(), jc, prm.matvec_max, nmv);
        jc += 1;
        if (jc < m) {
            launch(GmOpScale{d_scal + S_HN, d_w, col(jc), 0.0}, rr_part());    // v_{j+1} = (1 / hn) w
            return MK_OK;
        }
        // the cycle is full (a run that stopped in this step does none of this: the halt word is up)
        if ((rc = enqueue_cycle_end(m, false)) != MK_OK) return rc;
        mk_launch_spmv(this, d_x, MkPlainEpi{d_w});
        nmv += 1;
        launch(GmOpResid{d_b, d_w, col(0)}, rr_part());
        hipLaunchKernelGGL(gm_start_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, rr_part(), np_stream, d_scal, gs, d_status,
                           d_hist, next_halt(), 0, prm.abstol, prm.reltol, prm.matvec_max, nmv);
        launch(GmOpScale{d_scal + S_BETA, col(0), col(0), 0.0}, rr_part());
        jc = 0;
        return MK_OK;
    }

    // the cycle end of a run that halted inside a cycle: once, after the halt has been observed (poll), for the steps the
    // device counted
    int drain() override {
        if (!halted || end_applied) return MK_OK;
        end_applied = true;
        const int j = (int)h_scal[S_J];
        if (j < 1 || j > m) return MK_OK;                      // (halted at a cycle's start: x is complete)
        const int rc = enqueue_cycle_end(j, true);
        if (rc != MK_OK) return rc;
        MK_HIP(hipGetLastError());
        return mk_ctx().pending_rc;
    }

    int finish(mk_result *res) override {
        int rc = poll();
        if (rc != MK_OK) return rc;
        fill_result(res);
        res->residNorm = h_scal[S_RESID];
        res->residNorm0 = h_scal[S_RESID0];
        res->threshold = h_scal[S_THRESH];
        res->aux[0] = h_scal[S_RESTARTS];
        res->aux[1] = h_scal[S_LASTJ];
        res->aux[2] = (double)basis_bytes;
        return MK_OK;
    }

    const double *x() const override { return d_x; }
    const double *vector(int i) const override { return i == 0 ? d_w : nullptr; }
};

}  // namespace

mk_solver *mk_make_gmres() { return new GmresSolver(); }
