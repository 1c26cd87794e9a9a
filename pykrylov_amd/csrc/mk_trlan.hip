// mk_trlan.hip -- thick-restart Lanczos (Wu and Simon) for a few extreme eigenpairs of a symmetric operator, device resident
// (solver kind MK_TRLAN; no reference module).  The NumPy restatement is tests/_trlan_ref.py.
//
// One pass of the driver = one whole cycle; V = [v_1 .. v_m, v_{m+1}, spare columns] lives in one allocation (m = ncv).
// Step j (1-based) of a cycle that starts behind l kept Ritz vectors, j = l + 1 .. m:
//   P   w = A v_j                                                                            [product, in A's format]
//   D   h_i = <v_i, w>, i = 1..j: GM_GROUP columns per launch with one read of w             [ceil(j / GM_GROUP) launches]
//   U   w = w - h_i v_i, i ascending, GM_GROUP columns per launch; D and U run twice, the lead lane adds the second
//       coefficients to the first, and the last group of the second U accumulates <w, w>    [ceil(j / GM_GROUP) launches]
//   E   one workgroup, one lane writes: alpha_j = h_j, beta_{j+1} = sqrt<w, w>, tmax, the counts, and the breakdown test
//       beta_{j+1} not > 2^-26 tmax (mk_lanczos.hip's), which raises the halt words: the rest of the cycle does nothing
//   S   v_{j+1} = (1 / beta_{j+1}) w                                                         [stream]
// The cycle ends on the host: one download of alpha, beta and the status, the eigenproblem of the m x m projected matrix
// (diag(theta_kept), the arrow beta S[m, kept] in row and column l + 1, tridiagonal behind it) by cyclic Jacobi, the stop
// tests, one upload of the rotation coefficients, and
//   R   V[:, :keep] = V[:, :m] S[:, kept]  (the end of the run: X = V S[:, wanted])          [ceil(kk / TR_KT) launches]
// a lane owning a pair of rows, walking the m columns once with up to TR_KT accumulators per row; the coefficients sit in
// LDS and are read as broadcasts.  The last group of columns is rotated in place (a lane writes a row after it has read all
// of it, and no other lane touches that row); the groups before it go to the spare columns and are copied down afterwards.
// Then v_{l+1} = v_{m+1} and the next cycle.  (mk_params.window != 0: the same rotation composed of GmOpCombine launches,
// one output column at a time into spare columns -- V is read once per output column; same bits; what tools/trlan_bench.py
// measures R against.)
//
// With a Chebyshev filter (the block mk_params_filter, mk_chebfilt.hip; the restatement is tests/_chebfilt_ref.py) P is
// w = rho(A) v_j, `degree` launches of the product kernel, and the cycle wants B's largest Ritz values whatever `which` says.
// B's estimates only open a gate: once it has been met, and in the last cycle the budget allows, the restart rotation is
// followed by the verification on A (`verify`): per wanted vector one plain product, <x, A x>, and ||A x - theta x||.
//
// Launches per step: 1 + 4 ceil(j / GM_GROUP) + 2.  Bytes per step: the product + 2 (16 j + 24 ceil(j / GM_GROUP)) n + 16 n.
// Bytes per rotation of kk columns: 8 n (m ceil(kk / TR_KT) + kk), plus 16 n per column copied down (kk > TR_KT).
// Every operation rounds on its own (-ffp-contract=off); every dot has the lanes, the grid and the tree of
// mk_stream_kernel<MkOpDot>, then mk_total.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "mk_multicol.h"
#include "mk_rotate.h"
#include "mk_solver.h"

namespace {

constexpr int TR_KT = 16;                                    // output columns per rotation launch

// the shared scalar file (poll() brings it to the host)
enum { S_B0 = 0, S_BETA = 1, S_TMAX = 2, S_J = 3, S_BREAK = 4 };

// the cycle's own scalar file: alpha_j and beta_{j+1} by step (one download per cycle), and the column being orthogonalised
struct TrScal {
    double *alpha, *beta, *h;
};

struct TrOpStart {              // out = start (or the hashed vector) ; partial <out, out>
    static constexpr int NACC = 1, SLOT0 = 0;
    const double *start;
    double *out;
    uint64_t seed;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        double2 v;
        if (start) {
            v = mk_ld2(start, i);
        } else {
            v.x = mk_cell_field(i, seed) - 1.0;
            v.y = mk_cell_field(i + 1, seed) - 1.0;
        }
        mk_st2(out, i, v);
        acc[0] += v.x * v.x;
        acc[0] += v.y * v.y;
    }
    __device__ void one(int64_t i, double *acc) {
        const double v = start ? start[i] : mk_cell_field(i, seed) - 1.0;
        out[i] = v;
        acc[0] += v * v;
    }
};

struct TrOpScale {              // out = (1 / *d) * in
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

// ||start|| and the test on it: a start vector without a positive, finite norm halts the run before its first step
__global__ __launch_bounds__(MK_BLOCK) void tr_start_kernel(const double *rr_part, int np, double *scal, MkHalt halt) {
    __shared__ double s4[4];
    const double b0 = __dsqrt_rn(mk_total(rr_part, np, s4));
    if (threadIdx.x == 0) {
        scal[S_B0] = b0;
        halt.out(!(isfinite(b0) && b0 > 0.0));
    }
}

// E: the end of the step on column jc (0-based), after which the run has made nmv products; `later`: not the run's first step
__global__ __launch_bounds__(MK_BLOCK) void tr_step_kernel(const double *ww_part, int np, double *scal, TrScal ts, MkStatus *st,
                                                           MkHalt halt, int jc, int64_t nmv, int later) {
    __shared__ double s4[4];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double beta = __dsqrt_rn(mk_total(ww_part, np, s4));
    if (threadIdx.x == 0) {
        const double alpha = ts.h[jc];
        double tm = fabs(alpha);
        if (later) tm = tm + scal[S_BETA];                    // (beta_j: of the step before, in this cycle or the last one)
        const double t0 = scal[S_TMAX];
        const double tmax = tm > t0 ? tm : t0;
        const bool stop = !(beta > 0x1.0p-26 * tmax);
        ts.alpha[jc] = alpha;
        ts.beta[jc] = beta;
        scal[S_BETA] = beta;
        scal[S_TMAX] = tmax;
        scal[S_J] = (double)(jc + 1);
        scal[S_BREAK] = stop ? 1.0 : 0.0;
        st->itn += 1;
        st->nMatvec = nmv;
        halt.out(stop);
    }
}

// Verification of a filtered run (mk_params_filter) on A itself: w = A x by the plain product, <x, w> by MkOpDot, then
//   t = w - theta x, theta the total of that dot; partial <t, t>; the lead lane leaves theta in the record
struct TrOpResid {
    static constexpr int NACC = 1, SLOT0 = 1;
    const double *part;         // slot 0: the partials of <x, A x>
    int np;
    const double *x, *w;
    double *rec;                // rec[0] = theta
    double theta;
    __device__ bool prologue(double *s4, bool lead) {
        theta = mk_total(part, np, s4);
        if (lead) rec[0] = theta;
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        const double2 xv = mk_ld2(x, i), wv = mk_ld2(w, i);
        const double t0 = wv.x - theta * xv.x, t1 = wv.y - theta * xv.y;
        acc[0] += t0 * t0;
        acc[0] += t1 * t1;
    }
    __device__ void one(int64_t i, double *acc) {
        const double t = w[i] - theta * x[i];
        acc[0] += t * t;
    }
};

// rec[1] = ||A x - theta x|| from the partials TrOpResid left in slot 1
__global__ __launch_bounds__(MK_BLOCK) void tr_resid_kernel(const double *rr_part, int np, double *rec) {
    __shared__ double s4[4];
    const double r = __dsqrt_rn(mk_total(rr_part, np, s4));
    if (threadIdx.x == 0) rec[1] = r;
}

// (R, tr_rotate_kernel, and the Jacobi solver of the small eigenproblem, tr_jacobi, live in mk_rotate.h: LOBPCG shares them)

struct TrlanSolver : mk_solver {
    double *d_w = nullptr;
    double *d_V = nullptr;           // m + 1 + spare columns of ld doubles
    double *d_tscal = nullptr;       // TrScal's storage, then the record of 3 nev doubles
    double *d_tpart = nullptr;       // two banks of `nslot` coefficient slots, then <w, w> and <start, start>
    double *d_Y = nullptr;           // the rotation coefficients, group after group
    double *h_ab = nullptr, *h_Y = nullptr;   // pinned: alpha and beta of a cycle; the coefficients and the record on their way up
    hipEvent_t rot0 = nullptr, rot1 = nullptr;
    TrScal ts{};
    int m = 0, nev = 0, keep = 0, which = 0, nslot = 0, spare = 0;
    int64_t ld = 0;
    size_t basis_bytes = 0, ybytes = 0;
    bool allocated = false;
    // the run's host state
    std::vector<double> T, ja, js, theta, est;
    std::vector<int> order, first_met;
    int l = 0, cycles = 0, sweeps = 0, nconv = 0, breakdown = 0, conv = 0;
    bool finished = false, rotated = false;
    int64_t nmv = 0;
    double anorm = 0.0, threshold = 0.0, resid = 0.0, b0 = 0.0, rot_ms = 0.0;
    int64_t steps = 0;               // Lanczos steps enqueued so far
    // the filtered cycle (mk_params_filter): Lanczos on B = rho(A), verified on A
    mk_filter *filt = nullptr;       // (owned)
    const MkDeviceOp *fop = nullptr; // the filter as the device operator it is
    int fdeg = 0;
    bool probe = false;              // mk_params.restart = 1: set-up applies the filter to its vector and ends the run
    double *d_ftab = nullptr;        // the filter's table (mk_solver_vector(nev + 1))
    int64_t ntab = 0;
    double anorm_a = 0.0, thr_a = 0.0;   // max(|a|, |b|, |a0|) and max(abstol, reltol anorm_a): fixed for the run
    double *d_vpart = nullptr;       // two slots of partial sums, then 2 nev doubles: theta_i and ||A x_i - theta_i x_i||
    bool verifying = false;          // B's gate has been met: every cycle from now on is verified on A
    std::vector<double> th_a, res_a; // ... of the last verification, by kept column
    std::vector<int> perm;           // returned pair i (theta_A ascending) is kept column perm[i]

    ~TrlanSolver() override {
        if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
        hipFree(d_vpart);
        hipFree(d_ftab);
        if (filt) mk_filter_free(filt);
        hipFree(d_V);
        hipFree(d_tscal);
        hipFree(d_tpart);
        hipFree(d_Y);
        if (h_ab) hipHostFree(h_ab);
        if (h_Y) hipHostFree(h_Y);
        if (rot0) hipEventDestroy(rot0);
        if (rot1) hipEventDestroy(rot1);
    }

    double *col(int k) const { return d_V + (size_t)k * (size_t)ld; }
    double *bank(int b) const { return d_tpart + (size_t)b * nslot * MK_MAXP; }
    double *ww_part() const { return d_tpart + (size_t)2 * nslot * MK_MAXP; }
    double *rr_part() const { return ww_part() + MK_MAXP; }
    double *d_rec() const { return d_tscal + (size_t)3 * m; }
    double *d_vrec() const { return d_vpart + (size_t)2 * MK_MAXP; }

    // The tail of mk_params_filter (mk_solver_create): the solver creates the filter and owns it.  prm.restart = 1 is the
    // probe -- no Lanczos run, set-up applies the filter to its vector --, whose `which` means nothing.
    int make_filter(int32_t degree, double a, double b, double a0) override {
        if (prm.restart != 0 && prm.restart != 1)
            return mk_fail(MK_ERR_ARG, "mk_solver_create: thick-restart Lanczos with a filter takes restart = 0 (the solver) or 1 "
                           "(the probe), got %d", (int)prm.restart);
        mk_filter *F = nullptr;
        int rc = mk_filter_create(A, degree, a, b, a0, &F);
        if (rc != MK_OK) return rc;
        const mk_csr *FA = nullptr;
        mk_filter_describe(F, &FA, &fdeg, &a, &b, &a0);
        probe = prm.restart == 1;
        if (!probe && (a0 > b ? 1 : 0) != eig_which) {
            mk_filter_free(F);
            return mk_fail(MK_ERR_ARG, "mk_solver_create: the filter's reference point lies %s its interval: it wants the %s "
                           "eigenvalues, `which` the %s", a0 > b ? "above" : "below", a0 > b ? "largest" : "smallest",
                           eig_which ? "largest" : "smallest");
        }
        filt = F;
        fop = mk_filter_as_op(F);
        anorm_a = std::max(std::fabs(a), std::max(std::fabs(b), std::fabs(a0)));
        const std::vector<double> t = mk_filter_table(F);
        ntab = (int64_t)t.size();
        MK_HIP(hipMalloc((void **)&d_ftab, sizeof(double) * t.size()));
        MK_HIP(hipMemcpy(d_ftab, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice));
        return MK_OK;
    }

    template <class Op>
    void launch(const Op &op, double *partials) {
        hipLaunchKernelGGL(mk_stream_kernel<Op>, dim3(mk_grid_stream(n)), dim3(MK_BLOCK), 0, stream, op, n, next_halt(), partials);
    }

    GmCols cols(int c0, int nc) const {
        GmCols v;
        for (int c = 0; c < GM_GROUP; ++c) v.col[c] = col(c0 + (c < nc ? c : 0));
        return v;
    }

    int allocate() {
        m = eig_ncv;
        nev = eig_nev;
        keep = eig_keep;
        which = eig_which;
        nslot = (m + GM_GROUP - 1) / GM_GROUP * GM_GROUP;
        spare = TR_KT * ((keep + TR_KT - 1) / TR_KT - 1);
        if (prm.window) spare = keep;                          // (the composed rotation writes every column out of place)
        ld = ((n + 1) & ~(int64_t)1) + 2;    // n rounded up to even, and the 16 bytes of zeroed slack a product's input needs
        basis_bytes = sizeof(double) * (size_t)(m + 1 + spare) * (size_t)ld;
        if (d_V) return mk_fail(MK_ERR_STATE, "thick-restart Lanczos: an earlier set-up of this solver ran out of device memory");
        if (hipMalloc((void **)&d_V, basis_bytes) != hipSuccess) {
            (void)hipGetLastError();
            d_V = nullptr;
            return mk_fail(MK_ERR_HIP, "thick-restart Lanczos: out of device memory for the basis: %d + 1 + %d columns of %lld rows "
                           "need %zu bytes; a smaller ncv needs less", m, spare, (long long)n, basis_bytes);
        }
        MK_HIP(hipMemsetAsync(d_V, 0, basis_bytes, stream));
        MK_HIP(hipMalloc((void **)&d_tscal, sizeof(double) * ((size_t)3 * m + (size_t)3 * nev)));
        ts.alpha = d_tscal;
        ts.beta = d_tscal + m;
        ts.h = d_tscal + 2 * m;
        const size_t pbytes = sizeof(double) * ((size_t)2 * nslot + 2) * MK_MAXP;
        MK_HIP(hipMalloc((void **)&d_tpart, pbytes));
        MK_HIP(hipMemsetAsync(d_tpart, 0, pbytes, stream));
        // a rotation's coefficients: at most ceil(keep / TR_KT) groups of m x TR_KT; the record travels through the same buffer
        ybytes = sizeof(double) * std::max((size_t)m * (size_t)(spare + TR_KT), (size_t)3 * nev);
        MK_HIP(hipMalloc((void **)&d_Y, ybytes));
        MK_HIP(hipHostMalloc((void **)&h_Y, ybytes, hipHostMallocDefault));
        MK_HIP(hipHostMalloc((void **)&h_ab, sizeof(double) * (size_t)2 * m, hipHostMallocDefault));
        MK_HIP(hipEventCreate(&rot0));
        MK_HIP(hipEventCreate(&rot1));
        int rc;
        if ((rc = alloc_vec(&d_w, n)) != MK_OK) return rc;
        allocated = true;
        return MK_OK;
    }

    int setup(const double *start, const double *guess) override {
        if (guess)
            return mk_fail(MK_ERR_ARG, "mk_solver_setup: thick-restart Lanczos takes a start vector and no initial guess");
        if (probe) {
            if (!start) return mk_fail(MK_ERR_ARG, "mk_solver_setup: the filter probe takes the vector to apply the filter to");
            int prc;
            if (!d_w && (prc = alloc_vec(&d_w, n)) != MK_OK) return prc;
            if ((prc = fop->enqueue(start, d_w, stream, nullptr, nullptr)) != MK_OK) return prc;
            static const int up[2] = {1, 1};
            MK_HIP(hipMemcpyAsync(d_halt, up, sizeof(up), hipMemcpyHostToDevice, stream));
            MK_HIP(hipStreamSynchronize(stream));
            finished = true;
            return MK_OK;
        }
        if (prm.matvec_max < (int64_t)eig_ncv)
            return mk_fail(MK_ERR_ARG, "mk_solver_setup: thick-restart Lanczos matvec_max = %lld is below ncv = %d: the first cycle "
                           "does not fit", (long long)prm.matvec_max, eig_ncv);
        if (filt && prm.matvec_max < (int64_t)eig_ncv * fdeg + eig_nev)
            return mk_fail(MK_ERR_ARG, "mk_solver_setup: filtered thick-restart Lanczos matvec_max = %lld is below ncv * degree + "
                           "nev = %lld: the first cycle and its verification do not fit", (long long)prm.matvec_max,
                           (long long)eig_ncv * fdeg + eig_nev);
        int rc;
        if (!allocated && (rc = allocate()) != MK_OK) return rc;
        if (filt && !d_vpart) {
            const size_t vb = sizeof(double) * ((size_t)2 * MK_MAXP + (size_t)2 * eig_nev);
            MK_HIP(hipMalloc((void **)&d_vpart, vb));
            MK_HIP(hipMemsetAsync(d_vpart, 0, vb, stream));
        }
        verifying = false;
        steps = 0;
        th_a.assign(nev, 0.0);
        res_a.assign(nev, 0.0);
        perm.resize(nev);
        for (int i = 0; i < nev; ++i) perm[i] = i;
        const double rel_a = prm.reltol * anorm_a;
        thr_a = rel_a > prm.abstol ? rel_a : prm.abstol;
        MK_HIP(hipMemsetAsync(d_tscal, 0, sizeof(double) * ((size_t)3 * m + (size_t)3 * nev), stream));
        T.assign((size_t)m * m, 0.0);
        ja.assign((size_t)m * m, 0.0);
        js.assign((size_t)m * m, 0.0);
        theta.assign(m, 0.0);
        est.assign(m, 0.0);
        order.assign(m, 0);
        first_met.assign(nev, -1);
        l = cycles = sweeps = nconv = breakdown = conv = 0;
        finished = rotated = false;
        nmv = 0;
        anorm = threshold = resid = rot_ms = 0.0;
        launch(TrOpStart{start, col(0), eig_seed}, rr_part());
        hipLaunchKernelGGL(tr_start_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, rr_part(), np_stream, d_scal, next_halt());
        launch(TrOpScale{d_scal + S_B0, col(0), col(0), 0.0}, rr_part());      // v_1 = (1 / ||start||) start
        MK_HIP(hipMemcpyAsync(h_ab, d_scal + S_B0, sizeof(double), hipMemcpyDeviceToHost, stream));
        MK_HIP(hipStreamSynchronize(stream));
        b0 = h_ab[0];
        if (!(std::isfinite(b0) && b0 > 0.0))
            return mk_fail(MK_ERR_ARG, "mk_solver_setup: thick-restart Lanczos: ||start|| = %g, the start vector must have a "
                           "positive, finite norm", b0);
        return MK_OK;
    }

    void enqueue_step(int jc) {
        if (filt) {                                            // w = rho(A) v_j: fdeg products under the loop's halt words
            const int rc = fop->enqueue(col(jc), d_w, stream, d_halt, &q);
            if (rc != MK_OK && mk_ctx().pending_rc == MK_OK) mk_ctx().pending_rc = rc;
            nmv += fdeg;
        } else {
            mk_launch_spmv(this, col(jc), MkPlainEpi{d_w});
            nmv += 1;
        }
        const int ncol = jc + 1;
        for (int p = 0; p < 2; ++p) {
            for (int c0 = 0; c0 < ncol; c0 += GM_GROUP) {
                const int nc = ncol - c0 < GM_GROUP ? ncol - c0 : GM_GROUP;
                launch(GmOpMultiDot{d_w, cols(c0, nc), nc}, bank(p) + (size_t)c0 * MK_MAXP);
            }
            for (int c0 = 0; c0 < ncol; c0 += GM_GROUP) {
                const int nc = ncol - c0 < GM_GROUP ? ncol - c0 : GM_GROUP;
                const bool last = p == 1 && c0 + GM_GROUP >= ncol;
                if (last)
                    launch(GmOpUpdate<true>{bank(p) + (size_t)c0 * MK_MAXP, np_stream, ts.h + c0, p, d_w, cols(c0, nc), nc, {}},
                           ww_part());
                else
                    launch(GmOpUpdate<false>{bank(p) + (size_t)c0 * MK_MAXP, np_stream, ts.h + c0, p, d_w, cols(c0, nc), nc, {}},
                           ww_part());
            }
        }
        hipLaunchKernelGGL(tr_step_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, ww_part(), np_stream, d_scal, ts, d_status,
                           next_halt(), jc, nmv, steps > 0 ? 1 : 0);
        steps += 1;
        launch(TrOpScale{d_scal + S_BETA, d_w, col(jc + 1), 0.0}, rr_part());   // v_{j+1} = (1 / beta_{j+1}) w
    }

    // R: columns 0 .. kk - 1 of V = V[:, :rows] S[:, pick[0 .. kk)]; S is rows x rows, row major.  Runs whatever the halt words
    // say (a breakdown has raised them before the run's last rotation).
    int rotate(int rows, const int *pick, int kk) {
        if (prm.window) return rotate_composed(rows, pick, kk);
        const int groups = (kk + TR_KT - 1) / TR_KT;
        size_t off = 0;
        std::vector<size_t> offs(groups);
        std::vector<int> njs(groups), NJs(groups);
        for (int gI = 0; gI < groups; ++gI) {
            const int j0 = gI * TR_KT, nj = kk - j0 < TR_KT ? kk - j0 : TR_KT;
            const int NJ = nj <= 4 ? 4 : (nj <= 8 ? 8 : TR_KT);
            offs[gI] = off;
            njs[gI] = nj;
            NJs[gI] = NJ;
            for (int c = 0; c < rows; ++c)
                for (int j = 0; j < NJ; ++j) h_Y[off + (size_t)c * NJ + j] = j < nj ? js[(size_t)c * rows + pick[j0 + j]] : 0.0;
            off += (size_t)rows * NJ;
        }
        if (off * sizeof(double) > ybytes) return mk_fail(MK_ERR_STATE, "thick-restart Lanczos: the rotation does not fit its buffer");
        MK_HIP(hipMemcpyAsync(d_Y, h_Y, sizeof(double) * off, hipMemcpyHostToDevice, stream));
        MK_HIP(hipEventRecord(rot0, stream));
        const dim3 grid(mk_grid_stream(n)), block(MK_BLOCK);
        for (int gI = 0; gI < groups; ++gI) {
            // every group but the last goes to the spare columns: the columns it would overwrite are still to be read
            double *W = gI + 1 < groups ? col(m + 1 + gI * TR_KT) : col(gI * TR_KT);
            const double *Y = d_Y + offs[gI];
            if (NJs[gI] == 4) hipLaunchKernelGGL(tr_rotate_kernel<4>, grid, block, 0, stream, d_V, ld, rows, Y, njs[gI], W, n);
            else if (NJs[gI] == 8) hipLaunchKernelGGL(tr_rotate_kernel<8>, grid, block, 0, stream, d_V, ld, rows, Y, njs[gI], W, n);
            else hipLaunchKernelGGL(tr_rotate_kernel<TR_KT>, grid, block, 0, stream, d_V, ld, rows, Y, njs[gI], W, n);
        }
        if (groups > 1)
            MK_HIP(hipMemcpyAsync(col(0), col(m + 1), sizeof(double) * (size_t)(groups - 1) * TR_KT * (size_t)ld,
                                  hipMemcpyDeviceToDevice, stream));
        MK_HIP(hipEventRecord(rot1, stream));
        rotated = true;
        return MK_OK;
    }

    // the same rotation from GmOpCombine launches (GMRES' cycle end): column j = sum_c Y[c, j] v_c, GM_GROUP columns per launch
    int rotate_composed(int rows, const int *pick, int kk) {
        for (int j = 0; j < kk; ++j)
            for (int c = 0; c < rows; ++c) h_Y[(size_t)j * rows + c] = js[(size_t)c * rows + pick[j]];
        MK_HIP(hipMemcpyAsync(d_Y, h_Y, sizeof(double) * (size_t)kk * rows, hipMemcpyHostToDevice, stream));
        MK_HIP(hipEventRecord(rot0, stream));
        for (int j = 0; j < kk; ++j)
            for (int c0 = 0; c0 < rows; c0 += GM_GROUP) {
                const int nc = rows - c0 < GM_GROUP ? rows - c0 : GM_GROUP;
                hipLaunchKernelGGL(mk_stream_kernel<GmOpCombine>, dim3(mk_grid_stream(n)), dim3(MK_BLOCK), 0, stream,
                                   GmOpCombine{d_Y + (size_t)j * rows + c0, col(m + 1 + j), cols(c0, nc), nc, c0 == 0 ? 1 : 0, {}}, n,
                                   MkHalt{d_nohalt, 0, 0}, rr_part());
            }
        MK_HIP(hipMemcpyAsync(col(0), col(m + 1), sizeof(double) * (size_t)kk * (size_t)ld, hipMemcpyDeviceToDevice, stream));
        MK_HIP(hipEventRecord(rot1, stream));
        rotated = true;
        return MK_OK;
    }

    int enqueue_pass() override {
        if (finished) return MK_OK;
        for (int jc = l; jc < m; ++jc) enqueue_step(jc);
        MK_HIP(hipGetLastError());
        MK_HIP(hipMemcpyAsync(h_ab, ts.alpha, sizeof(double) * (size_t)2 * m, hipMemcpyDeviceToHost, stream));
        int rc = poll();                                       // (the one synchronisation of the cycle)
        if (rc != MK_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        if (mk_ctx().pending_rc != MK_OK) return mk_ctx().pending_rc;   // (a host operator callback failed)
        read_rotation_time();
        const int me = (int)h_scal[S_J];                       // columns of this cycle's projected matrix
        breakdown = h_scal[S_BREAK] != 0.0 ? 1 : 0;
        if (me < 1 || me > m || (!breakdown && me != m))
            return mk_fail(MK_ERR_STATE, "thick-restart Lanczos: the device counted %d steps in a cycle of %d", me, m);
        const double *alpha = h_ab, *beta = h_ab + m;
        for (int j = l; j < me; ++j)
            if (!std::isfinite(alpha[j]) || !std::isfinite(beta[j]))
                return mk_fail(MK_ERR_ARG, "thick-restart Lanczos: alpha or beta of step %d of cycle %d is not finite (a matrix or "
                               "start vector with entries that are not finite, or overflow)", j + 1, cycles + 1);
        for (int j = l; j < me; ++j) {
            T[(size_t)j * m + j] = alpha[j];
            if (j + 1 < me) T[(size_t)j * m + j + 1] = T[(size_t)(j + 1) * m + j] = beta[j];
        }
        const double blast = beta[me - 1];
        cycles += 1;
        for (int i = 0; i < me; ++i)
            for (int k = 0; k < me; ++k) ja[(size_t)i * me + k] = T[(size_t)i * m + k];
        sweeps = tr_jacobi(me, ja.data(), js.data(), order.data());
        if (sweeps < 0)
            return mk_fail(MK_ERR_STATE, "thick-restart Lanczos: the Jacobi iteration on the %d x %d projected matrix did not end "
                           "within %d sweeps", me, me, TR_SWEEPS);
        // theta ascending; `order` becomes the wanted order: ascending for the smallest, descending for the largest
        for (int i = 0; i < me; ++i) theta[i] = ja[(size_t)order[i] * me + order[i]];
        std::vector<int> colof(order.begin(), order.begin() + me);          // sorted position -> column of S
        for (int i = 0; i < me; ++i) {
            est[i] = breakdown ? 0.0 : std::fabs(blast * js[(size_t)(me - 1) * me + colof[i]]);
            const double at = std::fabs(theta[i]);
            if (at > anorm) anorm = at;
        }
        const double rel = prm.reltol * anorm;
        threshold = rel > prm.abstol ? rel : prm.abstol;
        const int nret = nev < me ? nev : me;
        // (a filtered run wants B's largest whatever `which` says: rho is positive and monotone on the wanted side)
        const int ord = filt ? 1 : which;
        const auto wanted = [&](int i) { return ord == 0 ? i : me - 1 - i; };   // sorted position of the i-th wanted pair
        resid = 0.0;
        nconv = 0;
        for (int i = 0; i < nret; ++i) {
            const double e = est[wanted(i)];
            if (e > resid) resid = e;
            if (e <= threshold) {
                nconv += 1;
                if (first_met[i] < 0) first_met[i] = cycles;
            }
        }
        hist.push_back(resid);
        hist2.push_back(0.0);
        const auto host_ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        conv = (nret == nev && nconv == nev) ? 1 : 0;
        std::vector<int> pick;
        // the restart: the first `keep` of the wanted order stay
        const auto restart = [&]() -> int {
            for (int i = 0; i < keep; ++i) pick.push_back(colof[wanted(i)]);
            const int rrc = rotate(m, pick.data(), keep);
            if (rrc != MK_OK) return rrc;
            MK_HIP(hipMemcpyAsync(col(keep), col(m), sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
            std::fill(T.begin(), T.end(), 0.0);
            for (int i = 0; i < keep; ++i) {
                T[(size_t)i * m + i] = theta[wanted(i)];
                T[(size_t)i * m + keep] = T[(size_t)keep * m + i] = blast * js[(size_t)(m - 1) * m + pick[i]];
            }
            l = keep;
            return MK_OK;
        };
        if (filt) {
            // B's estimates are a gate only.  The rotation first -- the restart's, whose first nev columns are the wanted Ritz
            // vectors in B's descending order (after a breakdown: those vectors alone) --, then, once the gate has been met and
            // in the last cycle the budget allows, the verification on A; the run goes on from the restart if that fails.
            const bool gate = conv != 0;
            conv = 0;
            if (gate) verifying = true;
            if (breakdown) nmv = h_status->nMatvec;            // (the launches behind the breakdown did nothing)
            const int64_t cost = (int64_t)(m - keep) * fdeg + nev;   // the next cycle and the verification it may need
            int nx = nev;
            if (breakdown) {
                nx = nret;
                for (int i = 0; i < nret; ++i) pick.push_back(colof[wanted(i)]);
                if ((rc = rotate(me, pick.data(), nret)) != MK_OK) return rc;
            } else if ((rc = restart()) != MK_OK) {
                return rc;
            }
            if (breakdown || verifying || nmv + cost > prm.matvec_max) {
                if ((rc = verify(nx)) != MK_OK) return rc;
                resid = 0.0;
                nconv = 0;
                for (int i = 0; i < nx; ++i) {
                    if (!(res_a[i] <= resid)) resid = res_a[i];
                    if (res_a[i] <= thr_a) nconv += 1;
                }
                hist.back() = resid;
                conv = (nx == nev && nconv == nev) ? 1 : 0;
                if (conv || breakdown || nmv + cost > prm.matvec_max) {
                    for (int i = 0; i < nev; ++i) {
                        const bool have = i < nx;
                        h_Y[3 * i] = have ? th_a[perm[i]] : std::nan("");
                        h_Y[3 * i + 1] = have ? res_a[perm[i]] : std::nan("");
                        h_Y[3 * i + 2] = have ? (double)first_met[perm[i]] : -1.0;
                    }
                    MK_HIP(hipMemcpyAsync(d_rec(), h_Y, sizeof(double) * (size_t)3 * nev, hipMemcpyHostToDevice, stream));
                    static const int up[2] = {1, 1};
                    MK_HIP(hipMemcpyAsync(d_halt, up, sizeof(up), hipMemcpyHostToDevice, stream));
                    MK_HIP(hipStreamSynchronize(stream));
                    finished = true;
                }
            }
            hist2.back() = host_ms();
            return MK_OK;
        }
        if (conv || breakdown || nmv + (int64_t)(m - keep) > prm.matvec_max) {
            // the end: X = V S[:, wanted] in ascending order of theta, the record, and the halt words for the driver
            for (int i = 0; i < nret; ++i) pick.push_back(colof[which == 0 ? i : me - nret + i]);
            if ((rc = rotate(me, pick.data(), nret)) != MK_OK) return rc;
            MK_HIP(hipStreamSynchronize(stream));              // (h_Y is reused for the record)
            for (int i = 0; i < nev; ++i) {
                const bool have = i < nret;
                const int pos = which == 0 ? i : me - nret + i;                // sorted position of returned pair i
                const int rank = which == 0 ? i : nret - 1 - i;                // its place in the wanted order
                h_Y[3 * i] = have ? theta[pos] : std::nan("");
                h_Y[3 * i + 1] = have ? est[pos] : std::nan("");
                h_Y[3 * i + 2] = have ? (double)first_met[rank] : -1.0;
            }
            MK_HIP(hipMemcpyAsync(d_rec(), h_Y, sizeof(double) * (size_t)3 * nev, hipMemcpyHostToDevice, stream));
            static const int up[2] = {1, 1};
            MK_HIP(hipMemcpyAsync(d_halt, up, sizeof(up), hipMemcpyHostToDevice, stream));
            MK_HIP(hipStreamSynchronize(stream));
            hist2.back() = host_ms();
            finished = true;
            return MK_OK;
        }
        if ((rc = restart()) != MK_OK) return rc;
        hist2.back() = host_ms();
        return MK_OK;
    }

    // The verification of a filtered run: theta_i = <x_i, A x_i> and ||A x_i - theta_i x_i|| for the kept columns i < nx, by
    // launches that no halt word stops (a breakdown has raised them), then the 2 nx scalars come down; `perm` orders the
    // columns by theta ascending (ties by column).  The residual is formed from A x - theta x itself: <A x, A x> - theta^2
    // cancels at 1e-8 ||A||.
    int verify(int nx) {
        const auto nohalt = [&] { return MkHalt{d_nohalt, 0, 0}; };
        for (int i = 0; i < nx; ++i) {
            mk_spmv_launch_blocks(A, mk_grid_spmv_for(A), stream, col(i), MkPlainEpi{d_w}, MkNoGate(), nohalt, d_part);
            hipLaunchKernelGGL(mk_stream_kernel<MkOpDot<0>>, dim3(mk_grid_stream(n)), dim3(MK_BLOCK), 0, stream,
                               MkOpDot<0>{col(i), d_w}, n, nohalt(), d_vpart);
            hipLaunchKernelGGL(mk_stream_kernel<TrOpResid>, dim3(mk_grid_stream(n)), dim3(MK_BLOCK), 0, stream,
                               TrOpResid{d_vpart, np_stream, col(i), d_w, d_vrec() + 2 * i, 0.0}, n, nohalt(), d_vpart);
            hipLaunchKernelGGL(tr_resid_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, d_vpart + MK_MAXP, np_stream, d_vrec() + 2 * i);
        }
        nmv += nx;
        MK_HIP(hipGetLastError());
        MK_HIP(hipMemcpyAsync(h_ab, d_vrec(), sizeof(double) * (size_t)2 * nx, hipMemcpyDeviceToHost, stream));
        MK_HIP(hipStreamSynchronize(stream));
        if (mk_ctx().pending_rc != MK_OK) return mk_ctx().pending_rc;
        for (int i = 0; i < nx; ++i) {
            th_a[i] = h_ab[2 * i];
            res_a[i] = h_ab[2 * i + 1];
            if (!std::isfinite(th_a[i]) || !std::isfinite(res_a[i]))
                return mk_fail(MK_ERR_ARG, "thick-restart Lanczos: the verification of pair %d on A is not finite (theta = %g, "
                               "residual = %g)", i + 1, th_a[i], res_a[i]);
        }
        for (int i = 0; i < nev; ++i) perm[i] = i;
        std::stable_sort(perm.begin(), perm.begin() + nx, [&](int x, int y) { return th_a[x] < th_a[y]; });
        return MK_OK;
    }

    void read_rotation_time() {                                // (after a synchronisation: the last rotation has finished)
        float ms = 0.f;
        if (rotated && hipEventElapsedTime(&ms, rot0, rot1) == hipSuccess) rot_ms = ms;
        rotated = false;
    }

    int finish(mk_result *res) override {
        int rc = poll();
        if (rc != MK_OK) return rc;
        read_rotation_time();
        fill_result(res);
        res->converged = conv;
        res->residNorm = resid;
        res->residNorm0 = b0;
        res->threshold = threshold;
        res->Anorm = anorm;
        res->aux[0] = (double)cycles;
        res->aux[1] = (double)m;
        res->aux[2] = (double)keep;
        res->aux[3] = (double)basis_bytes;
        res->aux[4] = (double)nconv;
        res->aux[5] = (double)breakdown;
        res->aux[6] = (double)sweeps;
        res->aux[7] = rot_ms;
        if (filt) {                                            // (the host's count: the verification's products are in it)
            res->nMatvec = nmv;
            res->threshold = thr_a;
            res->Anorm = anorm_a;
        }
        return MK_OK;
    }

    // (a filtered run leaves its vectors where the restart rotation put them, in B's descending order: `perm` finds them)
    const double *x() const override { return probe ? d_w : (filt && allocated ? col(perm[0]) : d_V); }
    const double *vector(int i) const override {
        if (filt && i == eig_nev + 1) return d_ftab;
        if (!allocated || i < 0 || i > nev) return nullptr;
        return i < nev ? col(filt ? perm[i] : i) : d_rec();
    }
    int64_t vector_len(int i) const override { return filt && i == eig_nev + 1 ? ntab : (i == nev ? 3 * (int64_t)nev : n); }
};

}  // namespace

mk_solver *mk_make_trlan() { return new TrlanSolver(); }
