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

// E: the end of the step on column jc (0-based), whose product was the run's product number nmv
__global__ __launch_bounds__(MK_BLOCK) void tr_step_kernel(const double *ww_part, int np, double *scal, TrScal ts, MkStatus *st,
                                                           MkHalt halt, int jc, int64_t nmv) {
    __shared__ double s4[4];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double beta = __dsqrt_rn(mk_total(ww_part, np, s4));
    if (threadIdx.x == 0) {
        const double alpha = ts.h[jc];
        double tm = fabs(alpha);
        if (nmv > 1) tm = tm + scal[S_BETA];                   // (beta_j: of the step before, in this cycle or the last one)
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

    ~TrlanSolver() override {
        if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
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
        if (prm.matvec_max < (int64_t)eig_ncv)
            return mk_fail(MK_ERR_ARG, "mk_solver_setup: thick-restart Lanczos matvec_max = %lld is below ncv = %d: the first cycle "
                           "does not fit", (long long)prm.matvec_max, eig_ncv);
        int rc;
        if (!allocated && (rc = allocate()) != MK_OK) return rc;
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
        mk_launch_spmv(this, col(jc), MkPlainEpi{d_w});
        nmv += 1;
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
                           next_halt(), jc, nmv);
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
        const auto wanted = [&](int i) { return which == 0 ? i : me - 1 - i; };   // sorted position of the i-th wanted pair
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
        // the restart: the first `keep` of the wanted order stay
        for (int i = 0; i < keep; ++i) pick.push_back(colof[wanted(i)]);
        if ((rc = rotate(m, pick.data(), keep)) != MK_OK) return rc;
        MK_HIP(hipMemcpyAsync(col(keep), col(m), sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
        std::fill(T.begin(), T.end(), 0.0);
        for (int i = 0; i < keep; ++i) {
            T[(size_t)i * m + i] = theta[wanted(i)];
            T[(size_t)i * m + keep] = T[(size_t)keep * m + i] = blast * js[(size_t)(m - 1) * m + pick[i]];
        }
        l = keep;
        hist2.back() = host_ms();
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
        return MK_OK;
    }

    const double *x() const override { return d_V; }
    const double *vector(int i) const override {
        if (!allocated || i < 0 || i > nev) return nullptr;
        return i < nev ? col(i) : d_rec();
    }
    int64_t vector_len(int i) const override { return i == nev ? 3 * (int64_t)nev : n; }
};

}  // namespace

mk_solver *mk_make_trlan() { return new TrlanSolver(); }
