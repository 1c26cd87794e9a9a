// mk_trsvd.hip -- thick-restart Golub-Kahan-Lanczos bidiagonalisation (Baglama and Reichel 2005; SLEPc's TRLBD) for a few
// extreme singular triplets of a tall device operator, device resident (solver kind MK_TRSVD; no reference module,
// DESIGN.md 3.17).  The NumPy restatement is tests/_trsvd_ref.py.
//
// A is R x C with R >= C; A' is the device matrix of mk_solver_set_transpose.  One pass of the driver = one whole cycle.
// U = [u_1 .. u_m, spare columns] (length R) and V = [v_1 .. v_m, v_{m+1}, spare columns] (length C) are one allocation
// each (m = ncv); B is the m x m upper triangular projected matrix, kept on the host.  Step j (1-based) of a cycle that
// starts behind l kept triplets, j = l + 1 .. m:
//   PA  u = A v_j, written into its column of U                                              [product, in A's format]
//       reorth = 1 (both bases): D, U, D, U of mk_multicol.h against u_1 .. u_{j-1}, the last U accumulating <u, u>
//                                (j = 1: one MkOpDot launch instead)                         [4 ceil((j-1) / GM_GROUP) launches]
//       reorth = 0 (V only):     the product's row epilogue SvEpiU subtracts B[j-1, j] u_{j-1} and accumulates <u, u> on
//                                the way out (j = 1: nothing to subtract); j = l + 1 behind a restart: a plain product,
//                                then the arrow u -= sum_i B[i, l+1] u_i by GmOpUpdateGiven, GM_GROUP columns per launch,
//                                the last one accumulating <u, u>                            [0, or ceil(l / GM_GROUP) launches]
//   EA  one workgroup, one lane writes: alpha_j = sqrt<u, u>, the running scale, the counts, and the breakdown test
//       alpha_j not > 2^-26 smax, which raises the halt words: the rest of the cycle does nothing
//   SA  u_j = (1 / alpha_j) u, in place                                                      [stream]
//   PT  w = A' u_j, written into column j + 1 of V                                           [product, in A''s format]
//       D, U, D, U against v_1 .. v_j (always), the last U accumulating <w, w>              [4 ceil(j / GM_GROUP) launches]
//   EB  as EA for beta_j = sqrt<w, w> (B[j, j+1] for j < m)
//   SB  v_{j+1} = (1 / beta_j) w, in place                                                   [stream]
// smax is the largest alpha or beta accepted so far in the run (0 before the first step: alpha_1 must be positive).
// The cycle ends on the host: one download of alpha, beta and the status, B[:me, :me] = X diag(s) Y' by a one-sided
// (Hestenes) Jacobi iteration (sv_jacobi below), the estimates |beta_m X[me, i]|, the stop tests, one upload of the rotation
// coefficients, and TRLAN's rotation kernel (mk_rotate.h) on U with X and on V with Y: at a restart the `keep` wanted
// triplets move to the front, v_{keep+1} = v_{m+1}, B = diag(s_kept) with the arrow beta_m X[m, kept_i] in column keep + 1;
// at the end of the run U X[:, wanted] and V Y[:, wanted].
//
// Launches per step: reorth = 1: 2 + 4 ceil((j-1) / G) + 4 ceil(j / G) + 4; reorth = 0: 2 + 4 ceil(j / G) + 4.
// Bytes per step beyond the two plain products: V side 2 (16 j + 24 ceil(j / G)) C + 16 C; U side, reorth = 1:
// 2 (16 (j-1) + 24 ceil((j-1) / G)) R + 16 R; reorth = 0: 8 R more in the product (u_{j-1}) + 16 R, and in the first step
// behind a restart (8 l + 16 ceil(l / G)) R for the arrow.
// Every operation rounds on its own (-ffp-contract=off); every dot but SvEpiU's has the lanes, the grid and the tree of
// mk_stream_kernel<MkOpDot>, then mk_total; SvEpiU's has the row order of A's product kernel (like EpiU of mk_lls.hip).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "mk_multicol.h"
#include "mk_rotate.h"
#include "mk_solver.h"

namespace {

constexpr int SV_KT = 16;                                    // output columns per rotation launch (TR_KT of mk_trlan.hip)
constexpr int SV_SWEEPS = 40;                                // sweeps after which sv_jacobi gives up
constexpr double SV_SKIP = 0x1.0p-6;                         // a pair with d + SV_SKIP |c| == d is orthogonal enough

// the shared scalar file (poll() brings it to the host)
enum { S_B0 = 0, S_VAL = 1, S_SMAX = 2, S_J = 3, S_BREAK = 4 };
enum { SV_BREAK_NONE = 0, SV_BREAK_BETA = 1, SV_BREAK_ALPHA = 2, SV_BREAK_START = 3 };

// the cycle's own scalar file: alpha_j and beta_j by step (one download per cycle), the coefficients of the two
// orthogonalisations, and the arrow the host uploads at a restart
struct SvScal {
    double *alpha, *beta, *hv, *hu, *arrow;
};

struct SvOpStart {              // out = start (or the hashed vector) ; partial <out, out>
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

struct SvOpScale {              // SA, SB: x = (1 / *d) x, in place
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *d;
    double *x;
    double s;
    __device__ bool prologue(double *, bool) {
        s = 1.0 / d[0];
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 v = mk_ld2(x, i);
        v.x = s * v.x;
        v.y = s * v.y;
        mk_st2(x, i, v);
    }
    __device__ void one(int64_t i, double *) { x[i] = s * x[i]; }
};

// PA of the one-sided mode: u_j[i] = (A v_j)[i] - beta u_{j-1}[i] with the partial <u_j, u_j>; beta = B[j-1, j] is read
// from the device.  `prev` null (the first step of a run): nothing to subtract, the norm is still wanted.
struct SvEpiU {
    static constexpr int NACC = 1, SLOT0 = 0;
    static constexpr bool NO_MARCH = true;         // (rectangular operators: mk_device.h MkNoMarch)
    const double *coef;
    const double *prev;
    double *u;
    double beta;
    int nt;              // u goes past the caches (vectors beyond the Infinity Cache; mk_store_stream, mk_solver.h)
    __device__ void prologue(double *) { beta = prev ? coef[0] : 0.0; }
    __device__ double xin(double x) const { return x; }
    __device__ void row(int64_t i, double sum, double *acc) {
        const double t = prev ? sum - beta * prev[i] : sum;
        mk_store_stream(u + i, t, nt);
        acc[0] += t * t;
    }
};

struct SvEpiPlain {             // y = M x, nothing fused (PT, and PA where the orthogonalisation follows in stream launches)
    static constexpr int NACC = 0, SLOT0 = 0;
    static constexpr bool NO_MARCH = true;         // (rectangular operators: mk_device.h MkNoMarch)
    double *y;
    int nt;
    __device__ void prologue(double *) {}
    __device__ double xin(double x) const { return x; }
    __device__ void row(int64_t i, double sum, double *) { mk_store_stream(y + i, sum, nt); }
};

// ||start|| and the test on it: a start vector without a positive, finite norm halts the run before its first step
__global__ __launch_bounds__(MK_BLOCK) void sv_start_kernel(const double *rr_part, int np, double *scal, MkHalt halt) {
    __shared__ double s4[4];
    const double b0 = __dsqrt_rn(mk_total(rr_part, np, s4));
    if (threadIdx.x == 0) {
        const bool bad = !(isfinite(b0) && b0 > 0.0);
        scal[S_B0] = b0;
        scal[S_VAL] = b0;
        if (bad) scal[S_BREAK] = (double)SV_BREAK_START;
        halt.out(bad);
    }
}

// EA (`is_alpha`) and EB: the end of half a step on column jc (0-based); `nmv` counts the run's products so far
__global__ __launch_bounds__(MK_BLOCK) void sv_step_kernel(const double *part, int np, double *scal, double *dst, MkStatus *st,
                                                           MkHalt halt, int jc, int64_t nmv, int is_alpha) {
    __shared__ double s4[4];
    if (halt.in()) {
        if (threadIdx.x == 0) halt.out(true);
        return;
    }
    const double val = __dsqrt_rn(mk_total(part, np, s4));
    if (threadIdx.x == 0) {
        const double s0 = scal[S_SMAX];
        const bool stop = !(val > 0x1.0p-26 * s0);
        *dst = val;
        scal[S_VAL] = val;
        if (!stop) scal[S_SMAX] = val > s0 ? val : s0;
        if (is_alpha) {
            scal[S_J] = (double)(jc + 1);
            st->itn += 1;
        }
        if (stop) scal[S_BREAK] = (double)(is_alpha ? SV_BREAK_ALPHA : SV_BREAK_BETA);
        st->nMatvec = nmv;
        halt.out(stop);
    }
}

// The small SVD: one-sided (Hestenes) Jacobi on the m x m matrix `g` (row major; a copy of B), row-cyclic pairs (p, q),
// p < q, of COLUMNS.  With a = <g_p, g_p>, b = <g_q, g_q>, c = <g_p, g_q> (row index ascending) a pair is skipped when
// c == 0, when sqrt(a) + sqrt(b) equals one of the two (a column that is negligible against the other: what is left of a
// zero singular value, whose inner products are noise) or when d + SV_SKIP |c| == d for d = sqrt(a) sqrt(b) -- exact float64
// comparisons, no tolerance.  Otherwise zeta = (b - a) / (2 c), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)),
// cs = 1 / sqrt(1 + t^2), sn = cs t, and the columns p, q of g and of y become cs g_p - sn g_q and sn g_p + cs g_q.  Ends
// after a sweep without rotations: s = the column norms, x = the normalised columns, B = x diag(s) y'.  A column whose norm
// has s_max + s == s_max is a zero singular value to working precision: s = 0 and its column of x is zero, so nothing is
// NaN.  `order`: the columns by descending s, ties by index.  Returns the sweeps, or -1 after SV_SWEEPS sweeps that all
// rotated.  B'B is never formed: its eigenvalues would lose the small singular values.  Restated operation by operation
// in tests/_trsvd_ref.py (jacobi_svd).
static int sv_jacobi(int m, double *g, double *y, double *s, double *x, int *order) {
    for (int i = 0; i < m; ++i)
        for (int k = 0; k < m; ++k) y[(size_t)i * m + k] = i == k ? 1.0 : 0.0;
    for (int sweep = 1; sweep <= SV_SWEEPS; ++sweep) {
        int rotations = 0;
        for (int p = 0; p < m - 1; ++p) {
            for (int q = p + 1; q < m; ++q) {
                double a = 0.0, b = 0.0, c = 0.0;
                for (int k = 0; k < m; ++k) {
                    const double gp = g[(size_t)k * m + p], gq = g[(size_t)k * m + q];
                    a = a + gp * gp;
                    b = b + gq * gq;
                    c = c + gp * gq;
                }
                if (c == 0.0) continue;
                const double sa = std::sqrt(a), sb = std::sqrt(b);
                if (sa + sb == sa || sa + sb == sb) continue;
                const double d = sa * sb;
                if (d + SV_SKIP * std::fabs(c) == d) continue;
                const double zeta = (b - a) / (2.0 * c);
                double t = 1.0 / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                if (zeta < 0.0) t = -t;
                const double cs = 1.0 / std::sqrt(1.0 + t * t);
                const double sn = cs * t;
                for (int k = 0; k < m; ++k) {
                    const double gp = g[(size_t)k * m + p], gq = g[(size_t)k * m + q];
                    g[(size_t)k * m + p] = cs * gp - sn * gq;
                    g[(size_t)k * m + q] = sn * gp + cs * gq;
                    const double yp = y[(size_t)k * m + p], yq = y[(size_t)k * m + q];
                    y[(size_t)k * m + p] = cs * yp - sn * yq;
                    y[(size_t)k * m + q] = sn * yp + cs * yq;
                }
                rotations += 1;
            }
        }
        if (rotations == 0) {
            double top = 0.0;
            for (int i = 0; i < m; ++i) {
                double a = 0.0;
                for (int k = 0; k < m; ++k) a = a + g[(size_t)k * m + i] * g[(size_t)k * m + i];
                s[i] = std::sqrt(a);
                if (s[i] > top) top = s[i];
            }
            for (int i = 0; i < m; ++i) {
                const bool zero = top + s[i] == top;
                if (zero) s[i] = 0.0;
                for (int k = 0; k < m; ++k) x[(size_t)k * m + i] = zero ? 0.0 : g[(size_t)k * m + i] / s[i];
            }
            for (int i = 0; i < m; ++i) order[i] = i;
            std::stable_sort(order, order + m, [&](int i, int k) { return s[i] > s[k]; });
            return sweep;
        }
    }
    return -1;
}

struct Basis {                       // columns of `len` entries, `ld` apart, `cols` of them before the spare ones
    double *d = nullptr;
    int64_t len = 0, ld = 0;
    int cols = 0, np = 1;
    size_t bytes = 0;
    double *col(int k) const { return d + (size_t)k * (size_t)ld; }
};

struct TrsvdSolver : mk_solver {
    Basis U, V;
    double *d_tscal = nullptr;       // SvScal's storage, then the record of 3 nsv doubles
    double *d_tpart = nullptr;       // two banks of `nslot` coefficient slots, then <u, u> / <w, w> and <start, start>
    double *d_Y = nullptr;           // the rotation coefficients: U's half, then V's
    double *h_ab = nullptr, *h_Y = nullptr, *h_rec = nullptr;   // pinned: alpha and beta of a cycle; coefficients, arrow and record on their way up
    hipEvent_t rot0 = nullptr, rot1 = nullptr;
    SvScal ts{};
    int m = 0, nsv = 0, keep = 0, which = 0, full = 1, nslot = 0, spare = 0, np_A = 1;
    size_t yhalf = 0;                // doubles per half of d_Y / h_Y
    bool allocated = false;
    // the run's host state
    std::vector<double> B, G, Xs, Ys, sv, est;
    std::vector<int> order, first_met;
    int l = 0, cycles = 0, sweeps = 0, nconv = 0, breakdown = 0, conv = 0, nret = 0;
    bool finished = false, rotated = false;
    int64_t nmv = 0;
    double anorm = 0.0, threshold = 0.0, resid = 0.0, b0 = 0.0, rot_ms = 0.0;

    ~TrsvdSolver() override {
        if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
        hipFree(U.d);
        hipFree(V.d);
        hipFree(d_tscal);
        hipFree(d_tpart);
        hipFree(d_Y);
        if (h_ab) hipHostFree(h_ab);
        if (h_Y) hipHostFree(h_Y);
        if (h_rec) hipHostFree(h_rec);
        if (rot0) hipEventDestroy(rot0);
        if (rot1) hipEventDestroy(rot1);
    }

    double *bank(int b) const { return d_tpart + (size_t)b * nslot * MK_MAXP; }
    double *ww_part() const { return d_tpart + (size_t)2 * nslot * MK_MAXP; }
    double *rr_part() const { return ww_part() + MK_MAXP; }
    double *d_rec() const { return d_tscal + (size_t)5 * nslot; }

    template <class Op>
    void launch(const Op &op, int64_t len, double *partials) {
        hipLaunchKernelGGL(mk_stream_kernel<Op>, dim3(mk_grid_stream(len)), dim3(MK_BLOCK), 0, stream, op, len, next_halt(), partials);
    }

    static GmCols cols(const Basis &W, int c0, int nc) {
        GmCols v;
        for (int c = 0; c < GM_GROUP; ++c) v.col[c] = W.col(c0 + (c < nc ? c : 0));
        return v;
    }

    int alloc_basis(Basis &W, int64_t len, int ncols, const char *name) {
        W.len = len;
        W.cols = ncols;
        W.np = mk_grid_stream(len);
        W.ld = ((len + 1) & ~(int64_t)1) + 2;   // rounded up to even, and the 16 bytes of zeroed slack a product's input needs
        W.bytes = sizeof(double) * (size_t)(ncols + spare) * (size_t)W.ld;
        if (hipMalloc((void **)&W.d, W.bytes) != hipSuccess) {
            (void)hipGetLastError();
            W.d = nullptr;
            return mk_fail(MK_ERR_HIP, "thick-restart SVD: out of device memory for the basis %s: %d + %d columns of %lld rows "
                           "need %zu bytes; a smaller ncv needs less", name, ncols, spare, (long long)len, W.bytes);
        }
        MK_HIP(hipMemsetAsync(W.d, 0, W.bytes, stream));
        return MK_OK;
    }

    int allocate() {
        m = eig_ncv;
        nsv = eig_nev;
        keep = eig_keep;
        which = eig_which;
        full = prm.reorth;
        nslot = (m + GM_GROUP - 1) / GM_GROUP * GM_GROUP;
        spare = SV_KT * ((keep + SV_KT - 1) / SV_KT - 1);
        if (U.d || V.d) return mk_fail(MK_ERR_STATE, "thick-restart SVD: an earlier set-up of this solver ran out of device memory");
        int rc;
        if ((rc = alloc_basis(U, A->nrows, m, "U")) != MK_OK) return rc;
        if ((rc = alloc_basis(V, A->ncols, m + 1, "V")) != MK_OK) return rc;
        const size_t sbytes = sizeof(double) * ((size_t)5 * nslot + (size_t)3 * nsv);
        MK_HIP(hipMalloc((void **)&d_tscal, sbytes));
        ts.alpha = d_tscal;
        ts.beta = d_tscal + nslot;
        ts.hv = d_tscal + 2 * nslot;
        ts.hu = d_tscal + 3 * nslot;
        ts.arrow = d_tscal + 4 * nslot;
        const size_t pbytes = sizeof(double) * ((size_t)2 * nslot + 2) * MK_MAXP;
        MK_HIP(hipMalloc((void **)&d_tpart, pbytes));
        MK_HIP(hipMemsetAsync(d_tpart, 0, pbytes, stream));
        // a rotation's coefficients: at most ceil(keep / SV_KT) groups of m x SV_KT, once for U and once for V
        yhalf = (size_t)m * (size_t)(spare + SV_KT);
        MK_HIP(hipMalloc((void **)&d_Y, sizeof(double) * 2 * yhalf));
        MK_HIP(hipHostMalloc((void **)&h_Y, sizeof(double) * 2 * yhalf, hipHostMallocDefault));
        MK_HIP(hipHostMalloc((void **)&h_ab, sizeof(double) * (size_t)2 * nslot, hipHostMallocDefault));
        MK_HIP(hipHostMalloc((void **)&h_rec, sizeof(double) * ((size_t)3 * nsv + (size_t)nslot), hipHostMallocDefault));
        MK_HIP(hipEventCreate(&rot0));
        MK_HIP(hipEventCreate(&rot1));
        np_A = mk_grid_spmv_for(A);
        allocated = true;
        return MK_OK;
    }

    int end_run() {                  // the record, and the halt words for the driver
        for (int i = 0; i < nsv; ++i) {
            const bool have = i < nret;
            // returned triplet i, in descending order of s: its column of the small problem and its place in the wanted order
            const int pos = which == 1 ? i : (int)order.size() - nret + i;
            const int rank = which == 1 ? i : nret - 1 - i;
            h_rec[3 * i] = have ? sv[order[(size_t)pos]] : -1.0;
            h_rec[3 * i + 1] = have ? est[pos] : 0.0;
            h_rec[3 * i + 2] = have ? (double)first_met[rank] : -1.0;
        }
        MK_HIP(hipMemcpyAsync(d_rec(), h_rec, sizeof(double) * (size_t)3 * nsv, hipMemcpyHostToDevice, stream));
        static const int up[2] = {1, 1};
        MK_HIP(hipMemcpyAsync(d_halt, up, sizeof(up), hipMemcpyHostToDevice, stream));
        MK_HIP(hipStreamSynchronize(stream));
        finished = true;
        return MK_OK;
    }

    int setup(const double *start, const double *guess) override {
        if (guess)
            return mk_fail(MK_ERR_ARG, "mk_solver_setup: the thick-restart SVD takes a start vector and no initial guess");
        if (!At) return mk_fail(MK_ERR_STATE, "thick-restart SVD: call mk_solver_set_transpose first");
        if (At->ex.mode >= 0 || At->row_block)
            return mk_fail(MK_ERR_UNSUPPORTED, "thick-restart SVD: the transposed operator is row-partitioned (it carries an "
                           "exchange plan or a row block); the solver is single-GPU");
        int rc;
        if (!allocated && (rc = allocate()) != MK_OK) return rc;
        MK_HIP(hipMemsetAsync(d_tscal, 0, sizeof(double) * ((size_t)5 * nslot + (size_t)3 * nsv), stream));
        B.assign((size_t)m * m, 0.0);
        G.assign((size_t)m * m, 0.0);
        Xs.assign((size_t)m * m, 0.0);
        Ys.assign((size_t)m * m, 0.0);
        sv.assign(m, 0.0);
        est.assign(m, 0.0);
        order.clear();
        first_met.assign(nsv, -1);
        l = cycles = sweeps = nconv = breakdown = conv = nret = 0;
        finished = rotated = false;
        nmv = 0;
        anorm = threshold = resid = rot_ms = 0.0;
        launch(SvOpStart{start, V.col(0), eig_seed}, V.len, rr_part());
        hipLaunchKernelGGL(sv_start_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, rr_part(), V.np, d_scal, next_halt());
        launch(SvOpScale{d_scal + S_B0, V.col(0), 0.0}, V.len, rr_part());      // v_1 = (1 / ||start||) start
        MK_HIP(hipMemcpyAsync(h_ab, d_scal + S_B0, sizeof(double), hipMemcpyDeviceToHost, stream));
        MK_HIP(hipStreamSynchronize(stream));
        b0 = h_ab[0];
        if (!(std::isfinite(b0) && b0 > 0.0)) {               // halted before the first step: no triplet, nothing NaN
            breakdown = SV_BREAK_START;
            return end_run();
        }
        if (2 * (int64_t)m > prm.matvec_max) return end_run();  // the first cycle does not fit: it is not started
        return MK_OK;
    }

    void orthogonalise(const Basis &W, double *w, int ncol, double *h) {      // D, U, D, U; the last U accumulates <w, w>
        for (int p = 0; p < 2; ++p) {
            for (int c0 = 0; c0 < ncol; c0 += GM_GROUP) {
                const int nc = ncol - c0 < GM_GROUP ? ncol - c0 : GM_GROUP;
                launch(GmOpMultiDot{w, cols(W, c0, nc), nc}, W.len, bank(p) + (size_t)c0 * MK_MAXP);
            }
            for (int c0 = 0; c0 < ncol; c0 += GM_GROUP) {
                const int nc = ncol - c0 < GM_GROUP ? ncol - c0 : GM_GROUP;
                const bool last = p == 1 && c0 + GM_GROUP >= ncol;
                if (last)
                    launch(GmOpUpdate<true>{bank(p) + (size_t)c0 * MK_MAXP, W.np, h + c0, p, w, cols(W, c0, nc), nc, {}}, W.len,
                           ww_part());
                else
                    launch(GmOpUpdate<false>{bank(p) + (size_t)c0 * MK_MAXP, W.np, h + c0, p, w, cols(W, c0, nc), nc, {}}, W.len,
                           ww_part());
            }
        }
    }

    template <class Epi>
    void product(const mk_csr *M, const double *x, const Epi &epi, double *partials) {
        mk_spmv_launch_blocks(M, mk_grid_spmv_for(M), stream, x, epi, MkNoGate(), [&] { return next_halt(); }, partials);
    }

    void enqueue_step(int jc) {
        double *u = U.col(jc), *w = V.col(jc + 1);
        int np_uu = U.np;
        nmv += 1;
        if (full) {
            product(A, V.col(jc), SvEpiPlain{u, mk_store_nt(A)}, ww_part());
            if (jc > 0) orthogonalise(U, u, jc, ts.hu);
            else launch(MkOpDot<0>{u, u}, U.len, ww_part());
        } else if (jc == l && l > 0) {                         // the arrow: u -= sum_i B[i, l] u_i
            product(A, V.col(jc), SvEpiPlain{u, mk_store_nt(A)}, ww_part());
            for (int c0 = 0; c0 < l; c0 += GM_GROUP) {
                const int nc = l - c0 < GM_GROUP ? l - c0 : GM_GROUP;
                if (c0 + GM_GROUP >= l)
                    launch(GmOpUpdateGiven<true>{ts.arrow + c0, u, cols(U, c0, nc), nc, {}}, U.len, ww_part());
                else
                    launch(GmOpUpdateGiven<false>{ts.arrow + c0, u, cols(U, c0, nc), nc, {}}, U.len, ww_part());
            }
        } else {
            product(A, V.col(jc), SvEpiU{jc > 0 ? ts.beta + (jc - 1) : nullptr, jc > 0 ? U.col(jc - 1) : nullptr, u, 0.0, mk_store_nt(A)},
                    ww_part());
            np_uu = np_A;
        }
        hipLaunchKernelGGL(sv_step_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, ww_part(), np_uu, d_scal, ts.alpha + jc, d_status,
                           next_halt(), jc, nmv, 1);
        launch(SvOpScale{d_scal + S_VAL, u, 0.0}, U.len, rr_part());            // u_j = (1 / alpha_j) u
        nmv += 1;
        product(At, u, SvEpiPlain{w, mk_store_nt(At)}, ww_part());
        orthogonalise(V, w, jc + 1, ts.hv);
        hipLaunchKernelGGL(sv_step_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, ww_part(), V.np, d_scal, ts.beta + jc, d_status,
                           next_halt(), jc, nmv, 0);
        launch(SvOpScale{d_scal + S_VAL, w, 0.0}, V.len, rr_part());            // v_{j+1} = (1 / beta_j) w
    }

    // R: columns 0 .. kk - 1 of W = W[:, :rows] S[:, pick[0 .. kk)]; S is rows x rows, row major; `half` selects the part of
    // the coefficient buffers (U's rotation and V's are enqueued back to back).  Runs whatever the halt words say.
    int rotate(const Basis &W, int half, const double *S, int rows, const int *pick, int kk) {
        const int groups = (kk + SV_KT - 1) / SV_KT;
        double *hy = h_Y + (size_t)half * yhalf, *dy = d_Y + (size_t)half * yhalf;
        size_t off = 0;
        std::vector<size_t> offs(groups);
        std::vector<int> njs(groups), NJs(groups);
        for (int gI = 0; gI < groups; ++gI) {
            const int j0 = gI * SV_KT, nj = kk - j0 < SV_KT ? kk - j0 : SV_KT;
            const int NJ = nj <= 4 ? 4 : (nj <= 8 ? 8 : SV_KT);
            if ((off + (size_t)rows * NJ) > yhalf) return mk_fail(MK_ERR_STATE, "thick-restart SVD: the rotation does not fit its buffer");
            offs[gI] = off;
            njs[gI] = nj;
            NJs[gI] = NJ;
            for (int c = 0; c < rows; ++c)
                for (int j = 0; j < NJ; ++j) hy[off + (size_t)c * NJ + j] = j < nj ? S[(size_t)c * rows + pick[j0 + j]] : 0.0;
            off += (size_t)rows * NJ;
        }
        MK_HIP(hipMemcpyAsync(dy, hy, sizeof(double) * off, hipMemcpyHostToDevice, stream));
        const dim3 grid(mk_grid_stream(W.len)), block(MK_BLOCK);
        for (int gI = 0; gI < groups; ++gI) {
            // every group but the last goes to the spare columns: the columns it would overwrite are still to be read
            double *out = gI + 1 < groups ? W.col(W.cols + gI * SV_KT) : W.col(gI * SV_KT);
            const double *Y = dy + offs[gI];
            if (NJs[gI] == 4) hipLaunchKernelGGL(tr_rotate_kernel<4>, grid, block, 0, stream, W.d, W.ld, rows, Y, njs[gI], out, W.len);
            else if (NJs[gI] == 8) hipLaunchKernelGGL(tr_rotate_kernel<8>, grid, block, 0, stream, W.d, W.ld, rows, Y, njs[gI], out, W.len);
            else hipLaunchKernelGGL(tr_rotate_kernel<SV_KT>, grid, block, 0, stream, W.d, W.ld, rows, Y, njs[gI], out, W.len);
        }
        if (groups > 1)
            MK_HIP(hipMemcpyAsync(W.col(0), W.col(W.cols), sizeof(double) * (size_t)(groups - 1) * SV_KT * (size_t)W.ld,
                                  hipMemcpyDeviceToDevice, stream));
        return MK_OK;
    }

    // (called after the cycle's synchronisation: the coefficient buffers of the last rotation are free again)
    int rotate_both(int rows, const int *pick, int kk) {
        MK_HIP(hipEventRecord(rot0, stream));
        int rc;
        if ((rc = rotate(U, 0, Xs.data(), rows, pick, kk)) != MK_OK) return rc;
        if ((rc = rotate(V, 1, Ys.data(), rows, pick, kk)) != MK_OK) return rc;
        MK_HIP(hipEventRecord(rot1, stream));
        rotated = true;
        return MK_OK;
    }

    int enqueue_pass() override {
        if (finished) return MK_OK;
        for (int jc = l; jc < m; ++jc) enqueue_step(jc);
        MK_HIP(hipGetLastError());
        MK_HIP(hipMemcpyAsync(h_ab, ts.alpha, sizeof(double) * (size_t)2 * nslot, hipMemcpyDeviceToHost, stream));
        int rc = poll();                                       // (the one synchronisation of the cycle)
        if (rc != MK_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        if (mk_ctx().pending_rc != MK_OK) return mk_ctx().pending_rc;   // (a host operator callback failed)
        read_rotation_time();
        const int me = (int)h_scal[S_J];                       // columns of this cycle's projected matrix
        breakdown = (int)h_scal[S_BREAK];
        if (me < 1 || me > m || (!breakdown && me != m))
            return mk_fail(MK_ERR_STATE, "thick-restart SVD: the device counted %d steps in a cycle of %d", me, m);
        const double *alpha = h_ab, *beta = h_ab + nslot;
        for (int j = l; j < me; ++j)
            if (!std::isfinite(alpha[j]) || (!std::isfinite(beta[j]) && !(breakdown == SV_BREAK_ALPHA && j == me - 1)))
                return mk_fail(MK_ERR_ARG, "thick-restart SVD: alpha or beta of step %d of cycle %d is not finite (a matrix or "
                               "start vector with entries that are not finite, or overflow)", j + 1, cycles + 1);
        for (int j = l; j < me; ++j) {
            B[(size_t)j * m + j] = alpha[j];
            if (j + 1 < me) B[(size_t)j * m + j + 1] = beta[j];
        }
        if (breakdown == SV_BREAK_ALPHA) {                     // A v_me lies in the span of U: alpha = 0, u = 0
            B[(size_t)(me - 1) * m + me - 1] = 0.0;
            MK_HIP(hipMemsetAsync(U.col(me - 1), 0, sizeof(double) * (size_t)U.len, stream));
        }
        const double blast = beta[me - 1];
        cycles += 1;
        for (int i = 0; i < me; ++i)
            for (int k = 0; k < me; ++k) G[(size_t)i * me + k] = B[(size_t)i * m + k];
        order.assign(me, 0);
        sweeps = sv_jacobi(me, G.data(), Ys.data(), sv.data(), Xs.data(), order.data());
        if (sweeps < 0)
            return mk_fail(MK_ERR_STATE, "thick-restart SVD: the Jacobi iteration on the %d x %d projected matrix did not end "
                           "within %d sweeps", me, me, SV_SWEEPS);
        // `order`: the columns of X and Y by descending s; est by sorted position
        for (int i = 0; i < me; ++i) est[i] = breakdown ? 0.0 : std::fabs(blast * Xs[(size_t)(me - 1) * me + order[i]]);
        if (sv[order[0]] > anorm) anorm = sv[order[0]];
        const double rel = prm.reltol * anorm;
        threshold = rel > prm.abstol ? rel : prm.abstol;
        nret = nsv < me ? nsv : me;
        const auto wanted = [&](int i) { return which == 1 ? i : me - 1 - i; };   // sorted position of the i-th wanted triplet
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
        conv = (nret == nsv && nconv == nsv) ? 1 : 0;
        std::vector<int> pick;
        if (conv || breakdown || nmv + 2 * (int64_t)(m - keep) > prm.matvec_max) {
            // the end: U X[:, wanted] and V Y[:, wanted] in descending order of s
            for (int i = 0; i < nret; ++i) pick.push_back(order[which == 1 ? i : me - nret + i]);
            if ((rc = rotate_both(me, pick.data(), nret)) != MK_OK) return rc;
            if ((rc = end_run()) != MK_OK) return rc;
            hist2.back() = host_ms();
            return MK_OK;
        }
        // the restart: the first `keep` of the wanted order stay
        for (int i = 0; i < keep; ++i) pick.push_back(order[wanted(i)]);
        if ((rc = rotate_both(m, pick.data(), keep)) != MK_OK) return rc;
        MK_HIP(hipMemcpyAsync(V.col(keep), V.col(m), sizeof(double) * (size_t)V.len, hipMemcpyDeviceToDevice, stream));
        std::fill(B.begin(), B.end(), 0.0);
        double *h_arrow = h_rec + (size_t)3 * nsv;
        for (int i = 0; i < keep; ++i) {
            B[(size_t)i * m + i] = sv[pick[i]];
            h_arrow[i] = B[(size_t)i * m + keep] = blast * Xs[(size_t)(m - 1) * m + pick[i]];
        }
        MK_HIP(hipMemcpyAsync(ts.arrow, h_arrow, sizeof(double) * (size_t)keep, hipMemcpyHostToDevice, stream));
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
        res->istop = sweeps;
        res->residNorm = resid;
        res->residNorm0 = b0;
        res->threshold = threshold;
        res->Anorm = anorm;
        res->aux[0] = (double)cycles;
        res->aux[1] = (double)m;
        res->aux[2] = (double)keep;
        res->aux[3] = (double)(U.bytes + V.bytes);
        res->aux[4] = (double)nconv;
        res->aux[5] = (double)breakdown;
        res->aux[6] = (double)full;
        res->aux[7] = rot_ms;
        return MK_OK;
    }

    const double *x() const override { return V.d; }
    const double *vector(int i) const override {
        if (!allocated || i < 0 || i > 2 * nsv) return nullptr;
        return i < nsv ? V.col(i) : (i < 2 * nsv ? U.col(i - nsv) : d_rec());
    }
    int64_t vector_len(int i) const override { return i < nsv ? V.len : (i < 2 * nsv ? U.len : 3 * (int64_t)nsv); }
};

}  // namespace

mk_solver *mk_make_trsvd() { return new TrsvdSolver(); }
