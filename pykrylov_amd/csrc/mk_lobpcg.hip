// mk_lobpcg.hip -- LOBPCG (Knyazev 2001): a block, preconditioned eigensolver with soft locking for a few extreme eigenpairs
// of a symmetric operator, device resident (solver kind MK_LOBPCG; no reference module).  The NumPy
// restatement is tests/_lobpcg_ref.py.
//
// nb = the block size, sgn = +1 for the smallest and -1 for the largest eigenvalues (the method minimises the Rayleigh
// quotient of sgn A).  Set-up: X = the start block, A X (nb products), the small problem of (sgn X'AX, X'X), X <- X C,
// A X <- (A X) C, and the residuals.  One pass of the driver = one iteration; all small matrices live on the host:
//   host   threshold = max(abstol, reltol anorm); the stop tests; soft locking: active = active and (rn > threshold), na columns
//       (a locked column stays locked; if nothing is active and the run has not converged, every column above the threshold
//       is active again and P is dropped); a column that leaves the active set drops its P column
//   W   W_k = precon R_j per active column j (a copy without one)                          [the preconditioner's launches]
//   O   W_k <- W_k - X (X'W_k), GM_GROUP columns of X per launch, twice; the last update accumulates <W_k, W_k>;
//       W_k <- W_k / ||W_k||                                                               [(4 ceil(nb / GM_GROUP) + 1) na launches]
//   P   A W_k                                                                              [na products, in A's format]
//   G   S = [X, W, P], AS = [AX, AW, AP], m = nb + na + np <= 48: S'S and S'(AS) by lb_gram_kernel, the tiles on and above the
//       diagonal in one launch each, then lb_total_kernel; one download of both            [4 launches]
//   host   H = sgn S'(AS) mirrored; d = diag(G)^-1/2; Cholesky of d G d with the pivot test v > 2^-26; T = L^-1 (d H d) L^-T
//       symmetrised; (theta, Z) = tr_jacobi(T); C = d L^-T Z.  A pivot that fails: the leading problem without P (a restart);
//       again: breakdown, the run ends with the last iterate.  One upload of the coefficients
//   R   X <- S C[:, :nb], AX <- AS C[:, :nb], P <- [W, P] C[nb:, active], AP likewise, by tr_rotate_kernel out of place into
//       the other column set (X and P both read S); an active column whose coefficients are all zero gets no P  [4 launches]
//   N   P_k, AP_k <- (1 / ||P_k||) (P_k, AP_k)                                             [2 np launches]
//   E   R = AX - X diag(sgn theta) and the nb column norms in one sweep; one download of the norms   [3 launches]
// A pass has two downloads: the host needs the norms of the rotated block before it can pick the next active set.
// Columns of n doubles moved per iteration beyond the products and the preconditioner, m = nb + 2 na: W 2 na (none with a
// general preconditioner), O na (2 (2 nb + 3 ceil(nb / 8)) + 2), G 2 x 16 per 8 x 8 tile, R 2 (m + nb) + 2 (m - nb + na),
// N 5 na, E 3 nb.
// Every operation rounds on its own (-ffp-contract=off); every inner product has the lanes, the grid and the tree of
// mk_stream_kernel<MkOpDot>, then mk_total -- the Gram kernel's entries included.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "mk_multicol.h"
#include "mk_rotate.h"
#include "mk_solver.h"

namespace {

constexpr int LB_MAXB = MK_LOBPCG_MAX_BLOCK;
constexpr int LB_MAXM = 3 * LB_MAXB;                         // columns of S = [X, W, P]
constexpr double LB_PIVOT = 0x1.0p-26;

struct LbOpStart {              // out = the hashed vector of `seed`
    static constexpr int NACC = 0, SLOT0 = 0;
    double *out;
    uint64_t seed;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 v;
        v.x = mk_cell_field(i, seed) - 1.0;
        v.y = mk_cell_field(i + 1, seed) - 1.0;
        mk_st2(out, i, v);
    }
    __device__ void one(int64_t i, double *) { out[i] = mk_cell_field(i, seed) - 1.0; }
};

// (a, b) <- (1 / sqrt(total)) (a, b), `total` the sum of the np partials at `part` (b may be null)
struct LbOpScale {
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *part;
    int np;
    double *a, *b;
    double s;
    __device__ bool prologue(double *s4, bool) {
        s = 1.0 / __dsqrt_rn(mk_total(part, np, s4));
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 v = mk_ld2(a, i);
        v.x = s * v.x;
        v.y = s * v.y;
        mk_st2(a, i, v);
        if (b) {
            double2 u = mk_ld2(b, i);
            u.x = s * u.x;
            u.y = s * u.y;
            mk_st2(b, i, u);
        }
    }
    __device__ void one(int64_t i, double *) {
        a[i] = s * a[i];
        if (b) b[i] = s * b[i];
    }
};

// E: R_c = AX_c - t_c X_c for the nb columns (ld apart) and the partial sums of <R_c, R_c> into slot c, in one sweep
struct LbOpResid {
    static constexpr int NACC = LB_MAXB, SLOT0 = 0;
    const double *X, *AX;
    double *R;
    int64_t ld;
    int nb;
    const double *st;            // sgn theta_c on the device
    double t[LB_MAXB];
    __device__ bool prologue(double *, bool) {
#pragma unroll
        for (int c = 0; c < LB_MAXB; ++c) t[c] = c < nb ? st[c] : 0.0;
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
#pragma unroll
        for (int c = 0; c < LB_MAXB; ++c)
            if (c < nb) {
                const size_t o = (size_t)c * (size_t)ld;
                const double2 x = mk_ld2(X + o, i), a = mk_ld2(AX + o, i);
                double2 r;
                r.x = a.x - t[c] * x.x;
                r.y = a.y - t[c] * x.y;
                mk_st2(R + o, i, r);
                acc[c] += r.x * r.x;
                acc[c] += r.y * r.y;
            }
    }
    __device__ void one(int64_t i, double *acc) {
#pragma unroll
        for (int c = 0; c < LB_MAXB; ++c)
            if (c < nb) {
                const size_t o = (size_t)c * (size_t)ld + (size_t)i;
                const double r = AX[o] - t[c] * X[o];
                R[o] = r;
                acc[c] += r * r;
            }
    }
};

// out[c] = sqrt(total of slot c), one workgroup per column
__global__ __launch_bounds__(MK_BLOCK) void lb_norms_kernel(const double *part, int np, double *out) {
    __shared__ double s4[4];
    const double v = __dsqrt_rn(mk_total(part + (size_t)blockIdx.x * MK_MAXP, np, s4));
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

__global__ void lb_status_kernel(MkStatus *st, int64_t itn, int64_t nmv) {
    st->itn = itn;
    st->nMatvec = nmv;
}

// G: the partial sums of the T x T tile (bi, bj), bi <= bj, of U'V for tall operands of m columns each, `ld` apart; blockIdx.y
// numbers the tiles on and above the diagonal row by row.  Lane g of the S = gridDim.x * MK_BLOCK lanes owns the row pairs
// g, g + S, ... and the odd tail row goes to lane (n / 2) % S, as in mk_stream_kernel; per entry (i, j) a lane adds
// u_i.x v_j.x, then u_i.y v_j.y -- MkOpDot's additions in its order -- so that the workgroup's sum lands in
// part[(i m + j) MK_MAXP + blockIdx.x] with the bits mk_stream_kernel<MkOpDot> gives the two columns.  T + T loads of 16
// bytes feed 2 T T multiply-adds.  A tile at the edge reads column i0 (j0) in place of the columns past m and drops the
// results; a diagonal tile computes the entries below the diagonal too, and nobody reads them.
template <int T>
__global__ __launch_bounds__(MK_BLOCK) void lb_gram_kernel(const double *__restrict__ U, const double *__restrict__ V, int64_t ld,
                                                           int m, double *__restrict__ part, int64_t n) {
    __shared__ double s4[4];
    const int nt = (m + T - 1) / T;
    int bi = 0, rest = (int)blockIdx.y;
    while (bi < nt - 1 && rest >= nt - bi) {
        rest -= nt - bi;
        ++bi;
    }
    const int bj = bi + rest;
    if (bj >= nt) return;
    const int i0 = bi * T, j0 = bj * T;
    const int ni = m - i0 < T ? m - i0 : T, nj = m - j0 < T ? m - j0 : T;
    const int64_t S = (int64_t)gridDim.x * MK_BLOCK;
    const int64_t g = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
    const int64_t npair = n >> 1;
    double acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = 0.0;
    for (int64_t q = g; q < npair; q += S) {
        double2 u[T], v[T];
#pragma unroll
        for (int i = 0; i < T; ++i) u[i] = mk_ld2(U + (size_t)(i0 + (i < ni ? i : 0)) * (size_t)ld, 2 * q);
#pragma unroll
        for (int j = 0; j < T; ++j) v[j] = mk_ld2(V + (size_t)(j0 + (j < nj ? j : 0)) * (size_t)ld, 2 * q);
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j) {
                acc[i][j] += u[i].x * v[j].x;
                acc[i][j] += u[i].y * v[j].y;
            }
    }
    if ((n & 1) && g == (npair % S)) {
        double u[T], v[T];
#pragma unroll
        for (int i = 0; i < T; ++i) u[i] = U[(size_t)(i0 + (i < ni ? i : 0)) * (size_t)ld + (size_t)(n - 1)];
#pragma unroll
        for (int j = 0; j < T; ++j) v[j] = V[(size_t)(j0 + (j < nj ? j : 0)) * (size_t)ld + (size_t)(n - 1)];
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j) acc[i][j] += u[i] * v[j];
    }
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
            if (i < ni && j < nj) {                          // (uniform over the workgroup: every lane meets the barriers)
                const double tot = mk_block_sum(acc[i][j], s4);
                if (threadIdx.x == 0) part[((size_t)(i0 + i) * m + (size_t)(j0 + j)) * MK_MAXP + blockIdx.x] = tot;
            }
}

// out[i m + j] = the total of entry (i, j), i <= j, one workgroup per entry; `transposed`: the composed Gram's slots (j m + i)
__global__ __launch_bounds__(MK_BLOCK) void lb_total_kernel(const double *part, int np, int m, int transposed, double *out) {
    __shared__ double s4[4];
    const int i = (int)blockIdx.x / m, j = (int)blockIdx.x % m;
    if (j < i) return;
    const size_t slot = transposed ? (size_t)j * m + i : (size_t)i * m + j;
    const double tot = mk_total(part + slot * MK_MAXP, np, s4);
    if (threadIdx.x == 0) out[(size_t)i * m + j] = tot;
}

// The small generalised problem H c = theta G c of order m (G, H row major with row length ldg, both triangles given):
// d = diag(G)^-1/2, the Cholesky factor L of d G d with the pivot test v > LB_PIVOT, T = L^-1 (d H d) L^-T symmetrised,
// tr_jacobi, C = d L^-T Z.  theta ascending, C (m x m, row major) with the vectors in its columns.  Returns the Jacobi
// sweeps, -1 when a pivot or a diagonal entry of G fails its test (NaN included), -2 when T is not finite or Jacobi does not
// end.  Restated operation by operation in tests/_lobpcg_ref.py (rayleigh_ritz).
int lb_small_problem(int m, const double *G, const double *H, int ldg, double *theta, double *C) {
    std::vector<double> d(m), Gs((size_t)m * m), Hs((size_t)m * m), L((size_t)m * m, 0.0), Y((size_t)m * m), Tt((size_t)m * m),
        a((size_t)m * m), z((size_t)m * m), Q((size_t)m * m);
    std::vector<int> order(m);
    const auto at = [m](std::vector<double> &M, int i, int j) -> double & { return M[(size_t)i * m + j]; };
    for (int i = 0; i < m; ++i) {
        const double g = G[(size_t)i * ldg + i];
        if (!(g > 0.0)) return -1;
        d[i] = 1.0 / std::sqrt(g);
    }
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            at(Gs, i, j) = (d[i] * G[(size_t)i * ldg + j]) * d[j];
            at(Hs, i, j) = (d[i] * H[(size_t)i * ldg + j]) * d[j];
        }
    for (int j = 0; j < m; ++j)
        for (int i = j; i < m; ++i) {
            double s = at(Gs, i, j);
            for (int k = 0; k < j; ++k) s = s - at(L, i, k) * at(L, j, k);
            if (i == j) {
                if (!(s > LB_PIVOT)) return -1;
                at(L, j, j) = std::sqrt(s);
            } else {
                at(L, i, j) = s / at(L, j, j);
            }
        }
    const auto forward = [&](std::vector<double> &B, std::vector<double> &out) {      // out = L^-1 B, row by row
        for (int i = 0; i < m; ++i)
            for (int c = 0; c < m; ++c) {
                double r = at(B, i, c);
                for (int k = 0; k < i; ++k) r = r - at(L, i, k) * at(out, k, c);
                at(out, i, c) = r / at(L, i, i);
            }
    };
    forward(Hs, Y);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) at(Q, i, j) = at(Y, j, i);
    forward(Q, Tt);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            at(a, i, j) = 0.5 * (at(Tt, i, j) + at(Tt, j, i));
            if (!std::isfinite(at(a, i, j))) return -2;
        }
    const int sweeps = tr_jacobi(m, a.data(), z.data(), order.data());
    if (sweeps < 0) return -2;
    for (int i = 0; i < m; ++i) theta[i] = at(a, order[i], order[i]);
    for (int i = m - 1; i >= 0; --i)
        for (int c = 0; c < m; ++c) {
            double r = at(z, i, order[c]);
            for (int k = i + 1; k < m; ++k) r = r - at(L, k, i) * at(Q, k, c);
            at(Q, i, c) = r / at(L, i, i);
        }
    for (int i = 0; i < m; ++i)
        for (int c = 0; c < m; ++c) C[(size_t)i * m + c] = d[i] * at(Q, i, c);
    return sweeps;
}

struct LobpcgSolver : mk_solver {
    double *d_ws = nullptr;          // the one allocation: the columns, then the small buffers below
    double *h_buf = nullptr;         // pinned: the Gram matrices and the norms on their way down, the coefficients on their way up
    double *colS[2] = {nullptr, nullptr}, *colAS[2] = {nullptr, nullptr}, *colR = nullptr;   // 3 nb columns each; R: nb
    double *d_gpart = nullptr, *d_gh = nullptr, *d_rpart = nullptr, *d_rn = nullptr, *d_st = nullptr, *d_Y = nullptr,
           *d_bank = nullptr, *d_h = nullptr, *d_ww = nullptr, *d_rec = nullptr;
    double *h_gh = nullptr, *h_rn = nullptr, *h_up = nullptr;
    hipEvent_t g0 = nullptr, g1 = nullptr;
    hipEvent_t ph[5] = {};           // an iteration's phases: [0] W [1] O [2] P [3] G, host and upload [4] R, N, E
    bool timed = false;
    double ph_ms[3] = {};            // of the last iteration: the preconditioner, the products, the rotations with N and E
    int nb = 0, nev = 0, which = 0, cb = 0, pm = 0;          // cb: the block the columns are sized for; pm: the probe's columns
    bool probe = false, allocated = false;
    int64_t ld = 0;
    size_t ws_bytes = 0, gslots = 0;
    double sgn = 1.0;
    // the run's host state
    int cur = 0, na = 0, p_at = 0, iters = 0, sweeps = 0, restarts = 0, breakdown = 0, conv = 0, nconv = 0;
    bool finished = false, has_p = false;
    int64_t nmv = 0;
    double anorm = 0.0, threshold = 0.0, resid = 0.0, gram_ms = 0.0;
    double theta[LB_MAXB] = {}, rn[LB_MAXB] = {};
    bool active[LB_MAXB] = {};
    int act[LB_MAXB] = {}, first_met[LB_MAXB] = {};
    std::vector<int> pcol;           // the columns of X that the stored P columns belong to, in storage order
    std::vector<double> G, H, C, thall;

    bool takes_precon() const override { return !probe; }

    ~LobpcgSolver() override {
        if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
        hipFree(d_ws);
        if (h_buf) hipHostFree(h_buf);
        if (g0) hipEventDestroy(g0);
        if (g1) hipEventDestroy(g1);
        for (hipEvent_t e : ph)
            if (e) hipEventDestroy(e);
    }

    double *xc(int s, int j) const { return colS[s] + (size_t)j * (size_t)ld; }
    double *axc(int s, int j) const { return colAS[s] + (size_t)j * (size_t)ld; }
    double *rcol(int j) const { return colR + (size_t)j * (size_t)ld; }
    double *bank(int b) const { return d_bank + (size_t)b * LB_MAXB * MK_MAXP; }

    template <class Op>
    void launch(const Op &op, double *partials) {
        hipLaunchKernelGGL(mk_stream_kernel<Op>, dim3(mk_grid_stream(n)), dim3(MK_BLOCK), 0, stream, op, n, next_halt(), partials);
    }

    GmCols cols(const double *base, int c0, int nc) const {
        GmCols v;
        for (int c = 0; c < GM_GROUP; ++c) v.col[c] = base + (size_t)(c0 + (c < nc ? c : 0)) * (size_t)ld;
        return v;
    }

    int allocate() {
        nb = eig_ncv;
        nev = eig_nev;
        which = eig_which;
        probe = prm.restart != 0;
        if (probe) {
            pm = eig_ncv;
            nb = nev = 1;
        }
        sgn = which == 0 ? 1.0 : -1.0;
        cb = probe ? LB_MAXB : nb;
        ld = ((n + 1) & ~(int64_t)1) + 2;    // n rounded up to even, and the 16 bytes of zeroed slack a product's input needs
        const size_t ncols = (size_t)13 * cb;
        gslots = (size_t)LB_MAXM * LB_MAXM + GM_GROUP;       // (a composed Gram's last launch writes GM_GROUP slots)
        const size_t small = 2 * gslots * MK_MAXP + 2 * (size_t)LB_MAXM * LB_MAXM + (size_t)LB_MAXB * MK_MAXP + 2 * LB_MAXB
                             + 2 * (size_t)LB_MAXM * LB_MAXB + 2 * (size_t)LB_MAXB * MK_MAXP + LB_MAXB + MK_MAXP + 3 * LB_MAXB;
        ws_bytes = sizeof(double) * (ncols * (size_t)ld + small);
        if (d_ws) return mk_fail(MK_ERR_STATE, "LOBPCG: an earlier set-up of this solver ran out of device memory");
        if (hipMalloc((void **)&d_ws, ws_bytes) != hipSuccess) {
            (void)hipGetLastError();
            d_ws = nullptr;
            return mk_fail(MK_ERR_HIP, "LOBPCG: out of device memory for the workspace: 13 x %d columns of %lld rows need %zu bytes; "
                           "a smaller block needs less", cb, (long long)n, ws_bytes);
        }
        MK_HIP(hipMemsetAsync(d_ws, 0, ws_bytes, stream));
        double *p = d_ws;
        const auto take = [&p](size_t cnt) {
            double *q = p;
            p += cnt;
            return q;
        };
        for (int s = 0; s < 2; ++s) {
            colS[s] = take((size_t)3 * cb * (size_t)ld);
            colAS[s] = take((size_t)3 * cb * (size_t)ld);
        }
        colR = take((size_t)cb * (size_t)ld);
        d_gpart = take(2 * gslots * MK_MAXP);
        d_gh = take(2 * (size_t)LB_MAXM * LB_MAXM);
        d_rpart = take((size_t)LB_MAXB * MK_MAXP);
        d_rn = take(LB_MAXB);
        d_st = take(LB_MAXB);
        d_Y = take(2 * (size_t)LB_MAXM * LB_MAXB);
        d_bank = take(2 * (size_t)LB_MAXB * MK_MAXP);
        d_h = take(LB_MAXB);
        d_ww = take(MK_MAXP);
        d_rec = take(3 * LB_MAXB);
        const size_t pinned = 2 * (size_t)LB_MAXM * LB_MAXM + LB_MAXB + 2 * (size_t)LB_MAXM * LB_MAXB + LB_MAXB + 3 * LB_MAXB;
        MK_HIP(hipHostMalloc((void **)&h_buf, sizeof(double) * pinned, hipHostMallocDefault));
        h_gh = h_buf;
        h_rn = h_gh + 2 * (size_t)LB_MAXM * LB_MAXM;
        h_up = h_rn + LB_MAXB;               // [the X coefficients | the P coefficients | sgn theta | the record]
        MK_HIP(hipEventCreate(&g0));
        MK_HIP(hipEventCreate(&g1));
        for (hipEvent_t &e : ph) MK_HIP(hipEventCreate(&e));
        allocated = true;
        return MK_OK;
    }

    // the Gram matrix U'V of m columns each into out (m x m, the entries on and above the diagonal), through the partial sums
    // of bank `b`
    void gram(const double *U, const double *V, int m, int b, double *out) {
        double *part = d_gpart + (size_t)b * gslots * MK_MAXP;
        const int grid = mk_grid_stream(n);
        if (prm.window == 1) {                               // composed of GmOpMultiDot launches: column j against 0 .. j
            for (int j = 0; j < m; ++j)
                for (int c0 = 0; c0 <= j; c0 += GM_GROUP) {
                    const int nc = j + 1 - c0 < GM_GROUP ? j + 1 - c0 : GM_GROUP;
                    hipLaunchKernelGGL(mk_stream_kernel<GmOpMultiDot>, dim3(grid), dim3(MK_BLOCK), 0, stream,
                                       GmOpMultiDot{V + (size_t)j * (size_t)ld, cols(U, c0, nc), nc}, n, MkHalt{d_nohalt, 0, 0},
                                       part + ((size_t)j * m + c0) * MK_MAXP);
                }
        } else {
            const int T = prm.window == 4 || prm.window == 8 ? prm.window : (m <= 8 ? 4 : 8);
            const int nt = (m + T - 1) / T;
            const dim3 g2(grid, nt * (nt + 1) / 2);
            if (T == 4) hipLaunchKernelGGL(lb_gram_kernel<4>, g2, dim3(MK_BLOCK), 0, stream, U, V, ld, m, part, n);
            else hipLaunchKernelGGL(lb_gram_kernel<8>, g2, dim3(MK_BLOCK), 0, stream, U, V, ld, m, part, n);
        }
        hipLaunchKernelGGL(lb_total_kernel, dim3(m * m), dim3(MK_BLOCK), 0, stream, part, np_stream, m, prm.window == 1 ? 1 : 0, out);
    }

    // both Gram matrices of the first m columns of column set s, on the host: G = S'S, H = sgn S'(AS), mirrored
    int grams_to_host(int s, int m) {
        MK_HIP(hipEventRecord(g0, stream));
        gram(colS[s], colS[s], m, 0, d_gh);
        gram(colS[s], colAS[s], m, 1, d_gh + (size_t)m * m);
        MK_HIP(hipEventRecord(g1, stream));
        MK_HIP(hipGetLastError());
        MK_HIP(hipMemcpyAsync(h_gh, d_gh, sizeof(double) * 2 * (size_t)m * m, hipMemcpyDeviceToHost, stream));
        MK_HIP(hipStreamSynchronize(stream));
        if (mk_ctx().pending_rc != MK_OK) return mk_ctx().pending_rc;          // (a host operator callback failed)
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g0, g1) == hipSuccess) gram_ms = ms;
        G.assign((size_t)m * m, 0.0);
        H.assign((size_t)m * m, 0.0);
        for (int i = 0; i < m; ++i)
            for (int j = i; j < m; ++j) {
                G[(size_t)i * m + j] = G[(size_t)j * m + i] = h_gh[(size_t)i * m + j];
                H[(size_t)i * m + j] = H[(size_t)j * m + i] = sgn * h_gh[(size_t)m * m + (size_t)i * m + j];
            }
        return MK_OK;
    }

    void rotate(const double *V, int rows, const double *Y, int nj, int NJ, double *W) {
        const dim3 grid(mk_grid_stream(n)), block(MK_BLOCK);
        if (NJ == 4) hipLaunchKernelGGL(tr_rotate_kernel<4>, grid, block, 0, stream, V, ld, rows, Y, nj, W, n);
        else if (NJ == 8) hipLaunchKernelGGL(tr_rotate_kernel<8>, grid, block, 0, stream, V, ld, rows, Y, nj, W, n);
        else hipLaunchKernelGGL(tr_rotate_kernel<16>, grid, block, 0, stream, V, ld, rows, Y, nj, W, n);
    }
    static int width(int nj) { return nj <= 4 ? 4 : (nj <= 8 ? 8 : 16); }

    // E, the download of the norms, and the host's part of the next iteration's head: the stop tests and the active set
    int residuals() {
        for (int j = 0; j < nb; ++j) h_up[2 * LB_MAXM * LB_MAXB + j] = sgn * theta[j];
        MK_HIP(hipMemcpyAsync(d_st, h_up + 2 * LB_MAXM * LB_MAXB, sizeof(double) * nb, hipMemcpyHostToDevice, stream));
        launch(LbOpResid{colS[cur], colAS[cur], colR, ld, nb, d_st, {}}, d_rpart);
        hipLaunchKernelGGL(lb_norms_kernel, dim3(nb), dim3(MK_BLOCK), 0, stream, d_rpart, np_stream, d_rn);
        hipLaunchKernelGGL(lb_status_kernel, dim3(1), dim3(1), 0, stream, d_status, (int64_t)iters, nmv);
        MK_HIP(hipGetLastError());
        MK_HIP(hipMemcpyAsync(h_rn, d_rn, sizeof(double) * nb, hipMemcpyDeviceToHost, stream));
        MK_HIP(hipStreamSynchronize(stream));
        for (int j = 0; j < nb; ++j) rn[j] = h_rn[j];
        if (timed) {                                         // (everything up to the norms has finished)
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ph[0], ph[1]) == hipSuccess) ph_ms[0] = ms;
            if (hipEventElapsedTime(&ms, ph[2], ph[3]) == hipSuccess) ph_ms[1] = ms;
            MK_HIP(hipEventRecord(g0, stream));
            MK_HIP(hipEventSynchronize(g0));
            if (hipEventElapsedTime(&ms, ph[4], g0) == hipSuccess) ph_ms[2] = ms;
            timed = false;
        }
        const double rel = prm.reltol * anorm;
        threshold = rel > prm.abstol ? rel : prm.abstol;
        resid = 0.0;
        nconv = 0;
        for (int j = 0; j < nev; ++j) {
            if (!(rn[j] <= resid)) resid = rn[j];            // (a NaN is the largest)
            if (rn[j] <= threshold) {
                nconv += 1;
                if (first_met[j] < 0) first_met[j] = iters;
            }
        }
        hist.push_back(resid);
        hist2.push_back(0.0);
        conv = nconv == nev ? 1 : 0;
        if (conv || breakdown) return finalize();
        bool any = false;
        for (int j = 0; j < nb; ++j) {
            active[j] = active[j] && rn[j] > threshold;
            any = any || active[j];
        }
        if (!any) {                                          // every column was locked, and a wanted one came back
            for (int j = 0; j < nb; ++j) active[j] = rn[j] > threshold;
            has_p = false;
            pcol.clear();
            restarts += 1;
        }
        na = 0;
        for (int j = 0; j < nb; ++j)
            if (active[j]) act[na++] = j;
        if (na == 0 || nmv + (int64_t)na > prm.matvec_max) return finalize();   // (na == 0: only norms that are not finite)
        return MK_OK;
    }

    // the end: the record and the halt words for the driver
    int finalize() {
        double *rec = h_up + 2 * LB_MAXM * LB_MAXB + LB_MAXB;
        for (int i = 0; i < nev; ++i) {
            const int c = which == 0 ? i : nev - 1 - i;
            rec[3 * i] = sgn * theta[c];
            rec[3 * i + 1] = rn[c];
            rec[3 * i + 2] = (double)first_met[c];
        }
        MK_HIP(hipMemcpyAsync(d_rec, rec, sizeof(double) * 3 * (size_t)nev, hipMemcpyHostToDevice, stream));
        static const int up[2] = {1, 1};
        MK_HIP(hipMemcpyAsync(d_halt, up, sizeof(up), hipMemcpyHostToDevice, stream));
        MK_HIP(hipStreamSynchronize(stream));
        finished = true;
        return MK_OK;
    }

    int setup(const double *start, const double *guess) override {
        if (guess) return mk_fail(MK_ERR_ARG, "mk_solver_setup: LOBPCG takes a start block and no initial guess");
        if (prm.restart == 0 && prm.matvec_max < (int64_t)eig_ncv)
            return mk_fail(MK_ERR_ARG, "mk_solver_setup: LOBPCG matvec_max = %lld is below the block size %d: the products of the "
                           "start block do not fit", (long long)prm.matvec_max, eig_ncv);
        int rc;
        if (!allocated && (rc = allocate()) != MK_OK) return rc;
        cur = na = p_at = iters = sweeps = restarts = breakdown = conv = nconv = 0;
        finished = has_p = false;
        nmv = 0;
        anorm = threshold = resid = gram_ms = 0.0;
        ph_ms[0] = ph_ms[1] = ph_ms[2] = 0.0;
        timed = false;
        pcol.clear();
        for (int j = 0; j < LB_MAXB; ++j) {
            theta[j] = rn[j] = 0.0;
            active[j] = true;
            first_met[j] = -1;
        }
        const int ncol = probe ? pm : nb;
        for (int j = 0; j < ncol; ++j) {                     // (a column of the caller's block need not be 16-byte aligned: a copy)
            if (start)
                MK_HIP(hipMemcpyAsync(xc(0, j), start + (size_t)j * (size_t)n, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice,
                                      stream));
            else
                launch(LbOpStart{xc(0, j), eig_seed + (uint64_t)j}, d_part);
        }
        if (probe) {                                         // the Gram kernel alone: U'U of the start block, mirrored
            if ((rc = grams_to_host(0, pm)) != MK_OK) return rc;
            MK_HIP(hipMemcpyAsync(d_gh, G.data(), sizeof(double) * (size_t)pm * pm, hipMemcpyHostToDevice, stream));
            return finalize();
        }
        for (int j = 0; j < nb; ++j) mk_launch_spmv(this, xc(0, j), MkPlainEpi{axc(0, j)});
        nmv = nb;
        if ((rc = grams_to_host(0, nb)) != MK_OK) return rc;
        thall.assign(LB_MAXM, 0.0);
        C.assign((size_t)LB_MAXM * LB_MAXM, 0.0);
        const int sw = lb_small_problem(nb, G.data(), H.data(), nb, thall.data(), C.data());
        if (sw == -2)
            return mk_fail(MK_ERR_ARG, "LOBPCG: the projected matrix of the start block is not finite (a matrix or start block with "
                           "entries that are not finite, or overflow)");
        if (sw < 0) {                                        // a start block that is (numerically) rank deficient
            breakdown = 1;
            for (int j = 0; j < nb; ++j) {
                const double g = G[(size_t)j * nb + j];
                theta[j] = g > 0.0 ? H[(size_t)j * nb + j] / g : 0.0;
                if (!std::isfinite(theta[j])) theta[j] = 0.0;
                if (std::fabs(theta[j]) > anorm) anorm = std::fabs(theta[j]);
            }
            return residuals();
        }
        sweeps = sw;
        const int NJ = width(nb);
        for (int c = 0; c < nb; ++c)
            for (int j = 0; j < NJ; ++j) h_up[(size_t)c * NJ + j] = j < nb ? C[(size_t)c * nb + j] : 0.0;
        MK_HIP(hipMemcpyAsync(d_Y, h_up, sizeof(double) * (size_t)nb * NJ, hipMemcpyHostToDevice, stream));
        rotate(colS[0], nb, d_Y, nb, NJ, colS[1]);
        rotate(colAS[0], nb, d_Y, nb, NJ, colAS[1]);
        cur = 1;
        for (int j = 0; j < nb; ++j) {
            theta[j] = thall[j];
            if (std::fabs(thall[j]) > anorm) anorm = std::fabs(thall[j]);
        }
        return residuals();
    }

    int enqueue_pass() override {
        if (finished) return MK_OK;
        int rc;
        const int s = cur, o = 1 - cur;
        // a column that left the active set drops its P column: the others move down behind the na columns of W
        if (has_p) {
            std::vector<int> kept;
            int dst = nb + na;
            for (size_t k = 0; k < pcol.size(); ++k) {
                if (!active[pcol[k]]) continue;
                const int src = p_at + (int)k;
                if (src != dst) {
                    MK_HIP(hipMemcpyAsync(xc(s, dst), xc(s, src), sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
                    MK_HIP(hipMemcpyAsync(axc(s, dst), axc(s, src), sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
                }
                kept.push_back(pcol[k]);
                dst += 1;
            }
            pcol.swap(kept);
            p_at = nb + na;
        }
        const int np_cols = has_p ? (int)pcol.size() : 0;
        // W, O
        MK_HIP(hipEventRecord(ph[0], stream));
        for (int k = 0; k < na; ++k) {
            double *w = xc(s, nb + k);
            const double *r = rcol(act[k]);
            if (slot[0].kind == MK_PRECON_NONE) launch(MkOpCopy{r, w}, d_part);
            else if (general_precon()) {
                if ((rc = apply_precon(r, w)) != MK_OK) return rc;
            } else launch(MkOpMul{d_prec(), r, w}, d_part);
        }
        MK_HIP(hipEventRecord(ph[1], stream));
        for (int k = 0; k < na; ++k) {
            double *w = xc(s, nb + k);
            for (int p = 0; p < 2; ++p) {
                for (int c0 = 0; c0 < nb; c0 += GM_GROUP) {
                    const int nc = nb - c0 < GM_GROUP ? nb - c0 : GM_GROUP;
                    launch(GmOpMultiDot{w, cols(colS[s], c0, nc), nc}, bank(p) + (size_t)c0 * MK_MAXP);
                }
                for (int c0 = 0; c0 < nb; c0 += GM_GROUP) {
                    const int nc = nb - c0 < GM_GROUP ? nb - c0 : GM_GROUP;
                    const bool last = p == 1 && c0 + GM_GROUP >= nb;
                    if (last)
                        launch(GmOpUpdate<true>{bank(p) + (size_t)c0 * MK_MAXP, np_stream, d_h + c0, p, w, cols(colS[s], c0, nc), nc, {}},
                               d_ww);
                    else
                        launch(GmOpUpdate<false>{bank(p) + (size_t)c0 * MK_MAXP, np_stream, d_h + c0, p, w, cols(colS[s], c0, nc), nc, {}},
                               d_ww);
                }
            }
            launch(LbOpScale{d_ww, np_stream, w, nullptr, 0.0}, d_part);
        }
        // P
        MK_HIP(hipEventRecord(ph[2], stream));
        for (int k = 0; k < na; ++k) mk_launch_spmv(this, xc(s, nb + k), MkPlainEpi{axc(s, nb + k)});
        nmv += na;
        MK_HIP(hipEventRecord(ph[3], stream));
        // G
        int m = nb + na + np_cols;
        if ((rc = grams_to_host(s, m)) != MK_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        int sw = lb_small_problem(m, G.data(), H.data(), m, thall.data(), C.data());
        if (sw == -1 && np_cols > 0) {                       // drop P and solve the leading problem again
            restarts += 1;
            const int full = m;
            m = nb + na;
            sw = lb_small_problem(m, G.data(), H.data(), full, thall.data(), C.data());
        }
        if (sw == -2)
            return mk_fail(MK_ERR_ARG, "LOBPCG: the projected matrix of iteration %d is not finite (a matrix, preconditioner or start "
                           "block with entries that are not finite, or overflow)", iters + 1);
        if (sw < 0) {                                        // X, theta and the norms are the last iterate's
            breakdown = 1;
            hipLaunchKernelGGL(lb_status_kernel, dim3(1), dim3(1), 0, stream, d_status, (int64_t)iters, nmv);
            return finalize();
        }
        sweeps = sw;
        for (int i = 0; i < m; ++i)
            if (std::fabs(thall[i]) > anorm) anorm = std::fabs(thall[i]);
        // R: the coefficients go up once, the rotations write the other column set
        // (a column of X that takes nothing from W and P -- a locked vector that moved into an active place when the Ritz
        //  values changed their order -- has a P of exact zeros: it gets none)
        const int prow = m - nb;
        int pk[LB_MAXB], npn = 0;
        for (int k = 0; k < na; ++k) {
            bool nz = false;
            for (int c = 0; c < prow; ++c) nz = nz || C[(size_t)(nb + c) * m + act[k]] != 0.0;
            if (nz) pk[npn++] = k;
        }
        const int NJx = width(nb), NJp = width(npn);
        double *yx = h_up, *yp = h_up + (size_t)LB_MAXM * LB_MAXB;
        for (int c = 0; c < m; ++c)
            for (int j = 0; j < NJx; ++j) yx[(size_t)c * NJx + j] = j < nb ? C[(size_t)c * m + j] : 0.0;
        for (int c = 0; c < prow; ++c)
            for (int j = 0; j < NJp; ++j) yp[(size_t)c * NJp + j] = j < npn ? C[(size_t)(nb + c) * m + act[pk[j]]] : 0.0;
        MK_HIP(hipMemcpyAsync(d_Y, h_up, sizeof(double) * 2 * (size_t)LB_MAXM * LB_MAXB, hipMemcpyHostToDevice, stream));
        const double *dyp = d_Y + (size_t)LB_MAXM * LB_MAXB;
        MK_HIP(hipEventRecord(ph[4], stream));
        rotate(colS[s], m, d_Y, nb, NJx, colS[o]);
        rotate(colAS[s], m, d_Y, nb, NJx, colAS[o]);
        if (npn > 0) {
            rotate(xc(s, nb), prow, dyp, npn, NJp, xc(o, nb + na));
            rotate(axc(s, nb), prow, dyp, npn, NJp, axc(o, nb + na));
        }
        // N
        for (int k = 0; k < npn; ++k) {
            launch(MkOpDot<0>{xc(o, nb + na + k), xc(o, nb + na + k)}, d_ww);
            launch(LbOpScale{d_ww, np_stream, xc(o, nb + na + k), axc(o, nb + na + k), 0.0}, d_part);
        }
        cur = o;
        has_p = npn > 0;
        p_at = nb + na;
        pcol.clear();
        for (int k = 0; k < npn; ++k) pcol.push_back(act[pk[k]]);
        for (int j = 0; j < nb; ++j) theta[j] = thall[j];
        iters += 1;
        const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        timed = true;
        rc = residuals();
        if (!hist2.empty()) hist2.back() = host_ms;
        return rc;
    }

    int finish(mk_result *res) override {
        int rc = poll();
        if (rc != MK_OK) return rc;
        fill_result(res);
        res->nMatvec = nmv;
        res->itn = iters;
        res->converged = conv;
        res->residNorm = resid;
        res->threshold = threshold;
        res->Anorm = anorm;
        res->aux[0] = (double)iters;
        res->aux[1] = (double)(probe ? pm : nb);
        res->aux[2] = (double)na;
        res->aux[3] = (double)ws_bytes;
        res->aux[4] = (double)nconv;
        res->aux[5] = (double)breakdown;
        res->aux[6] = (double)sweeps;
        res->aux[7] = probe ? gram_ms : (double)restarts;
        res->Acond = gram_ms;                                // (measurements of the last iteration, in milliseconds: the two Gram
        res->Arnorm = ph_ms[0];                              //  matrices; the preconditioner; the products; the rotations with
        res->ynorm = ph_ms[1];                               //  the scaling of P and the residuals)
        res->xnorm = ph_ms[2];
        return MK_OK;
    }

    const double *x() const override { return vector(0); }
    const double *vector(int i) const override {
        if (!allocated || i < 0) return nullptr;
        if (probe) return i == 0 ? d_gh : nullptr;
        if (i > nev) return nullptr;
        return i < nev ? xc(cur, which == 0 ? i : nev - 1 - i) : d_rec;
    }
    int64_t vector_len(int i) const override {
        if (probe) return (int64_t)pm * pm;
        return i == nev ? 3 * (int64_t)nev : n;
    }
};

}  // namespace

mk_solver *mk_make_lobpcg() { return new LobpcgSolver(); }
