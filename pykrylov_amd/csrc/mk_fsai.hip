// mk_fsai.hip -- FSAI, the factorized sparse approximate inverse of Kolotilina and Yeremin, of a symmetric positive definite
// device CSR matrix A ~ L L' (the preconditioner `precon * r` of mk_solver_set_precon_fsai).
//
// G ~ L^-1 is lower triangular on a fixed pattern (the stored lower triangle of A, or one the caller gives); the
// preconditioner is M^-1 = G' G.  Row i of G with pattern columns P[0] < ... < P[m-1] = i is the last row of inv(A[P, P]),
// scaled so that (G A G')_ii = 1: one small dense SPD solve per row, all rows independent -- no levels, no schedule.  An
// apply is two plain products, tmp = G in and out = G' tmp, through the product kernels and storage formats of every other
// matrix of the library.
//
//   gather    S[a][b] = A[P[a], P[b]], b <= a: the lower part of row P[a] of A merged with P (both ascending); a position A
//             does not store is 0.0, a stored zero is stored
//   Cholesky  s = S[a][b]; k = 0 .. b-1: s = s - L[a][k] L[b][k];  L[a][a] = sqrt(s), L[a][b] = s / L[b][b]
//   solve     y[m-1] = 1.0 / L[m-1][m-1];  a = m-1 .. 0: s = y[a] (0.0 below m-1); k = m-1 .. a+1: s = s - L[k][a] y[k];
//             y[a] = s / L[a][a]
//   scaling   g = y / sqrt(y[m-1])
//
// Every operation rounds on its own (-ffp-contract=off) and every entry is ONE sequential sum in the order written, whichever
// lane forms it: the factor does not depend on which kernel runs, on the lanes per row or on the grid.
#include <chrono>
#include <climits>
#include <cmath>

#include "mk_solver.h"

constexpr int MK_FSAI_SHORT = 4;          // longest row of the register kernel (5- and 7-point stencils: 3 and 4)

struct mk_fsai : MkDeviceOp {
    mk_csr *G = nullptr, *Gt = nullptr;   // owned
    double *d_tmp = nullptr;              // G in
    int *d_status = nullptr;              // smallest failing row of the set-up (INT_MAX: none)
    int64_t nnz = 0;
    int longest = 0;                      // longest row of G
    double setup_us = 0.0;
    size_t bytes = 0;                     // device bytes owned (CSR arrays, the vector, the words)
    ~mk_fsai() override;
    const char *noun() const override { return "FSAI preconditioner"; }
    int enqueue(const double *in, double *out, hipStream_t stream, int *flags, int64_t *q) const override;
};

// ------------------------------------------------------------------ the pattern from A
__global__ void mk_fsai_status_init(int *status) {
    if (threadIdx.x == 0) *status = INT_MAX;
}

// count[r + 1] = stored entries of row r with column <= r; a row that does not end there with its diagonal (or starts with
// a negative column) goes into *status
__global__ __launch_bounds__(MK_BLOCK) void mk_fsai_count_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                int64_t n, int32_t *__restrict__ count, int *status) {
    for (int64_t r = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * MK_BLOCK) {
        const int p0 = indptr[r], p1 = indptr[r + 1];
        int c = 0, last = -1;
        bool neg = false;
        for (int p = p0; p < p1; ++p) {
            const int j = indices[p];
            neg = neg || j < 0;
            if (j <= r) {
                ++c;
                last = j;
            }
        }
        if (last != (int)r || neg) atomicMin(status, (int)r);
        count[r + 1] = c;
    }
}

__global__ __launch_bounds__(MK_BLOCK) void mk_fsai_fill_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                               int64_t n, const int32_t *__restrict__ gptr, int32_t *__restrict__ gidx) {
    for (int64_t r = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * MK_BLOCK) {
        const int p1 = indptr[r + 1], q1 = gptr[r + 1];
        int q = gptr[r];
        for (int p = indptr[r]; p < p1 && q < q1; ++p)
            if (indices[p] <= r) gidx[q++] = indices[p];
    }
}

// ------------------------------------------------------------------ the set-up kernels
__host__ __device__ constexpr int mk_tri(int a, int b) { return a * (a + 1) / 2 + b; }   // packed lower triangle

// Rows of at most MK_FSAI_SHORT entries: one lane per row, everything in registers (every index below is a compile-time
// constant after unrolling: no scratch).
__global__ __launch_bounds__(MK_BLOCK) void mk_fsai_setup_short(const int32_t *__restrict__ aip, const int32_t *__restrict__ aix,
                                                               const double *__restrict__ av, const int32_t *__restrict__ gip,
                                                               const int32_t *__restrict__ gix, double *__restrict__ gv, int64_t n,
                                                               int *status) {
    constexpr int M = MK_FSAI_SHORT;
    for (int64_t i = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MK_BLOCK) {
        const int q0 = gip[i];
        const int m = gip[i + 1] - q0;
        int P[M];
#pragma unroll
        for (int a = 0; a < M; ++a) P[a] = a < m ? gix[q0 + a] : -1;
        double L[mk_tri(M - 1, M - 1) + 1];
#pragma unroll
        for (int k = 0; k <= mk_tri(M - 1, M - 1); ++k) L[k] = 0.0;
#pragma unroll
        for (int a = 0; a < M; ++a)
            if (a < m) {
                const int r = P[a], p1 = aip[r + 1];
                for (int p = aip[r]; p < p1; ++p) {
                    const int c = aix[p];
                    if (c > r) break;
                    const double v = av[p];
#pragma unroll
                    for (int b = 0; b <= a; ++b)
                        if (c == P[b]) L[mk_tri(a, b)] = v;
                }
            }
        bool bad = false;
#pragma unroll
        for (int b = 0; b < M; ++b)
            if (b < m) {
                double d = L[mk_tri(b, b)];
#pragma unroll
                for (int k = 0; k < b; ++k) d = d - L[mk_tri(b, k)] * L[mk_tri(b, k)];
                bad = bad || !(d > 0.0) || !isfinite(d);
                const double ld = sqrt(d);
                L[mk_tri(b, b)] = ld;
#pragma unroll
                for (int a = b + 1; a < M; ++a)
                    if (a < m) {
                        double s = L[mk_tri(a, b)];
#pragma unroll
                        for (int k = 0; k < b; ++k) s = s - L[mk_tri(a, k)] * L[mk_tri(b, k)];
                        L[mk_tri(a, b)] = s / ld;
                    }
            }
        double y[M], ylast = 0.0;
#pragma unroll
        for (int a = M - 1; a >= 0; --a) {
            y[a] = 0.0;
            if (a < m) {
                double s = (a == m - 1) ? 1.0 / L[mk_tri(a, a)] : 0.0;
#pragma unroll
                for (int k = M - 1; k > a; --k)
                    if (k < m) s = s - L[mk_tri(k, a)] * y[k];
                y[a] = s / L[mk_tri(a, a)];
                if (a == m - 1) ylast = y[a];
            }
        }
        const double sd = sqrt(ylast);
#pragma unroll
        for (int a = 0; a < M; ++a)
            if (a < m) gv[q0 + a] = y[a] / sd;
        if (bad) atomicMin(status, (int)i);
    }
}

// Rows of up to MK_FSAI_MAX_ROW entries: GL lanes per row, MK_BLOCK / GL rows per workgroup, the row's packed triangle in
// LDS.  Per row `stride` doubles (odd, so that the rows of one wave start on different banks): the triangle of `mmax` rows,
// ys (the running sums of the solve), dl (the diagonal of L) and P.  Column b of L is formed by the lanes together, entry
// (a, b) by lane (a - b - 1) % GL, after every lane has formed L[b][b] for itself (the same sequential sum: the same bits);
// the solve runs k = m-1 .. 0, every lane forms y[k] for itself and the lanes subtract L[k][a] y[k] from the sums a < k.
// All loops that hold a barrier run to `mmax`, which is uniform over the grid.
template <int GL>
__global__ __launch_bounds__(MK_BLOCK) void mk_fsai_setup_long(const int32_t *__restrict__ aip, const int32_t *__restrict__ aix,
                                                              const double *__restrict__ av, const int32_t *__restrict__ gip,
                                                              const int32_t *__restrict__ gix, double *__restrict__ gv, int64_t n,
                                                              int mmax, int stride, int *status) {
    extern __shared__ double mk_fsai_lds[];
    constexpr int RPB = MK_BLOCK / GL;
    const int grp = (int)threadIdx.x / GL, lane = (int)threadIdx.x % GL;
    double *const L = mk_fsai_lds + (size_t)grp * stride;
    double *const ys = L + mk_tri(mmax - 1, mmax - 1) + 1;
    double *const dl = ys + mmax;
    int *const P = reinterpret_cast<int *>(dl + mmax);
    for (int64_t base = (int64_t)blockIdx.x * RPB; base < n; base += (int64_t)gridDim.x * RPB) {
        const int64_t i = base + grp;
        const int q0 = i < n ? gip[i] : 0;
        const int m = i < n ? gip[i + 1] - q0 : 0;              // (<= mmax: the host has looked at every row)
        for (int a = lane; a < m; a += GL) P[a] = gix[q0 + a];
        __syncthreads();
        for (int a = lane; a < m; a += GL) {                    // gather row a of S
            double *const row = L + mk_tri(a, 0);
            for (int b = 0; b <= a; ++b) row[b] = 0.0;
            const int r = P[a], p1 = aip[r + 1];
            int b = 0;
            for (int p = aip[r]; p < p1 && b <= a; ++p) {
                const int c = aix[p];
                if (c > r) break;
                while (b <= a && P[b] < c) ++b;
                if (b <= a && P[b] == c) row[b++] = av[p];
            }
        }
        __syncthreads();
        bool bad = false;
        for (int b = 0; b < mmax; ++b) {                        // column b of L
            if (b < m) {
                const double *const rb = L + mk_tri(b, 0);
                double d = rb[b];
                for (int k = 0; k < b; ++k) d = d - rb[k] * rb[k];
                bad = bad || !(d > 0.0) || !isfinite(d);
                const double ld = sqrt(d);
                if (lane == 0) dl[b] = ld;                      // (rb[b] keeps S[b][b]: other lanes may still be reading it)
                for (int a = b + 1 + lane; a < m; a += GL) {
                    double *const ra = L + mk_tri(a, 0);
                    double s = ra[b];
                    for (int k = 0; k < b; ++k) s = s - ra[k] * rb[k];
                    ra[b] = s / ld;
                }
            }
            __syncthreads();
        }
        for (int a = lane; a < m; a += GL) ys[a] = (a == m - 1) ? 1.0 / dl[a] : 0.0;
        __syncthreads();
        double sd = 0.0;
        for (int k = mmax - 1; k >= 0; --k) {                   // y[k], then its term of every sum below it
            if (k < m) {
                const double yk = ys[k] / dl[k];
                if (k == m - 1) sd = sqrt(yk);
                if (lane == 0) gv[q0 + k] = yk / sd;
                const double *const rk = L + mk_tri(k, 0);
                for (int a = lane; a < k; a += GL) ys[a] = ys[a] - rk[a] * yk;
            }
            __syncthreads();
        }
        if (bad && lane == 0) atomicMin(status, (int)i);
    }
}

// doubles of LDS per row of the long kernel: the triangle, ys, dl, P (ints), rounded up to an odd number
static inline int mk_fsai_stride(int mmax) {
    const int s = mk_tri(mmax - 1, mmax - 1) + 1 + 2 * mmax + (mmax + 1) / 2;
    return s | 1;
}

// ------------------------------------------------------------------ the apply
// out = G' (G in) (in == out allowed: the first product writes d_tmp).  `q` = the solver's kernel counter (halt parity), or
// null for a standalone run.  Used by mk_fsai_apply and by the solvers' preconditioner sites (mk_solver.hip, mk_lls.hip).
int mk_fsai::enqueue(const double *in, double *out, hipStream_t st, int *flags, int64_t *q) const {
    if (n == 0) return MK_OK;
    const auto next = [&] { return halt(flags, q); };
    double *const nopart = nullptr;                              // (no fused dots: no partial sums are written)
    mk_spmv_launch_blocks(G, mk_grid_spmv_for(G), st, in, MkPlainEpi{d_tmp}, MkNoGate(), next, nopart);
    mk_spmv_launch_blocks(Gt, mk_grid_spmv_for(Gt), st, d_tmp, MkPlainEpi{out}, MkNoGate(), next, nopart);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

mk_fsai::~mk_fsai() {
    if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
    hipFree(d_tmp);
    hipFree(d_status);
    if (G) mk_csr_destroy(G);
    if (Gt) mk_csr_destroy(Gt);
}

// ======================================================================================
// C ABI
// ======================================================================================
static inline unsigned mk_fsai_grid(int64_t items, int per_block) {
    int64_t g = (items + per_block - 1) / per_block;
    const int64_t cap = 32 * (int64_t)(mk_ctx().num_cu > 0 ? mk_ctx().num_cu : 256);
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

extern "C" int mk_fsai_create(const mk_csr *A, const int32_t *pat_indptr, const int32_t *pat_indices, mk_fsai **out) {
    MK_REQUIRE_INIT();
    MK_ARG(A && out);
    MK_ARG((pat_indptr == nullptr) == (pat_indices == nullptr));
    const char *fn = "mk_fsai_create";
    if (A->comp_kind || A->host_fn || A->alias || A->nops)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator holds no CSR arrays of its own (a composite, reduced, block, "
                       "composed or matrix-free operator): form its matrix with to_csr_arrays() and a CsrOperator", fn);
    if (A->ex.mode >= 0 || A->row_block)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator is row-partitioned (it carries an exchange plan); the FSAI "
                       "preconditioner is single-GPU", fn);
    if (A->nrows != A->ncols)
        return mk_fail(MK_ERR_ARG, "%s: the matrix must be square, got %lld x %lld", fn, (long long)A->nrows,
                       (long long)A->ncols);
    if (A->nrows >= ((int64_t)1 << 31) - 1)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: %lld rows; the status word names a row in 32 bits (< 2^31 - 1)", fn,
                       (long long)A->nrows);
    if (A->nnz > 0 && (!A->d_indices || !A->d_data))
        return mk_fail(MK_ERR_STATE, "%s: the CSR arrays of this matrix were released", fn);
    const auto t0 = std::chrono::steady_clock::now();
    MkContext &c = mk_ctx();
    const int64_t n = A->nrows;
    // a given pattern: every check on the host, before a kernel reads through it
    if (pat_indptr) {
        if (pat_indptr[0] != 0) return mk_fail(MK_ERR_ARG, "%s: the pattern's indptr[0] is %d, not 0", fn, (int)pat_indptr[0]);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t p0 = pat_indptr[i], p1 = pat_indptr[i + 1];
            if (p1 <= p0)
                return mk_fail(MK_ERR_ARG, "%s: row %lld of the pattern is empty or its indptr decreases (every row ends with "
                               "its diagonal entry)", fn, (long long)i);
            for (int64_t p = p0; p < p1; ++p) {
                const int64_t j = pat_indices[p];
                if (j < 0 || j > i)
                    return mk_fail(MK_ERR_ARG, "%s: row %lld of the pattern holds column %lld: the pattern must be lower "
                                   "triangular", fn, (long long)i, (long long)j);
                if (p > p0 && j <= pat_indices[p - 1])
                    return mk_fail(MK_ERR_ARG, "%s: row %lld of the pattern is not sorted or repeats a column", fn, (long long)i);
            }
            if (pat_indices[p1 - 1] != i)
                return mk_fail(MK_ERR_ARG, "%s: row %lld of the pattern does not end with its diagonal entry", fn, (long long)i);
            if (p1 - p0 > MK_FSAI_MAX_ROW)
                return mk_fail(MK_ERR_ARG, "%s: row %lld of the pattern has %lld entries, more than MK_FSAI_MAX_ROW = %d", fn,
                               (long long)i, (long long)(p1 - p0), MK_FSAI_MAX_ROW);
        }
    }
    mk_fsai *F = new mk_fsai();
    F->n = n;
    int32_t *d_count = nullptr;
    const auto fail = [&](int code) {
        hipFree(d_count);
        delete F;
        return code;
    };
    // (16 bytes of slack behind the vector, zeroed: the product kernels read their input in 16-byte pairs)
    const size_t vbytes = sizeof(double) * (size_t)(n > 0 ? n : 1) + 16;
    if (hipMalloc((void **)&F->d_tmp, vbytes) != hipSuccess || hipMemsetAsync(F->d_tmp, 0, vbytes, c.stream) != hipSuccess ||
        hipMalloc((void **)&F->d_status, sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory for the vector (%zu bytes)", fn, vbytes));
    }
    int rc = F->init_nohalt(c.stream);
    if (rc != MK_OK) return fail(rc);
    F->bytes += vbytes + 3 * sizeof(int);                        // (the status word and the two halt words)
    int *const d_status = F->d_status;
    hipLaunchKernelGGL(mk_fsai_status_init, dim3(1), dim3(64), 0, c.stream, d_status);
    const size_t pbytes = sizeof(int32_t) * (size_t)(n + 1);
    std::vector<int32_t> h((size_t)n + 1, 0);
    int bad = INT_MAX;
    if (pat_indptr) {
        memcpy(h.data(), pat_indptr, pbytes);
    } else {
        // the stored lower triangle of A: a count per row, a host scan of n ints (as mk_csr_transpose does), a fill
        if (hipMalloc((void **)&d_count, pbytes) != hipSuccess || hipMemsetAsync(d_count, 0, pbytes, c.stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory for the row counts", fn));
        }
        if (n > 0)
            hipLaunchKernelGGL(mk_fsai_count_kernel, dim3(mk_fsai_grid(n, MK_BLOCK)), dim3(MK_BLOCK), 0, c.stream, A->d_indptr,
                               A->d_indices, n, d_count, d_status);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h.data(), d_count, pbytes, hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
            hipMemcpyAsync(&bad, d_status, sizeof(int), hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
            hipStreamSynchronize(c.stream) != hipSuccess)
            return fail(mk_fail(MK_ERR_HIP, "%s: counting the lower triangle failed", fn));
        if (bad != INT_MAX)
            return fail(mk_fail(MK_ERR_ARG, "%s: row %d stores no diagonal entry (every row must store its diagonal), or a "
                                "negative column", fn, bad));
        for (int64_t i = 0; i < n; ++i) {
            if (h[i + 1] > MK_FSAI_MAX_ROW)
                return fail(mk_fail(MK_ERR_ARG, "%s: row %lld of the pattern has %d entries, more than MK_FSAI_MAX_ROW = %d", fn,
                                    (long long)i, (int)h[i + 1], MK_FSAI_MAX_ROW));
            h[i + 1] += h[i];
        }
    }
    int longest = 0;
    for (int64_t i = 0; i < n; ++i) longest = h[i + 1] - h[i] > longest ? h[i + 1] - h[i] : longest;
    F->longest = longest;
    F->nnz = h[(size_t)n];
    rc = mk_csr_alloc(n, n, F->nnz, &F->G);
    if (rc != MK_OK) return fail(rc);
    mk_csr *G = F->G;
    if (hipMemcpyAsync(G->d_indptr, h.data(), pbytes, hipMemcpyHostToDevice, c.stream) != hipSuccess)
        return fail(mk_fail(MK_ERR_HIP, "%s: uploading the pattern failed", fn));
    if (pat_indptr) {
        if (F->nnz > 0 && hipMemcpyAsync(G->d_indices, pat_indices, sizeof(int32_t) * (size_t)F->nnz, hipMemcpyHostToDevice,
                                         c.stream) != hipSuccess)
            return fail(mk_fail(MK_ERR_HIP, "%s: uploading the pattern failed", fn));
    } else if (n > 0) {
        hipLaunchKernelGGL(mk_fsai_fill_kernel, dim3(mk_fsai_grid(n, MK_BLOCK)), dim3(MK_BLOCK), 0, c.stream, A->d_indptr,
                           A->d_indices, n, G->d_indptr, G->d_indices);
    }
    // the factor: one dense SPD solve per row
    if (n > 0 && longest <= MK_FSAI_SHORT) {
        hipLaunchKernelGGL(mk_fsai_setup_short, dim3(mk_fsai_grid(n, MK_BLOCK)), dim3(MK_BLOCK), 0, c.stream, A->d_indptr,
                           A->d_indices, A->d_data, G->d_indptr, G->d_indices, G->d_data, n, d_status);
    } else if (n > 0) {
        const int stride = mk_fsai_stride(longest);
        if (longest <= 16) {
            constexpr int GL = 8;
            hipLaunchKernelGGL(mk_fsai_setup_long<GL>, dim3(mk_fsai_grid(n, MK_BLOCK / GL)), dim3(MK_BLOCK),
                               sizeof(double) * (size_t)stride * (MK_BLOCK / GL), c.stream, A->d_indptr, A->d_indices, A->d_data,
                               G->d_indptr, G->d_indices, G->d_data, n, longest, stride, d_status);
        } else {
            constexpr int GL = 32;
            hipLaunchKernelGGL(mk_fsai_setup_long<GL>, dim3(mk_fsai_grid(n, MK_BLOCK / GL)), dim3(MK_BLOCK),
                               sizeof(double) * (size_t)stride * (MK_BLOCK / GL), c.stream, A->d_indptr, A->d_indices, A->d_data,
                               G->d_indptr, G->d_indices, G->d_data, n, longest, stride, d_status);
        }
    }
    // (the host arrays of the pattern are pageable: the copies above must be done before this call returns)
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, d_status, sizeof(int), hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
        hipStreamSynchronize(c.stream) != hipSuccess)
        return fail(mk_fail(MK_ERR_HIP, "%s: the set-up kernels failed", fn));
    hipFree(d_count);
    d_count = nullptr;
    if (bad != INT_MAX)
        return fail(mk_fail(MK_ERR_ARG, "%s: breakdown in row %d (a pivot of the Cholesky factor of A[P, P] is not positive, or "
                            "not finite): the matrix is not positive definite", fn, bad));
    rc = mk_csr_transpose(G, &F->Gt);
    if (rc != MK_OK) return fail(rc);
    F->bytes += 2 * (pbytes + (sizeof(int32_t) + sizeof(double)) * (size_t)(F->nnz + MK_CSR_PAD));
    F->setup_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    *out = F;
    return MK_OK;
}

extern "C" int mk_fsai_destroy(mk_fsai *F) {
    if (F) F->destroy();                                         // (while solvers still apply it: freed with the last of them)
    return MK_OK;
}

extern "C" int mk_fsai_apply(const mk_fsai *F, const double *in_dev, double *out_dev) {
    return MkDeviceOp::apply_standalone(F, in_dev, out_dev);
}

extern "C" int mk_fsai_info(const mk_fsai *F, int64_t *info, int32_t cap) {
    MK_ARG(F && (cap <= 0 || info));
    const int64_t v[MK_FSAI_INFO_LEN] = {F->n,
                                         F->nnz,
                                         F->longest,
                                         2,
                                         (int64_t)F->bytes,
                                         mk_csr_plan(F->G)->fmt,
                                         mk_csr_plan(F->Gt)->fmt,
                                         (int64_t)llround(F->setup_us)};
    for (int32_t k = 0; k < cap && k < MK_FSAI_INFO_LEN; ++k) info[k] = v[k];
    return MK_OK;
}

extern "C" int mk_fsai_download(const mk_fsai *F, int32_t *indptr_host, int32_t *indices_host, double *values_host) {
    MK_ARG(F);
    MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    if (indptr_host) MK_HIP(hipMemcpy(indptr_host, F->G->d_indptr, sizeof(int32_t) * (size_t)(F->n + 1), hipMemcpyDeviceToHost));
    if (indices_host && F->nnz > 0)
        MK_HIP(hipMemcpy(indices_host, F->G->d_indices, sizeof(int32_t) * (size_t)F->nnz, hipMemcpyDeviceToHost));
    if (values_host && F->nnz > 0)
        MK_HIP(hipMemcpy(values_host, F->G->d_data, sizeof(double) * (size_t)F->nnz, hipMemcpyDeviceToHost));
    return MK_OK;
}

extern "C" int mk_fsai_factors(const mk_fsai *F, mk_csr **G, mk_csr **Gt) {
    MK_ARG(F);
    if (G) *G = F->G;
    if (Gt) *Gt = F->Gt;
    return MK_OK;
}

extern "C" int mk_solver_set_precon_fsai(mk_solver *s, const mk_fsai *F) {
    return mk_set_precon(s, -1, MkPrecon::object(F), "mk_solver_set_precon_fsai");
}

extern "C" int mk_solver_set_lls_precon_fsai(mk_solver *s, int side, const mk_fsai *F) {
    return mk_set_precon(s, side, MkPrecon::object(F), "mk_solver_set_lls_precon_fsai");
}
