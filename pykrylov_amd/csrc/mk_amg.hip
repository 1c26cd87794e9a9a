// mk_amg.hip -- smoothed-aggregation algebraic multigrid of a symmetric device CSR matrix with a positive diagonal (the
// preconditioner `precon * r` of mk_solver_set_precon_amg): set-up on the device, one V(1,1)-cycle per apply.
//
// Per level (include/mikrylov.h, mk_amg_create, has the rules operation by operation):
//   diagonal, Gershgorin bound of D^-1 A          one lane per row, sums in stored order
//   strength, MIS(2) roots (Bell, Dalton, Olson)  64-bit keys {state, hash, index}; a round is two synchronous maximum
//                                                 propagations (buffer to buffer) and an update of the node's own key
//   aggregates                                    roots numbered by a device scan; two passes, each from its own buffer
//   P = T - (omega / lmax) D^-1 A T               expand per row, compress by the rule of mk_csr_from_coo
//   R = P',  A_next = R (A P)                     mk_csr_transpose; two expand-sort-compress products in row chunks
// The coarsest level is factored on the host (dense Cholesky, explicit inverse) and applied by one dense kernel.  Every
// floating-point result is ONE sequential sum in a documented order, formed by one lane: nothing depends on the grid, on the
// chunking of the products or on atomics (those are integer, or maxima of bit patterns).
//
// The cycle strings together what the library has: the level's smoother is an mk_cheb object, restriction and prolongation
// are products of R and P in whatever storage format their patterns earn, the residual and the coarse-grid correction are
// row epilogues (MkAmgEpi) of those products.
#include <chrono>
#include <climits>
#include <cmath>

#include "mk_solver.h"

constexpr int64_t MK_AMG_AUTO_CAP = (int64_t)1 << 26;   // entries of an expanded chunk when expand_cap = 0: 24 bytes each
                                                        // (row, column, value, and the sort's two index arrays) = 1.5 GiB

struct MkAmgLevel {
    const mk_csr *A = nullptr;            // level 0: borrowed (A->dependents counts the object); others: owned
    mk_csr *P = nullptr, *R = nullptr;    // owned; null on the last level
    mk_cheb *S = nullptr;                 // the smoother; null on a last level that is solved by its inverse
    int64_t n = 0, nnz = 0, nnz_p = 0, nagg = 0;
    int rounds = 0;
    int64_t expanded[3] = {0, 0, 0};      // entries of the lists of P, A P and R (A P)
    int chunks[3] = {0, 0, 0};
    double lmax = 0.0;
    int32_t *d_agg = nullptr;             // n ints; null on the last level
    double *d_x = nullptr, *d_r = nullptr, *d_b = nullptr;   // (d_b: levels >= 1)
};

struct mk_amg : MkDeviceOp {
    std::vector<MkAmgLevel> lev;
    int degree = 1;
    int coarse_kind = 0;                  // 1: the dense inverse; 0: the smoother alone
    int coarse_why = 0;                   // 0 -, 1 the last level is larger than coarse_max, 2 a pivot was not positive
    std::vector<double> h_ainv;           // row major
    double *d_ainv_t = nullptr;           // column major: lanes = rows read consecutive addresses
    double setup_us = 0.0;
    size_t bytes = 0;
    ~mk_amg() override;
    const char *noun() const override { return "AMG preconditioner"; }
    int enqueue(const double *in, double *out, hipStream_t stream, int *flags, int64_t *q) const override;
};

static inline unsigned amg_grid(int64_t items) {
    const int64_t g = (items + MK_BLOCK - 1) / MK_BLOCK;
    return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}
#define AMG_ROWS(r, n) for (int64_t r = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r < (n); r += (int64_t)gridDim.x * MK_BLOCK)

// ------------------------------------------------------------------ set-up kernels
__global__ void amg_words_init(unsigned long long *bound, int *status) {
    if (threadIdx.x == 0) {
        *bound = 0ull;
        status[0] = status[1] = INT_MAX;
    }
}

// diag[r] = the first stored a_rr; the Gershgorin bound of D^-1 A exactly as mk_cheb_bound_kernel forms it (the row added
// left to right in stored order, divided by |a_rr|, the maximum taken on the bit patterns); the smallest row whose diagonal
// entry is missing, not positive or not finite goes into *status
__global__ __launch_bounds__(MK_BLOCK) void amg_diag_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                           const double *__restrict__ data, int64_t n, double *__restrict__ diag,
                                                           unsigned long long *bound, int *status) {
    __shared__ unsigned long long smax;
    if (threadIdx.x == 0) smax = 0ull;
    __syncthreads();
    unsigned long long mb = 0ull;
    AMG_ROWS(r, n) {
        const int p1 = indptr[r + 1];
        double s = 0.0, arr = 0.0;
        bool have = false;
        for (int p = indptr[r]; p < p1; ++p) {
            const double a = data[p];
            s = s + fabs(a);
            if (!have && indices[p] == r) {
                arr = a;
                have = true;
            }
        }
        if (!have || !(arr > 0.0) || !isfinite(arr)) {
            atomicMin(status, (int)r);
            diag[r] = 1.0;
            continue;
        }
        diag[r] = arr;
        s = s / fabs(arr);
        const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(s));
        mb = b > mb ? b : mb;
    }
    atomicMax(&smax, mb);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(bound, smax);
}

// strong[p] for every stored entry and the start keys: state 1 (undecided), the hash, the index
__global__ __launch_bounds__(MK_BLOCK) void amg_strong_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                             const double *__restrict__ data, const double *__restrict__ diag,
                                                             int64_t n, double theta2, uint64_t seed, uint8_t *__restrict__ strong,
                                                             unsigned long long *__restrict__ key) {
    AMG_ROWS(i, n) {
        const int p1 = indptr[i + 1];
        const double ti = theta2 * diag[i];
        for (int p = indptr[i]; p < p1; ++p) {
            const int j = indices[p];
            const double v = data[p];
            strong[p] = (j != (int)i && v != 0.0 && v * v > ti * diag[j]) ? 1 : 0;
        }
        key[i] = (1ull << 62) | ((mk_cell_hash(i, seed) >> 34) << 32) | (unsigned long long)i;
    }
}

__global__ __launch_bounds__(MK_BLOCK) void amg_mis_max(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                       const uint8_t *__restrict__ strong, int64_t n,
                                                       const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out) {
    AMG_ROWS(i, n) {
        unsigned long long m = in[i];
        const int p1 = indptr[i + 1];
        for (int p = indptr[i]; p < p1; ++p)
            if (strong[p]) {
                const unsigned long long k = in[indices[p]];
                m = k > m ? k : m;
            }
        out[i] = m;
    }
}

// an undecided node whose distance-2 maximum is its own key goes in (state 2), one whose maximum is in goes out (state 0);
// *undecided counts what is left (integer adds, one per wave)
__global__ __launch_bounds__(MK_BLOCK) void amg_mis_update(int64_t n, unsigned long long *__restrict__ key,
                                                          const unsigned long long *__restrict__ m2, int *undecided) {
    const int64_t stride = (int64_t)gridDim.x * MK_BLOCK;
    for (int64_t base = (int64_t)blockIdx.x * MK_BLOCK; base < n; base += stride) {
        const int64_t i = base + threadIdx.x;
        bool left = false;
        if (i < n) {
            const unsigned long long k = key[i];
            if ((k >> 62) == 1ull) {
                const unsigned long long m = m2[i], body = k & ~(3ull << 62);
                if (m == k) key[i] = body | (2ull << 62);
                else if ((m >> 62) == 2ull) key[i] = body;
                else left = true;
            }
        }
        const unsigned long long votes = __ballot(left);
        if ((threadIdx.x & 63) == 0 && votes) atomicAdd(undecided, (int)__popcll(votes));
    }
}

__global__ __launch_bounds__(MK_BLOCK) void amg_root_flag(int64_t n, const unsigned long long *__restrict__ key, int32_t *__restrict__ flag) {
    AMG_ROWS(i, n) flag[i] = (key[i] >> 62) == 2ull ? 1 : 0;
}

// exclusive scan of n ints (out[n] = the total): sums of blocks of MK_BLOCK * 4 items, a sequential scan of those sums by one
// lane, and the scan inside every block.  Integers: the result does not depend on the order of the additions.
constexpr int AMG_SCAN_PER = 4;
__global__ __launch_bounds__(MK_BLOCK) void amg_scan_sums(const int32_t *__restrict__ in, int64_t n, int32_t *__restrict__ bsum) {
    __shared__ int32_t sh[MK_BLOCK];
    const int64_t i0 = ((int64_t)blockIdx.x * MK_BLOCK + threadIdx.x) * AMG_SCAN_PER;
    int32_t s = 0;
    for (int k = 0; k < AMG_SCAN_PER; ++k) s += (i0 + k < n) ? in[i0 + k] : 0;
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int off = MK_BLOCK / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = sh[0];
}
__global__ void amg_scan_top(int32_t *bsum, int nb) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int32_t run = 0;
        for (int b = 0; b < nb; ++b) {
            const int32_t v = bsum[b];
            bsum[b] = run;
            run += v;
        }
        bsum[nb] = run;
    }
}
__global__ __launch_bounds__(MK_BLOCK) void amg_scan_apply(const int32_t *__restrict__ in, int64_t n, const int32_t *__restrict__ bsum,
                                                          int nb, int32_t *__restrict__ out) {
    __shared__ int32_t sh[MK_BLOCK];
    const int t = (int)threadIdx.x;
    const int64_t i0 = ((int64_t)blockIdx.x * MK_BLOCK + t) * AMG_SCAN_PER;
    int32_t v[AMG_SCAN_PER], s = 0;
    for (int k = 0; k < AMG_SCAN_PER; ++k) {
        v[k] = (i0 + k < n) ? in[i0 + k] : 0;
        s += v[k];
    }
    sh[t] = s;
    __syncthreads();
    for (int off = 1; off < MK_BLOCK; off <<= 1) {       // inclusive scan of the lanes' sums
        const int32_t add = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    int32_t run = bsum[blockIdx.x] + sh[t] - s;
    for (int k = 0; k < AMG_SCAN_PER; ++k)
        if (i0 + k < n) {
            out[i0 + k] = run;
            run += v[k];
        }
    if (blockIdx.x == 0 && t == 0) out[n] = bsum[nb];
}

// pass 1: a root takes its own number, a node with strong root neighbours the root of the largest |a_ij| (the first in
// stored order on ties), anything else -1
__global__ __launch_bounds__(MK_BLOCK) void amg_agg_pass1(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                         const double *__restrict__ data, const uint8_t *__restrict__ strong,
                                                         const unsigned long long *__restrict__ key, const int32_t *__restrict__ rootnum,
                                                         int64_t n, int32_t *__restrict__ agg1) {
    AMG_ROWS(i, n) {
        int32_t best = -1;
        if ((key[i] >> 62) == 2ull) {
            best = rootnum[i];
        } else {
            double bv = -1.0;
            const int p1 = indptr[i + 1];
            for (int p = indptr[i]; p < p1; ++p)
                if (strong[p] && (key[indices[p]] >> 62) == 2ull) {
                    const double a = fabs(data[p]);
                    if (a > bv) {
                        bv = a;
                        best = rootnum[indices[p]];
                    }
                }
        }
        agg1[i] = best;
    }
}

// pass 2: what pass 1 left joins the aggregate of the strong neighbour that pass 1 assigned, by the same rule
__global__ __launch_bounds__(MK_BLOCK) void amg_agg_pass2(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                         const double *__restrict__ data, const uint8_t *__restrict__ strong,
                                                         const int32_t *__restrict__ agg1, int64_t n, int32_t *__restrict__ agg, int *status) {
    AMG_ROWS(i, n) {
        int32_t best = agg1[i];
        if (best < 0) {
            double bv = -1.0;
            const int p1 = indptr[i + 1];
            for (int p = indptr[i]; p < p1; ++p)
                if (strong[p] && agg1[indices[p]] >= 0) {
                    const double a = fabs(data[p]);
                    if (a > bv) {
                        bv = a;
                        best = agg1[indices[p]];
                    }
                }
            if (best < 0) {
                atomicMin(status, (int)i);
                best = 0;
            }
        }
        agg[i] = best;
    }
}

// entries of the expanded lists, per row
__global__ __launch_bounds__(MK_BLOCK) void amg_count_p(const int32_t *__restrict__ indptr, int64_t n, int32_t *__restrict__ count) {
    AMG_ROWS(i, n) count[i] = 1 + indptr[i + 1] - indptr[i];
}
__global__ __launch_bounds__(MK_BLOCK) void amg_count_prod(const int32_t *__restrict__ xp, const int32_t *__restrict__ xi,
                                                          const int32_t *__restrict__ yp, int64_t n, int32_t *__restrict__ count,
                                                          int *status) {
    AMG_ROWS(i, n) {
        long long c = 0;
        const int p1 = xp[i + 1];
        for (int p = xp[i]; p < p1; ++p) c += yp[xi[p] + 1] - yp[xi[p]];
        if (c > 2147483647LL) {
            atomicMin(status, (int)i);
            c = 0;
        }
        count[i] = (int32_t)c;
    }
}

// row i of P = T - (omega / lmax) D^-1 A T as a list: (agg(i), 1.0), then (agg(j), -((omega / lmax) (1.0 / a_ii)) a_ij) over
// the stored entries of row i in order.  Rows [r0, r1) into the chunk's arrays, row numbers relative to r0.
__global__ __launch_bounds__(MK_BLOCK) void amg_fill_p(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                      const double *__restrict__ data, const double *__restrict__ diag,
                                                      const int32_t *__restrict__ agg, double ow, int64_t r0, int64_t r1,
                                                      const int32_t *__restrict__ start, int32_t *__restrict__ rows,
                                                      int32_t *__restrict__ cols, double *__restrict__ vals) {
    AMG_ROWS(k, r1 - r0) {
        const int64_t i = r0 + k;
        int q = start[k];
        const double dinv = 1.0 / diag[i];
        const double c = -(ow * dinv);
        rows[q] = (int32_t)k;
        cols[q] = agg[i];
        vals[q] = 1.0;
        ++q;
        const int p1 = indptr[i + 1];
        for (int p = indptr[i]; p < p1; ++p, ++q) {
            rows[q] = (int32_t)k;
            cols[q] = agg[indices[p]];
            vals[q] = c * data[p];
        }
    }
}

// row i of X Y as a list: (j, x_ik y_kj) over the entries of row i of X in order and, within each, over row k of Y in order
__global__ __launch_bounds__(MK_BLOCK) void amg_fill_prod(const int32_t *__restrict__ xp, const int32_t *__restrict__ xi,
                                                         const double *__restrict__ xv, const int32_t *__restrict__ yp,
                                                         const int32_t *__restrict__ yi, const double *__restrict__ yv, int64_t r0,
                                                         int64_t r1, const int32_t *__restrict__ start, int32_t *__restrict__ rows,
                                                         int32_t *__restrict__ cols, double *__restrict__ vals) {
    AMG_ROWS(k, r1 - r0) {
        const int64_t i = r0 + k;
        int q = start[k];
        const int p1 = xp[i + 1];
        for (int p = xp[i]; p < p1; ++p) {
            const int kk = xi[p];
            const double x = xv[p];
            const int s1 = yp[kk + 1];
            for (int s = yp[kk]; s < s1; ++s, ++q) {
                rows[q] = (int32_t)k;
                cols[q] = yi[s];
                vals[q] = x * yv[s];
            }
        }
    }
}

__global__ __launch_bounds__(MK_BLOCK) void amg_shift_indptr(const int32_t *__restrict__ src, int64_t cnt, int32_t off, int32_t *__restrict__ dst) {
    AMG_ROWS(k, cnt) dst[k] = src[k] + off;
}

// ------------------------------------------------------------------ the cycle's kernels
// Row epilogue of the residual (y_r = b_r - s) and of the coarse-grid correction (y_r = b_r + s with b = y).  ONE type for
// both: every epilogue type instantiates mk_spmv_kernel once per storage format (mk_device.h, "Compile-time budget"); like
// MkChebEpi neither SYM_MARCH nor NO_MARCH -- level 0 is the solver's matrix and may be stored as a brick march.
struct MkAmgEpi {
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *b;
    double *y;
    int add;                    // launch uniform
    __device__ void prologue(double *) {}
    __device__ double xin(double v) const { return v; }
    __device__ __forceinline__ void step(int64_t r, double s, double br) { y[r] = add ? br + s : br - s; }
    __device__ void row(int64_t r, double s, double *) { step(r, s, b[r]); }
    // pipelined kernels (brick march): b[r] arrives as o[0], loaded at the top of the step
    static constexpr int NPF = 1;
    __device__ const double *pf_vec(int) const { return b; }
    __device__ void row_pf(int64_t r, double s, const double *o, double *) { step(r, s, o[0]); }
};

struct MkOpAmgAdd {             // out = a + b
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *a, *b;
    double *out;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 u = mk_ld2(a, i), v = mk_ld2(b, i);
        u.x = u.x + v.x;
        u.y = u.y + v.y;
        mk_st2(out, i, u);
    }
    __device__ void one(int64_t i, double *) { out[i] = a[i] + b[i]; }
};

// x = Ainv b on the coarsest level (n <= MK_AMG_MAX_COARSE), one workgroup: b goes to LDS first (b == x allowed), lane = row,
// the row summed left to right from 0.0
__global__ __launch_bounds__(MK_BLOCK) void amg_dense_kernel(const double *__restrict__ ainv_t, int n, const double *b, double *x,
                                                            MkHalt halt) {
    __shared__ double sb[MK_AMG_MAX_COARSE];
    const bool halted = halt.in();
    if (threadIdx.x == 0) halt.out(halted);
    if (halted) return;
    for (int c = threadIdx.x; c < n; c += MK_BLOCK) sb[c] = b[c];
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += MK_BLOCK) {
        double s = 0.0;
        for (int c = 0; c < n; ++c) s = s + ainv_t[(size_t)c * n + r] * sb[c];
        x[r] = s;
    }
}

// out = one V(1,1)-cycle on in (in == out allowed: `in` is read until the last launch, which alone writes `out`).  `q` = the
// solver's kernel counter (halt parity), or null for a standalone run.
int mk_amg::enqueue(const double *in, double *out, hipStream_t st, int *flags, int64_t *q) const {
    if (n == 0) return MK_OK;
    const auto next = [&] { return halt(flags, q); };
    double *const nopart = nullptr;
    const int L = (int)lev.size();
    const auto smooth = [&](const MkAmgLevel &v, const double *src, double *dst) {
        return mk_cheb_as_op(v.S)->enqueue(src, dst, st, flags, q);   // (q null: the smoother's own never-raised words)
    };
    const auto coarse = [&](const MkAmgLevel &v, const double *src, double *dst) {
        if (!coarse_kind) return smooth(v, src, dst);
        hipLaunchKernelGGL(amg_dense_kernel, dim3(1), dim3(MK_BLOCK), 0, st, d_ainv_t, (int)v.n, src, dst, next());
        return (int)MK_OK;
    };
    if (L == 1) {
        const int rc = coarse(lev[0], in, out);
        if (rc != MK_OK) return rc;
        MK_HIP(hipGetLastError());
        return MK_OK;
    }
    for (int l = 0; l + 1 < L; ++l) {                            // down: x = S b ; r = b - A x ; b_next = R r
        const MkAmgLevel &v = lev[(size_t)l];
        const double *b = l ? v.d_b : in;
        int rc = smooth(v, b, v.d_x);
        if (rc != MK_OK) return rc;
        mk_spmv_launch_blocks(v.A, mk_grid_spmv_for(v.A), st, v.d_x, MkAmgEpi{b, v.d_r, 0}, MkNoGate(), next, nopart);
        mk_spmv_launch_blocks(v.R, mk_grid_spmv_for(v.R), st, v.d_r, MkPlainEpi{lev[(size_t)l + 1].d_b}, MkNoGate(), next, nopart);
    }
    {
        const MkAmgLevel &v = lev[(size_t)L - 1];
        const int rc = coarse(v, v.d_b, v.d_x);
        if (rc != MK_OK) return rc;
    }
    for (int l = L - 2; l >= 0; --l) {                           // up: x += P e ; r = b - A x ; x = x + S r
        const MkAmgLevel &v = lev[(size_t)l];
        const double *b = l ? v.d_b : in;
        mk_spmv_launch_blocks(v.P, mk_grid_spmv_for(v.P), st, lev[(size_t)l + 1].d_x, MkAmgEpi{v.d_x, v.d_x, 1}, MkNoGate(), next, nopart);
        mk_spmv_launch_blocks(v.A, mk_grid_spmv_for(v.A), st, v.d_x, MkAmgEpi{b, v.d_r, 0}, MkNoGate(), next, nopart);
        const int rc = smooth(v, v.d_r, v.d_r);
        if (rc != MK_OK) return rc;
        hipLaunchKernelGGL(mk_stream_kernel<MkOpAmgAdd>, dim3(mk_grid_stream(v.n)), dim3(MK_BLOCK), 0, st,
                           MkOpAmgAdd{v.d_x, v.d_r, l ? v.d_x : out}, v.n, next(), nopart);
    }
    MK_HIP(hipGetLastError());
    return mk_ctx().pending_rc;
}

mk_amg::~mk_amg() {
    if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
    for (size_t l = 0; l < lev.size(); ++l) {
        MkAmgLevel &v = lev[l];
        if (v.S) mk_cheb_destroy(v.S);
        if (v.P) mk_csr_destroy(v.P);
        if (v.R) mk_csr_destroy(v.R);
        hipFree(v.d_agg);
        hipFree(v.d_x);
        hipFree(v.d_r);
        hipFree(v.d_b);
        if (v.A) {
            if (l == 0) mk_release_operand(v.A);
            else mk_csr_destroy(const_cast<mk_csr *>(v.A));
        }
    }
    hipFree(d_ainv_t);
}

// ------------------------------------------------------------------ set-up, host side
namespace {

struct AmgScratch {                       // device arrays of one coarsening step; freed when it goes out of scope
    std::vector<void *> ptrs;
    ~AmgScratch() {
        for (void *p : ptrs) hipFree(p);
    }
    template <class T>
    bool get(T **out, size_t count) {
        void *p = nullptr;
        if (hipMalloc(&p, sizeof(T) * (count ? count : 1)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        ptrs.push_back(p);
        *out = static_cast<T *>(p);
        return true;
    }
};

inline size_t amg_csr_bytes(int64_t nrows, int64_t nnz) {
    return sizeof(int32_t) * (size_t)(nrows + 1) + (sizeof(int32_t) + sizeof(double)) * (size_t)(nnz + MK_CSR_PAD);
}

// C = the compressed lists of the rows [0, nrows), `d_count[r]` entries each, written by `fill(r0, r1, d_start, rows, cols,
// vals)`: row chunks of at most `cap` entries (a longer row alone), every chunk compressed by mk_coo_compress_device and the
// chunks' CSR arrays put behind each other.  A row's result depends on its own list only: not on `cap`.
template <class Fill>
int amg_expand_compress(const char *fn, int64_t nrows, int64_t ncols, const int32_t *d_count, int64_t cap, const Fill &fill,
                        mk_csr **out, int64_t *expanded, int *chunks) {
    hipStream_t st = mk_ctx().stream;
    std::vector<int32_t> cnt((size_t)nrows + 1, 0);
    if (nrows > 0) MK_HIP(hipMemcpyAsync(cnt.data(), d_count, sizeof(int32_t) * (size_t)nrows, hipMemcpyDeviceToHost, st));
    MK_HIP(hipStreamSynchronize(st));
    std::vector<mk_csr *> parts;
    std::vector<int64_t> first;
    const auto drop = [&](int code) {
        for (mk_csr *p : parts) mk_csr_destroy(p);
        return code;
    };
    int64_t total = 0, nnz = 0;
    std::vector<int32_t> start;
    for (int64_t r0 = 0; r0 < nrows || parts.empty();) {
        int64_t r1 = r0, sum = 0;
        while (r1 < nrows && (r1 == r0 || sum + cnt[(size_t)r1] <= cap)) sum += cnt[(size_t)r1++];
        start.assign((size_t)(r1 - r0) + 1, 0);
        for (int64_t r = r0; r < r1; ++r) start[(size_t)(r - r0) + 1] = start[(size_t)(r - r0)] + cnt[(size_t)r];
        AmgScratch sc;
        int32_t *d_start = nullptr, *d_rows = nullptr, *d_cols = nullptr;
        double *d_vals = nullptr;
        if (!sc.get(&d_start, start.size()) || !sc.get(&d_rows, (size_t)sum) || !sc.get(&d_cols, (size_t)sum) || !sc.get(&d_vals, (size_t)sum))
            return drop(mk_fail(MK_ERR_HIP, "%s: out of device memory for an expanded chunk of %lld entries (lower expand_cap)", fn,
                                (long long)sum));
        if (hipMemcpyAsync(d_start, start.data(), sizeof(int32_t) * start.size(), hipMemcpyHostToDevice, st) != hipSuccess)
            return drop(mk_fail(MK_ERR_HIP, "%s: uploading the row starts of a chunk failed", fn));
        if (r1 > r0) fill(r0, r1, d_start, d_rows, d_cols, d_vals);
        mk_csr *part = nullptr;
        const int rc = mk_coo_compress_device(r1 - r0, ncols, sum, d_rows, d_cols, d_vals, start.data(), &part);
        if (rc != MK_OK) return drop(rc);
        parts.push_back(part);
        first.push_back(r0);
        total += sum;
        nnz += part->nnz;
        r0 = r1;
        if (nrows == 0) break;
    }
    *expanded = total;
    *chunks = (int)parts.size();
    if (parts.size() == 1) {
        *out = parts[0];
        return MK_OK;
    }
    if (nnz > 2147483647LL) return drop(mk_fail(MK_ERR_UNSUPPORTED, "%s: a level with %lld nonzeros exceeds the int32 index range", fn, (long long)nnz));
    mk_csr *C = nullptr;
    int rc = mk_csr_alloc(nrows, ncols, nnz, &C);
    if (rc != MK_OK) return drop(rc);
    int64_t off = 0;
    for (size_t k = 0; k < parts.size(); ++k) {
        const mk_csr *p = parts[k];
        const int64_t rows_k = p->nrows + (k + 1 == parts.size() ? 1 : 0);
        hipLaunchKernelGGL(amg_shift_indptr, dim3(amg_grid(rows_k)), dim3(MK_BLOCK), 0, st, p->d_indptr, rows_k, (int32_t)off,
                           C->d_indptr + first[k]);
        if (p->nnz > 0 &&
            (hipMemcpyAsync(C->d_indices + off, p->d_indices, sizeof(int32_t) * (size_t)p->nnz, hipMemcpyDeviceToDevice, st) != hipSuccess ||
             hipMemcpyAsync(C->d_data + off, p->d_data, sizeof(double) * (size_t)p->nnz, hipMemcpyDeviceToDevice, st) != hipSuccess)) {
            mk_csr_destroy(C);
            return drop(mk_fail(MK_ERR_HIP, "%s: joining the chunks failed", fn));
        }
        off += p->nnz;
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        mk_csr_destroy(C);
        return drop(mk_fail(MK_ERR_HIP, "%s: joining the chunks failed", fn));
    }
    drop(0);
    *out = C;
    return MK_OK;
}

int amg_product(const char *fn, const mk_csr *X, const mk_csr *Y, int64_t cap, int *d_status, mk_csr **out, int64_t *expanded,
                int *chunks) {
    hipStream_t st = mk_ctx().stream;
    AmgScratch sc;
    int32_t *d_count = nullptr;
    if (!sc.get(&d_count, (size_t)X->nrows)) return mk_fail(MK_ERR_HIP, "%s: out of device memory for the row counts", fn);
    if (X->nrows > 0)
        hipLaunchKernelGGL(amg_count_prod, dim3(amg_grid(X->nrows)), dim3(MK_BLOCK), 0, st, X->d_indptr, X->d_indices, Y->d_indptr,
                           X->nrows, d_count, d_status);
    int bad = INT_MAX;
    MK_HIP(hipMemcpyAsync(&bad, d_status, sizeof(int), hipMemcpyDeviceToHost, st));
    MK_HIP(hipStreamSynchronize(st));
    if (bad != INT_MAX)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: row %d of a Galerkin product expands to 2^31 entries or more", fn, bad);
    const auto fill = [&](int64_t r0, int64_t r1, const int32_t *d_start, int32_t *rows, int32_t *cols, double *vals) {
        hipLaunchKernelGGL(amg_fill_prod, dim3(amg_grid(r1 - r0)), dim3(MK_BLOCK), 0, st, X->d_indptr, X->d_indices, X->d_data,
                           Y->d_indptr, Y->d_indices, Y->d_data, r0, r1, d_start, rows, cols, vals);
    };
    return amg_expand_compress(fn, X->nrows, Y->ncols, d_count, cap, fill, out, expanded, chunks);
}

// the explicit inverse of the dense SPD matrix S (row major, overwritten) by the Cholesky recurrence of the FSAI block:
// false if a pivot is not positive and finite
bool amg_dense_inverse(int n, std::vector<double> &S, std::vector<double> &inv) {
    const size_t N = (size_t)n;
    std::vector<double> &Lm = S;                                 // the lower triangle becomes L
    for (size_t b = 0; b < N; ++b) {
        double d = Lm[b * N + b];
        for (size_t k = 0; k < b; ++k) d = d - Lm[b * N + k] * Lm[b * N + k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double ld = std::sqrt(d);
        Lm[b * N + b] = ld;
        for (size_t a = b + 1; a < N; ++a) {
            double s = Lm[a * N + b];
            for (size_t k = 0; k < b; ++k) s = s - Lm[a * N + k] * Lm[b * N + k];
            Lm[a * N + b] = s / ld;
        }
    }
    std::vector<double> Lt(N * N, 0.0), y(N), x(N);
    for (size_t a = 0; a < N; ++a)
        for (size_t k = 0; k <= a; ++k) Lt[k * N + a] = Lm[a * N + k];
    inv.assign(N * N, 0.0);
    for (size_t c = 0; c < N; ++c) {
        for (size_t a = 0; a < N; ++a) {                         // L y = e_c
            double s = a == c ? 1.0 : 0.0;
            for (size_t k = 0; k < a; ++k) s = s - Lm[a * N + k] * y[k];
            y[a] = s / Lm[a * N + a];
        }
        for (size_t a = N; a-- > 0;) {                           // L' x = y
            double s = y[a];
            for (size_t k = N; k-- > a + 1;) s = s - Lt[a * N + k] * x[k];
            x[a] = s / Lm[a * N + a];
        }
        for (size_t a = 0; a < N; ++a) inv[a * N + c] = x[a];
    }
    return true;
}

}   // namespace

// ======================================================================================
// C ABI
// ======================================================================================
extern "C" int mk_amg_create(const mk_csr *A, double theta, int32_t degree, double ratio, double omega, int32_t coarse_max,
                             int32_t max_levels, uint64_t seed, int64_t expand_cap, mk_amg **out) {
    MK_REQUIRE_INIT();
    MK_ARG(A && out);
    const char *fn = "mk_amg_create";
    if (A->comp_kind || A->host_fn || A->alias || A->nops)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator holds no CSR arrays of its own (a composite, reduced, block, "
                       "composed or matrix-free operator): form its matrix with to_csr_arrays() and a CsrOperator", fn);
    if (A->ex.mode >= 0 || A->row_block)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator is row-partitioned (it carries an exchange plan); the AMG "
                       "preconditioner is single-GPU", fn);
    if (A->nrows != A->ncols)
        return mk_fail(MK_ERR_ARG, "%s: the matrix must be square, got %lld x %lld", fn, (long long)A->nrows, (long long)A->ncols);
    if (A->nrows >= ((int64_t)1 << 31) - 1)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: %lld rows; a key names a row in 32 bits (< 2^31 - 1)", fn, (long long)A->nrows);
    if (!(theta >= 0.0) || !std::isfinite(theta)) return mk_fail(MK_ERR_ARG, "%s: theta = %g must be finite and >= 0", fn, theta);
    if (degree < 1 || degree > MK_CHEB_MAX_DEGREE) return mk_fail(MK_ERR_ARG, "%s: degree %d is outside 1 .. %d", fn, (int)degree, MK_CHEB_MAX_DEGREE);
    if (!(ratio > 1.0) || !std::isfinite(ratio)) return mk_fail(MK_ERR_ARG, "%s: ratio = %g must be finite and > 1", fn, ratio);
    if (!(omega > 0.0) || !std::isfinite(omega)) return mk_fail(MK_ERR_ARG, "%s: omega = %g must be finite and > 0", fn, omega);
    if (coarse_max < 1 || coarse_max > MK_AMG_MAX_COARSE)
        return mk_fail(MK_ERR_ARG, "%s: coarse_max %d is outside 1 .. %d", fn, (int)coarse_max, MK_AMG_MAX_COARSE);
    if (max_levels < 1 || max_levels > MK_AMG_MAX_LEVELS)
        return mk_fail(MK_ERR_ARG, "%s: max_levels %d is outside 1 .. %d", fn, (int)max_levels, MK_AMG_MAX_LEVELS);
    if (expand_cap < 0 || expand_cap > 2147483647LL)
        return mk_fail(MK_ERR_ARG, "%s: expand_cap %lld is outside 0 .. 2^31 - 1", fn, (long long)expand_cap);
    if (A->nnz > 0 && (!A->d_indices || !A->d_data)) return mk_fail(MK_ERR_STATE, "%s: the CSR arrays of this matrix were released", fn);
    const auto t0 = std::chrono::steady_clock::now();
    MkContext &c = mk_ctx();
    hipStream_t st = c.stream;
    const int64_t cap = expand_cap > 0 ? expand_cap : MK_AMG_AUTO_CAP;
    mk_amg *F = new mk_amg();
    F->n = A->nrows;
    F->degree = degree;
    const auto fail = [&](int code) {
        delete F;
        return code;
    };
    unsigned long long *d_bound = nullptr;                       // bits of the Gershgorin bound, then two status words
    AmgScratch top;
    if (!top.get(&d_bound, 2)) {
        (void)hipGetLastError();
        return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory", fn));
    }
    const int rc0 = F->init_nohalt(st);
    if (rc0 != MK_OK) return fail(rc0);
    F->bytes += 2 * sizeof(int);                                 // (the two halt words)
    int *const d_status = reinterpret_cast<int *>(d_bound + 1);
    F->lev.emplace_back();
    F->lev[0].A = A;
    A->dependents += 1;
    const double theta2 = theta * theta;
    for (int l = 0;; ++l) {
        const mk_csr *Al = F->lev[(size_t)l].A;
        const int64_t n = Al->nrows;
        F->lev[(size_t)l].n = n;
        F->lev[(size_t)l].nnz = Al->nnz;
        // the level's vectors (16 bytes of slack behind each, zeroed: the product kernels read their input in 16-byte pairs)
        const size_t vbytes = sizeof(double) * (size_t)(n > 0 ? n : 1) + 16;
        double **vecs[3] = {&F->lev[(size_t)l].d_x, &F->lev[(size_t)l].d_r, &F->lev[(size_t)l].d_b};
        for (int k = 0; k < (l ? 3 : 2); ++k) {
            if (hipMalloc((void **)vecs[k], vbytes) != hipSuccess || hipMemsetAsync(*vecs[k], 0, vbytes, st) != hipSuccess) {
                (void)hipGetLastError();
                return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory for the vectors of level %d (%zu bytes each)", fn, l, vbytes));
            }
            F->bytes += vbytes;
        }
        if (l) F->bytes += amg_csr_bytes(n, Al->nnz);
        // 1. diagonal and bound
        AmgScratch sc;
        double *d_diag = nullptr;
        if (!sc.get(&d_diag, (size_t)n)) return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory on level %d", fn, l));
        hipLaunchKernelGGL(amg_words_init, dim3(1), dim3(64), 0, st, d_bound, d_status);
        if (n > 0)
            hipLaunchKernelGGL(amg_diag_kernel, dim3((unsigned)(amg_grid(n) < 1024 ? amg_grid(n) : 1024)), dim3(MK_BLOCK), 0, st,
                               Al->d_indptr, Al->d_indices, Al->d_data, n, d_diag, d_bound, d_status);
        unsigned long long hb[2] = {0ull, 0ull};
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hb, d_bound, sizeof(hb), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(mk_fail(MK_ERR_HIP, "%s: the set-up kernels of level %d failed", fn, l));
        int bad = INT_MAX;
        memcpy(&bad, &hb[1], sizeof(int));
        if (bad != INT_MAX)
            return fail(mk_fail(MK_ERR_ARG, "%s: row %d of level %d has no positive diagonal entry (none is stored, or one that is "
                                "zero, negative or not finite)", fn, bad, l));
        double lmax = 0.0;
        memcpy(&lmax, &hb[0], sizeof(double));
        if (n > 0 && !(std::isfinite(lmax) && lmax > 0.0))
            return fail(mk_fail(MK_ERR_ARG, "%s: the Gershgorin bound of level %d is %g", fn, l, lmax));
        F->lev[(size_t)l].lmax = lmax;
        // 7. stopping
        bool last = n <= coarse_max || l + 1 >= max_levels;
        int32_t *d_agg = nullptr;
        int64_t nagg = 0;
        if (!last) {
            // 2. strength, 3. MIS(2) roots
            uint8_t *d_strong = nullptr;
            unsigned long long *d_key = nullptr, *d_m1 = nullptr, *d_m2 = nullptr;
            int32_t *d_flag = nullptr, *d_num = nullptr, *d_bsum = nullptr, *d_agg1 = nullptr;
            int *d_und = nullptr;
            const int nb = (int)((n + MK_BLOCK * AMG_SCAN_PER - 1) / (MK_BLOCK * AMG_SCAN_PER));
            if (!sc.get(&d_strong, (size_t)Al->nnz) || !sc.get(&d_key, (size_t)n) || !sc.get(&d_m1, (size_t)n) || !sc.get(&d_m2, (size_t)n) ||
                !sc.get(&d_flag, (size_t)n) || !sc.get(&d_num, (size_t)n + 1) || !sc.get(&d_bsum, (size_t)nb + 1) ||
                !sc.get(&d_agg1, (size_t)n) || !sc.get(&d_und, 1) || hipMalloc((void **)&d_agg, sizeof(int32_t) * (size_t)n) != hipSuccess) {
                (void)hipGetLastError();
                return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory for the aggregation of level %d", fn, l));
            }
            F->lev[(size_t)l].d_agg = d_agg;
            F->bytes += sizeof(int32_t) * (size_t)n;
            const unsigned g = amg_grid(n);
            hipLaunchKernelGGL(amg_strong_kernel, dim3(g), dim3(MK_BLOCK), 0, st, Al->d_indptr, Al->d_indices, Al->d_data, d_diag, n,
                               theta2, seed, d_strong, d_key);
            int rounds = 0;
            for (int und = 1; und > 0;) {
                hipMemsetAsync(d_und, 0, sizeof(int), st);
                hipLaunchKernelGGL(amg_mis_max, dim3(g), dim3(MK_BLOCK), 0, st, Al->d_indptr, Al->d_indices, d_strong, n, d_key, d_m1);
                hipLaunchKernelGGL(amg_mis_max, dim3(g), dim3(MK_BLOCK), 0, st, Al->d_indptr, Al->d_indices, d_strong, n, d_m1, d_m2);
                hipLaunchKernelGGL(amg_mis_update, dim3(g), dim3(MK_BLOCK), 0, st, n, d_key, d_m2, d_und);
                if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&und, d_und, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess)
                    return fail(mk_fail(MK_ERR_HIP, "%s: the MIS(2) kernels of level %d failed", fn, l));
                ++rounds;
                if (rounds > 100000) return fail(mk_fail(MK_ERR_STATE, "%s: MIS(2) on level %d did not finish", fn, l));
            }
            F->lev[(size_t)l].rounds = rounds;
            // 4. aggregates
            hipLaunchKernelGGL(amg_root_flag, dim3(g), dim3(MK_BLOCK), 0, st, n, d_key, d_flag);
            hipLaunchKernelGGL(amg_scan_sums, dim3(nb), dim3(MK_BLOCK), 0, st, d_flag, n, d_bsum);
            hipLaunchKernelGGL(amg_scan_top, dim3(1), dim3(64), 0, st, d_bsum, nb);
            hipLaunchKernelGGL(amg_scan_apply, dim3(nb), dim3(MK_BLOCK), 0, st, d_flag, n, d_bsum, nb, d_num);
            hipLaunchKernelGGL(amg_agg_pass1, dim3(g), dim3(MK_BLOCK), 0, st, Al->d_indptr, Al->d_indices, Al->d_data, d_strong, d_key,
                               d_num, n, d_agg1);
            hipLaunchKernelGGL(amg_agg_pass2, dim3(g), dim3(MK_BLOCK), 0, st, Al->d_indptr, Al->d_indices, Al->d_data, d_strong, d_agg1, n,
                               d_agg, d_status + 1);
            int32_t roots = 0;
            int lost = INT_MAX;
            if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&roots, d_num + n, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipMemcpyAsync(&lost, d_status + 1, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                return fail(mk_fail(MK_ERR_HIP, "%s: the aggregation kernels of level %d failed", fn, l));
            if (lost != INT_MAX)
                return fail(mk_fail(MK_ERR_ARG, "%s: row %d of level %d found no aggregate within two strong edges: the matrix is not "
                                    "symmetric", fn, lost, l));
            nagg = roots;
            F->lev[(size_t)l].nagg = nagg;
            if (nagg >= n) last = true;                          // the level does not shrink
        }
        if (last) break;
        // 5. prolongator
        MkAmgLevel &v = F->lev[(size_t)l];
        {
            int32_t *d_count = nullptr;
            if (!sc.get(&d_count, (size_t)n)) return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory on level %d", fn, l));
            hipLaunchKernelGGL(amg_count_p, dim3(amg_grid(n)), dim3(MK_BLOCK), 0, st, Al->d_indptr, n, d_count);
            const double ow = omega / lmax;
            const auto fill = [&](int64_t r0, int64_t r1, const int32_t *d_start, int32_t *rows, int32_t *cols, double *vals) {
                hipLaunchKernelGGL(amg_fill_p, dim3(amg_grid(r1 - r0)), dim3(MK_BLOCK), 0, st, Al->d_indptr, Al->d_indices, Al->d_data,
                                   d_diag, d_agg, ow, r0, r1, d_start, rows, cols, vals);
            };
            int rc = amg_expand_compress(fn, n, nagg, d_count, cap, fill, &v.P, &v.expanded[0], &v.chunks[0]);
            if (rc != MK_OK) return fail(rc);
            rc = mk_csr_transpose(v.P, &v.R);
            if (rc != MK_OK) return fail(rc);
        }
        v.nnz_p = v.P->nnz;
        F->bytes += 2 * amg_csr_bytes(n, v.nnz_p);
        // 6. Galerkin product
        mk_csr *AP = nullptr, *Anext = nullptr;
        int rc = amg_product(fn, Al, v.P, cap, d_status, &AP, &v.expanded[1], &v.chunks[1]);
        if (rc != MK_OK) return fail(rc);
        rc = amg_product(fn, v.R, AP, cap, d_status, &Anext, &v.expanded[2], &v.chunks[2]);
        mk_csr_destroy(AP);
        if (rc != MK_OK) return fail(rc);
        // the smoother of this level (the last level's is made below, if it needs one)
        rc = mk_cheb_create(Al, degree, lmax / ratio, lmax, 1, &v.S);
        if (rc != MK_OK) {
            mk_csr_destroy(Anext);
            return fail(rc);
        }
        F->lev.emplace_back();
        F->lev.back().A = Anext;
    }
    // 8. the coarsest level
    MkAmgLevel &v = F->lev.back();
    const int64_t nc = v.n;
    F->coarse_kind = 0;
    F->coarse_why = nc > coarse_max ? 1 : 0;
    if (nc <= coarse_max && nc > 0) {
        std::vector<int32_t> ip((size_t)nc + 1), ix((size_t)v.nnz);
        std::vector<double> dv((size_t)v.nnz), S((size_t)nc * (size_t)nc, 0.0);
        if (hipMemcpy(ip.data(), v.A->d_indptr, sizeof(int32_t) * ip.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            (v.nnz > 0 && (hipMemcpy(ix.data(), v.A->d_indices, sizeof(int32_t) * ix.size(), hipMemcpyDeviceToHost) != hipSuccess ||
                           hipMemcpy(dv.data(), v.A->d_data, sizeof(double) * dv.size(), hipMemcpyDeviceToHost) != hipSuccess)))
            return fail(mk_fail(MK_ERR_HIP, "%s: downloading the coarsest level failed", fn));
        for (int64_t r = 0; r < nc; ++r)
            for (int32_t p = ip[(size_t)r]; p < ip[(size_t)r + 1]; ++p) S[(size_t)r * (size_t)nc + (size_t)ix[(size_t)p]] = dv[(size_t)p];
        if (amg_dense_inverse((int)nc, S, F->h_ainv)) {
            std::vector<double> t((size_t)nc * (size_t)nc);
            for (int64_t r = 0; r < nc; ++r)
                for (int64_t cc = 0; cc < nc; ++cc) t[(size_t)cc * (size_t)nc + (size_t)r] = F->h_ainv[(size_t)r * (size_t)nc + (size_t)cc];
            if (hipMalloc((void **)&F->d_ainv_t, sizeof(double) * t.size()) != hipSuccess ||
                hipMemcpy(F->d_ainv_t, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipGetLastError();
                return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory for the coarse inverse", fn));
            }
            F->bytes += sizeof(double) * t.size();
            F->coarse_kind = 1;
        } else {
            F->h_ainv.clear();
            F->coarse_why = 2;
        }
    }
    if (!F->coarse_kind && nc > 0) {
        const int rc = mk_cheb_create(v.A, degree, v.lmax / ratio, v.lmax, 1, &v.S);
        if (rc != MK_OK) return fail(rc);
    }
    for (const MkAmgLevel &w : F->lev)
        if (w.S) {
            int64_t ci[MK_CHEB_INFO_LEN] = {0};
            mk_cheb_info(w.S, ci, MK_CHEB_INFO_LEN);
            F->bytes += (size_t)ci[4];
        }
    F->setup_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    *out = F;
    return MK_OK;
}

extern "C" int mk_amg_destroy(mk_amg *F) {
    if (F) F->destroy();                                         // (while solvers still apply it: freed with the last of them)
    return MK_OK;
}

extern "C" int mk_amg_apply(const mk_amg *F, const double *in_dev, double *out_dev) {
    return MkDeviceOp::apply_standalone(F, in_dev, out_dev);
}

extern "C" int mk_amg_info(const mk_amg *F, int32_t level, int64_t *info, int32_t cap) {
    MK_ARG(F && (cap <= 0 || info) && level >= -1 && level < (int32_t)F->lev.size());
    int64_t v[MK_AMG_INFO_LEN] = {0};
    const int64_t L = (int64_t)F->lev.size();
    if (level < 0) {
        int64_t rows = 0, nnz = 0;
        for (const MkAmgLevel &w : F->lev) {
            rows += w.n;
            nnz += w.nnz;
        }
        v[0] = L;
        v[1] = (int64_t)F->bytes;
        v[2] = (int64_t)llround(F->setup_us);
        v[3] = (L - 1) * (7 + 2 * (int64_t)F->degree) + (F->coarse_kind ? 1 : 1 + (int64_t)F->degree);
        v[4] = F->coarse_kind;
        v[5] = F->lev[0].nnz > 0 ? (1000 * nnz + F->lev[0].nnz / 2) / F->lev[0].nnz : 0;
        v[6] = F->lev[0].n > 0 ? (1000 * rows + F->lev[0].n / 2) / F->lev[0].n : 0;
        v[7] = nnz;
        v[8] = rows;
        v[9] = F->coarse_why;
    } else {
        const MkAmgLevel &w = F->lev[(size_t)level];
        v[0] = w.n;
        v[1] = w.nnz;
        v[2] = w.nnz_p;
        v[3] = w.nagg;
        v[4] = w.rounds;
        v[5] = w.expanded[1];
        v[6] = w.expanded[2];
        v[7] = w.chunks[1];
        v[8] = w.chunks[2];
        v[9] = w.chunks[0];
    }
    for (int32_t k = 0; k < cap && k < MK_AMG_INFO_LEN; ++k) info[k] = v[k];
    return MK_OK;
}

extern "C" int mk_amg_level(const mk_amg *F, int32_t level, int32_t which, mk_csr **borrowed) {
    MK_ARG(F && borrowed && level >= 0 && level < (int32_t)F->lev.size() && which >= 0 && which <= 2);
    const MkAmgLevel &w = F->lev[(size_t)level];
    *borrowed = which == 0 ? const_cast<mk_csr *>(w.A) : (which == 1 ? w.P : w.R);
    if (!*borrowed) return mk_fail(MK_ERR_ARG, "mk_amg_level: the last level (%d) has no P and no R", (int)level);
    return MK_OK;
}

extern "C" int mk_amg_download(const mk_amg *F, int32_t level, int32_t *agg_host, double *lmax_host) {
    MK_ARG(F && level >= 0 && level < (int32_t)F->lev.size());
    const MkAmgLevel &w = F->lev[(size_t)level];
    if (lmax_host) *lmax_host = w.lmax;
    if (agg_host) {
        if (!w.P) return mk_fail(MK_ERR_ARG, "mk_amg_download: the last level (%d) has no aggregates", (int)level);
        MK_HIP(hipStreamSynchronize(mk_ctx().stream));
        if (w.n > 0) MK_HIP(hipMemcpy(agg_host, w.d_agg, sizeof(int32_t) * (size_t)w.n, hipMemcpyDeviceToHost));
    }
    return MK_OK;
}

extern "C" int mk_amg_coarse(const mk_amg *F, double *inverse_host) {
    MK_ARG(F && inverse_host);
    if (!F->coarse_kind) return mk_fail(MK_ERR_STATE, "mk_amg_coarse: the coarsest level is solved by its smoother alone (mk_amg_info)");
    memcpy(inverse_host, F->h_ainv.data(), sizeof(double) * F->h_ainv.size());
    return MK_OK;
}

extern "C" int mk_solver_set_precon_amg(mk_solver *s, const mk_amg *F) {
    return mk_set_precon(s, -1, MkPrecon::object(F), "mk_solver_set_precon_amg");
}

extern "C" int mk_solver_set_lls_precon_amg(mk_solver *s, int side, const mk_amg *F) {
    return mk_set_precon(s, side, MkPrecon::object(F), "mk_solver_set_lls_precon_amg");
}
