// mk_lanczos.hip -- k steps of the symmetric Lanczos process on a device CSR matrix (mk_csr_lanczos): the tridiagonal
// T_k = tridiag(beta_j, alpha_j, beta_{j+1}) whose extreme eigenvalues give the Chebyshev preconditioner (mk_cheb.hip) an
// interval from the matrix instead of Gershgorin / 30.
//
// The recurrence is the one MINRES runs in its kernels K1 and K2 (mk_minres.hip), without a shift and without keeping v;
// with scale_diag the diagonally preconditioned form, which is Lanczos on D^-1/2 A D^-1/2 (D = diag(A) > 0).  No
// reorthogonalisation: the extreme Ritz values do not need it.
//
//   start     r2 = start (or the hashed vector mk_cell_field(i, seed) - 1.0);  y = r2 (dinv * r2);  beta_1 = sqrt<r2, y>
//   L1(j)     beta_j = sqrt(total) -- stop tests -- s = 1 / beta_j;  v = s y on the fly;  t = A v  (j > 1: t = t -
//             (beta_j / beta_{j-1}) r1);  partial <v, t>                                       [product, in A's format]
//   L2(j)     alpha_j = total;  ynew = (-alpha_j / beta_j) r2 + t, written over r1 (the pointers rotate);  scaled:
//             y = dinv ynew;  partial <ynew, y>                                                 [stream]
//   final     beta_{m+1} = sqrt(total)
//
// Two launches per step plus two (three when scaled: 1 / a_rr first).  A step moves the matrix plus 56 n bytes (L1: r1
// and the product's input in, t out; L2: r2 and t in, ynew out), 72 n when scaled (dinv in, y out).  The scalars stay in
// device memory until one download at the end; the host only enqueues.  The run stops on the device (MkHalt: launches
// after the stop do nothing) after step j when beta_{j+1} is not > 2^-26 max_{i<=j}(|alpha_i| + [i>1] beta_i) -- every
// Ritz value is then an eigenvalue to sqrt(eps) relative accuracy; this is what exact breakdown looks like -- or when a
// scalar is not finite.  Every operation rounds on its own (-ffp-contract=off) in the order written above; the two dots
// have the trees of every fused product dot and every stream dot of the library.
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "mk_solver.h"

namespace {

enum { SLOT_ALFA = 0, SLOT_YY = 1, NSLOT = 2 };

struct LzStatus {               // device memory, zeroed before the run, written by one lane (bad: atomicMax)
    int64_t done;               // steps completed
    int64_t nonfinite;          // step whose alpha or beta_{j+1} is not finite (0: none)
    int32_t bad;                // scaled: n - r of the smallest row r without a positive diagonal entry (0: none)
    int32_t halt[2];            // the parity halt words
    int32_t pad;
};

// the scalar file behind the status record: alpha_1..m, beta_1..m+1, tmax_0..m (tmax_j = max_{i<=j}(|alpha_i| + [i>1] beta_i))
struct LzScal {
    double *alpha, *beta, *tmax;
};

// scaled: dinv[r] = 1 / a_rr, the first stored diagonal entry of the row; a row without one, or with one that is not
// positive, goes into the status record and raises the halt word of the next launch (this is launch 0: it reads none)
__global__ __launch_bounds__(MK_BLOCK) void lz_dinv_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                          const double *__restrict__ data, int64_t n, double *__restrict__ dinv,
                                                          LzStatus *st) {
    for (int64_t r = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * MK_BLOCK) {
        double arr = 0.0;
        const int p1 = indptr[r + 1];
        for (int p = indptr[r]; p < p1; ++p) {
            if (indices[p] == r) {
                arr = data[p];
                break;
            }
        }
        if (!(arr > 0.0)) {
            atomicMax(&st->bad, (int)(n - r));
            st->halt[1] = 1;
            continue;
        }
        dinv[r] = 1.0 / arr;
    }
}

struct LzOpStart {              // r2 = start (hash) ; y = dinv * r2 ; partial <r2, y>
    static constexpr int NACC = 1, SLOT0 = SLOT_YY;
    const double *start, *dinv;
    double *r2, *y;
    uint64_t seed;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void elem(int64_t i, double rv, double *acc) {
        r2[i] = rv;
        double yv = rv;
        if (dinv) {
            yv = dinv[i] * rv;
            y[i] = yv;
        }
        acc[0] += rv * yv;
    }
    __device__ void pair(int64_t i, double *acc) {
        elem(i, start ? start[i] : mk_cell_field(i, seed) - 1.0, acc);
        elem(i + 1, start ? start[i + 1] : mk_cell_field(i + 1, seed) - 1.0, acc);
    }
    __device__ void one(int64_t i, double *acc) { elem(i, start ? start[i] : mk_cell_field(i, seed) - 1.0, acc); }
};

// beta_j from the partials of L2(j-1) (the start kernel's for j = 1) and the stop tests on it
struct LzGate {
    const double *part;
    int np;
    LzScal sc;
    LzStatus *st;
    int j;                      // step, 1-based
    __device__ bool open(double *s4, bool lead, bool *stop) {
        const double b = __dsqrt_rn(mk_total(part + SLOT_YY * MK_MAXP, np, s4));
        const bool finite = isfinite(b);
        const bool go = (j == 1) ? (finite && b > 0.0) : (finite && b > 0x1.0p-26 * sc.tmax[j - 1]);
        if (lead) sc.beta[j - 1] = b;
        if (!go) {
            if (lead) {
                st->done = j - 1;
                if (!finite) st->nonfinite = j > 1 ? j - 1 : 0;
            }
            *stop = true;
        }
        return go;
    }
};

// Row epilogue of L1.  ONE type for every step: `first` and `nt` are launch-uniform run-time fields, because every epilogue
// type instantiates mk_spmv_kernel once per storage format (mk_device.h, "Compile-time budget").  Neither SYM_MARCH nor
// NO_MARCH, for MkChebEpi's reasons (mk_cheb.hip): on formats 9 and 10 the step runs as the pipelined march kernel with
// r1[r] prefetched, on format 11 as the CSR gather kernel on the same arrays.
struct LzEpi {
    static constexpr int NACC = 1, SLOT0 = SLOT_ALFA;
    const double *part;
    int np;
    const double *bprev;        // beta_{j-1} (not read in the first step)
    const double *y, *r1;       // y: the product's input (r2, or dinv * r2)
    double *t;
    int first;                  // j == 1: no r1 term
    int nt;                     // t goes past the caches (vectors beyond the Infinity Cache; mk_store_stream)
    double s, c;
    __device__ void prologue(double *s4) {
        const double b = __dsqrt_rn(mk_total(part + SLOT_YY * MK_MAXP, np, s4));
        s = 1.0 / b;
        c = first ? 0.0 : b / bprev[0];
    }
    __device__ double xin(double yj) const { return s * yj; }
    __device__ __forceinline__ void step(int64_t i, double sum, double vv, double r1v, double *acc) {
        double tv = sum;
        if (!first) tv = tv - c * r1v;
        mk_store_stream(t + i, tv, nt);
        acc[0] += vv * tv;
    }
    __device__ void row(int64_t i, double sum, double *acc) { step(i, sum, s * y[i], r1[i], acc); }
    // y IS the product's input: where the kernel holds xin(y[i]) already it passes it
    __device__ void row_x(int64_t i, double sum, double vv, double *acc) { step(i, sum, vv, r1[i], acc); }
    // pipelined kernels (brick march): r1[i] arrives as o[0], loaded at the top of the step
    static constexpr int NPF = 1;
    __device__ const double *pf_vec(int) const { return r1; }
    __device__ void row_pf(int64_t i, double sum, const double *o, double *acc) { step(i, sum, s * y[i], o[0], acc); }
    __device__ void row_x_pf(int64_t i, double sum, double vv, const double *o, double *acc) { step(i, sum, vv, o[0], acc); }
};

struct LzOpL2 {
    static constexpr int NACC = 1, SLOT0 = SLOT_YY;
    const double *part;
    int np;
    LzScal sc;
    LzStatus *st;
    int j;
    const double *r2, *t;
    double *ynew;               // r1's storage: it becomes r2 of the next step
    const double *dinv;         // null: not scaled
    double *y;                  // dinv * ynew (scaled only)
    double c;
    bool bad;
    __device__ bool prologue(double *s4, bool lead) {
        const double alfa = mk_total(part + SLOT_ALFA * MK_MAXP, np, s4);
        const double b = sc.beta[j - 1];
        bad = !isfinite(alfa);
        c = -alfa / b;
        if (lead) {
            sc.alpha[j - 1] = alfa;
            double tm = fabs(alfa);
            if (j > 1) tm = tm + b;
            const double t0 = sc.tmax[j - 1];
            sc.tmax[j] = tm > t0 ? tm : t0;
            if (bad) {
                st->done = j - 1;
                st->nonfinite = j;
            }
        }
        return bad;
    }
    __device__ bool skip() const { return bad; }
    __device__ void pair(int64_t i, double *acc) {
        const double2 rv = mk_ld2(r2, i), tv = mk_ld2(t, i);
        double2 yv;
        yv.x = c * rv.x + tv.x;
        yv.y = c * rv.y + tv.y;
        mk_st2(ynew, i, yv);
        if (dinv) {
            const double2 gv = mk_ld2(dinv, i);
            double2 pv;
            pv.x = gv.x * yv.x;
            pv.y = gv.y * yv.y;
            mk_st2(y, i, pv);
            acc[0] += yv.x * pv.x;
            acc[0] += yv.y * pv.y;
        } else {
            acc[0] += yv.x * yv.x;
            acc[0] += yv.y * yv.y;
        }
    }
    __device__ void one(int64_t i, double *acc) {
        const double yv = c * r2[i] + t[i];
        ynew[i] = yv;
        if (dinv) {
            const double pv = dinv[i] * yv;
            y[i] = pv;
            acc[0] += yv * pv;
        } else {
            acc[0] += yv * yv;
        }
    }
};

// beta_{m+1} of a run that was not stopped
__global__ __launch_bounds__(MK_BLOCK) void lz_final_kernel(const double *part, int np, LzScal sc, LzStatus *st, MkHalt halt, int m) {
    __shared__ double s4[4];
    if (halt.in()) return;
    const double b = __dsqrt_rn(mk_total(part + SLOT_YY * MK_MAXP, np, s4));
    if (threadIdx.x == 0) {
        sc.beta[m] = b;
        st->done = m;
        if (!isfinite(b)) st->nonfinite = m;
    }
}

struct LzBuffers {              // freed on every way out of the call
    double *vec[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    double *part = nullptr;
    char *words = nullptr;
    char *h_words = nullptr;
    ~LzBuffers() {
        for (double *v : vec) hipFree(v);
        hipFree(part);
        hipFree(words);
        free(h_words);
    }
};

}  // namespace

extern "C" int mk_csr_lanczos(const mk_csr *A, int32_t steps, int32_t scale_diag, uint64_t seed, const double *start_dev,
                              double *alpha_host, double *beta_host, int64_t *info, int32_t cap) {
    MK_REQUIRE_INIT();
    MK_ARG(A && alpha_host && beta_host && (cap <= 0 || info));
    const char *fn = "mk_csr_lanczos";
    if (A->comp_kind || A->host_fn || A->alias || A->nops)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator holds no CSR arrays of its own (a composite, reduced, block, "
                       "composed or matrix-free operator): form its matrix with to_csr_arrays() and a CsrOperator", fn);
    if (A->ex.mode >= 0 || A->row_block)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator is row-partitioned (it carries an exchange plan); the "
                       "Lanczos estimate is single-GPU", fn);
    if (A->nrows != A->ncols)
        return mk_fail(MK_ERR_ARG, "%s: the matrix must be square, got %lld x %lld", fn, (long long)A->nrows,
                       (long long)A->ncols);
    if (A->nrows >= ((int64_t)1 << 31))
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: %lld rows; the status word names a row in 32 bits (< 2^31)", fn,
                       (long long)A->nrows);
    if (steps < 1) return mk_fail(MK_ERR_ARG, "%s: steps = %d, at least one step is needed", fn, (int)steps);
    if (A->nrows == 0) return mk_fail(MK_ERR_ARG, "%s: the matrix has no rows", fn);
    MK_ARG(MK_ALIGNED16(start_dev));
    const auto t0 = std::chrono::steady_clock::now();
    MkContext &c = mk_ctx();
    hipStream_t st = c.stream;
    const int64_t n = A->nrows;
    const int m = (int)((int64_t)steps < n ? (int64_t)steps : n);
    const int scaled = scale_diag ? 1 : 0;
    (void)mk_csr_plan(A);                                        // (the storage format is built on the first product: not inside the run)
    LzBuffers B;
    size_t bytes = 0;
    // r1 / r2 (in turn), t, and y, dinv when scaled; 16 bytes of slack behind every vector, zeroed: the product kernels read
    // their input in 16-byte pairs
    const size_t vbytes = sizeof(double) * (size_t)n + 16;
    for (int k = 0; k < (scaled ? 5 : 3); ++k) {
        if (hipMalloc((void **)&B.vec[k], vbytes) != hipSuccess || hipMemsetAsync(B.vec[k], 0, vbytes, st) != hipSuccess) {
            (void)hipGetLastError();
            return mk_fail(MK_ERR_HIP, "%s: out of device memory for the vectors (%zu bytes each)", fn, vbytes);
        }
        bytes += vbytes;
    }
    double *R[2] = {B.vec[0], B.vec[1]}, *d_t = B.vec[2], *d_y = B.vec[3], *d_dinv = B.vec[4];
    const size_t nscal = (size_t)3 * m + 2;
    const size_t wbytes = sizeof(LzStatus) + sizeof(double) * nscal, pbytes = sizeof(double) * NSLOT * MK_MAXP;
    B.h_words = (char *)malloc(wbytes);
    if (!B.h_words || hipMalloc((void **)&B.words, wbytes) != hipSuccess || hipMalloc((void **)&B.part, pbytes) != hipSuccess ||
        hipMemsetAsync(B.words, 0, wbytes, st) != hipSuccess || hipMemsetAsync(B.part, 0, pbytes, st) != hipSuccess) {
        (void)hipGetLastError();
        return mk_fail(MK_ERR_HIP, "%s: out of memory for the scalars", fn);
    }
    bytes += wbytes + pbytes;
    LzStatus *d_st = reinterpret_cast<LzStatus *>(B.words);
    double *d_sc = reinterpret_cast<double *>(B.words + sizeof(LzStatus));
    const LzScal sc{d_sc, d_sc + m, d_sc + 2 * m + 1};
    int64_t q = 0;                                               // launches so far (halt parity)
    int *flags = d_st->halt;
    const auto halt = [&] { return MkHalt{flags, (int)(q++ & 1), 0}; };
    if (scaled) {
        const int64_t g = (n + MK_BLOCK - 1) / MK_BLOCK;
        hipLaunchKernelGGL(lz_dinv_kernel, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(MK_BLOCK), 0, st, A->d_indptr, A->d_indices,
                           A->d_data, n, d_dinv, d_st);
        q += 1;
    }
    const int np_stream = mk_grid_stream(n), np_spmv = mk_grid_spmv_for(A);
    hipLaunchKernelGGL(mk_stream_kernel<LzOpStart>, dim3(np_stream), dim3(MK_BLOCK), 0, st,
                       LzOpStart{start_dev, scaled ? d_dinv : nullptr, R[1], d_y, seed}, n, halt(), B.part);
    const int nt = mk_store_nt(A);
    for (int j = 1; j <= m; ++j) {
        double *r1 = R[(j - 1) & 1], *r2 = R[j & 1];             // L2 writes the new r2 over r1: the roles swap every step
        const double *y = scaled ? d_y : r2;
        const LzEpi epi{B.part, np_stream, sc.beta + (j > 1 ? j - 2 : 0), y, r1, d_t, j == 1 ? 1 : 0, nt, 0.0, 0.0};
        mk_spmv_launch_blocks(A, np_spmv, st, y, epi, LzGate{B.part, np_stream, sc, d_st, j}, halt, B.part);
        hipLaunchKernelGGL(mk_stream_kernel<LzOpL2>, dim3(np_stream), dim3(MK_BLOCK), 0, st,
                           LzOpL2{B.part, np_spmv, sc, d_st, j, r2, d_t, r1, scaled ? d_dinv : nullptr, d_y, 0.0, false}, n, halt(),
                           B.part);
    }
    hipLaunchKernelGGL(lz_final_kernel, dim3(1), dim3(MK_BLOCK), 0, st, B.part, np_stream, sc, d_st, halt(), m);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(B.h_words, B.words, wbytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return mk_fail(MK_ERR_HIP, "%s: the kernels failed", fn);
    if (c.pending_rc != MK_OK) {
        const int rc = c.pending_rc;
        c.pending_rc = MK_OK;
        return rc;
    }
    LzStatus hs;
    memcpy(&hs, B.h_words, sizeof(hs));
    const double *h_sc = reinterpret_cast<const double *>(B.h_words + sizeof(LzStatus));
    const int done = (int)hs.done;
    for (int k = 0; k < done; ++k) alpha_host[k] = h_sc[k];
    for (int k = 0; k <= done; ++k) beta_host[k] = h_sc[m + k];
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    const int64_t v[MK_LANCZOS_INFO_LEN] = {done, q, (int64_t)bytes, (int64_t)llround(us), hs.nonfinite ? 1 : 0};
    for (int32_t k = 0; k < cap && k < MK_LANCZOS_INFO_LEN; ++k) info[k] = v[k];
    if (hs.bad)
        return mk_fail(MK_ERR_ARG, "%s: row %d has no positive diagonal entry (none is stored, or one that is zero or negative): "
                       "scale_diag needs D > 0 for D^-1/2 A D^-1/2 to exist", fn, (int)(n - hs.bad));
    if (hs.nonfinite)
        return mk_fail(MK_ERR_ARG, "%s: alpha or beta of step %lld is not finite (a matrix or start vector with entries that "
                       "are not finite, or overflow)", fn, (long long)hs.nonfinite);
    if (done < 1)
        return mk_fail(MK_ERR_ARG, "%s: beta_1 = %g: the start vector must have a positive, finite norm%s", fn, h_sc[m],
                       scaled ? " in the D^-1 inner product" : "");
    return MK_OK;
}
