// mk_cheb.hip -- Chebyshev polynomial preconditioner z = p_k(A) r of a symmetric device CSR matrix (the preconditioner
// `precon * r` of mk_solver_set_precon_cheb).
//
// The Chebyshev iteration for A z = r from z = 0 on an interval [lmin, lmax] that holds A's spectrum (Saad, Iterative
// Methods, Alg. 12.1); with Jacobi scaling the same iteration for D^-1 A z = D^-1 r.  An apply of degree k is one stream
// launch and k products of the matrix the solver already holds, in whatever storage format the builder chose for it -- no
// triangular dependency, no level schedule: the apply runs at the product kernel's rate.
//
//   init      res = in (dinv * in);  d_0 = res * c0;  out = d_0
//   step j    s = (A d_{j-1})_r (dinv_r * s);  rv = res_r - s;  d_j = c1_j d_{j-1} + c2_j rv;  out += d_j;  res = rv
//
// The step's vector work is the row epilogue of the product (MkChebEpi): d_{j-1}[r] IS the product's input, so a step moves
// the matrix plus about 40 n bytes (read res, out; write d_j, out, res).  The product's input is gathered by other rows, so
// d cannot be updated in place: two d buffers are used in turn.  Every operation rounds on its own (-ffp-contract=off) in
// the order written above; the row sum carries the bits of the plain product in every format, so the result does not
// depend on the format.  The coefficients depend on lmin, lmax and k only and are computed on the host at creation.
#include <chrono>
#include <climits>
#include <cmath>

#include "mk_solver.h"

constexpr double MK_CHEB_RATIO = 30.0;    // default lmin = lmax / 30: the convention of hypre and Ifpack2 for Chebyshev
                                          // smoothing without a lower estimate -- a convention, not a tuned number

struct mk_cheb : MkDeviceOp {
    const mk_csr *A = nullptr;            // borrowed matrix (A->dependents counts this object)
    int degree = 0;
    int scaled = 0;                       // Jacobi scaling: the iteration runs on D^-1 A
    double lmin = 0.0, lmax = 0.0;        // the interval as used
    int lmin_default = 0, lmax_default = 0;
    double c0 = 0.0;
    std::vector<double> c1, c2;           // c1[j - 1], c2[j - 1] of step j
    double *d_res = nullptr;              // residual of the iteration
    double *d_d[2] = {nullptr, nullptr};  // directions d_{j-1}, d_j in turn
    double *d_dinv = nullptr;             // 1 / a_rr (scaled only)
    unsigned long long *d_bound = nullptr;   // bits of the Gershgorin bound, then the status word (smallest bad row)
    double setup_us = 0.0;
    size_t bytes = 0;                     // device bytes owned
    ~mk_cheb() override;
    const char *noun() const override { return "Chebyshev preconditioner"; }
    int enqueue(const double *in, double *out, hipStream_t stream, int *flags, int64_t *q) const override;
};

// ------------------------------------------------------------------ kernels
struct MkOpChebInit {           // res = in (dinv * in) ; d0 = res * c0 ; out = d0     (in == out allowed)
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *in, *dinv;
    double *res, *d0, *out;
    double c0;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 v = mk_ld2(in, i);
        if (dinv) {
            const double2 g = mk_ld2(dinv, i);
            v.x = g.x * v.x;
            v.y = g.y * v.y;
        }
        mk_st2(res, i, v);
        double2 d;
        d.x = v.x * c0;
        d.y = v.y * c0;
        mk_st2(d0, i, d);
        mk_st2(out, i, d);
    }
    __device__ void one(int64_t i, double *) {
        double v = in[i];
        if (dinv) v = dinv[i] * v;
        res[i] = v;
        const double d = v * c0;
        d0[i] = d;
        out[i] = d;
    }
};

// Row epilogue of step j.  ONE type for every step: scaling, the last step and the coefficients are launch-uniform run-time
// fields, because every epilogue type instantiates mk_spmv_kernel once per storage format (mk_device.h, "Compile-time
// budget").
struct MkChebEpi {
    static constexpr int NACC = 0, SLOT0 = 0;
    // Neither SYM_MARCH nor NO_MARCH.  The matrix is the SOLVER's: a MINRES / SYMMLQ / BiCGSTAB matrix on a structured grid
    // may be stored as a brick march (formats 9, 10) and the steps should then run as that pipelined kernel, so NO_MARCH is
    // out.  SYM_MARCH would add the format-11 and general-geometry kernels, which take no prefetched epilogue operands
    // (mk_spmv_fmt9.h: plain products and CG only) -- this epilogue's res[r] and out[r] are exactly such operands.  Format 11
    // is what only a CG solver's matrix gets (mk_csr_march_pref caps every other loop's at format 10): a Chebyshev object
    // that preconditions CG on such a matrix, or shares it with a CG solver (and likewise on a march matrix of a general
    // geometry), has its steps run as the CSR gather kernel on the same arrays -- same row sums, same bits, at the gather
    // kernel's rate -- while CG's own product keeps its format-11 kernel.
    const double *dprev;        // d_{j-1}: the product's input
    const double *dinv;         // null: no scaling
    double *res, *dnext, *out;
    double c1, c2;
    int last;                   // the last step leaves res alone (nothing reads it any more)
    int nt;                     // d_j goes past the caches (vectors beyond the Infinity Cache; mk_store_stream)
    __device__ void prologue(double *) {}
    __device__ double xin(double v) const { return v; }
    __device__ __forceinline__ void step(int64_t r, double s, double dp, double rs, double ov) {
        if (dinv) s = dinv[r] * s;
        const double rv = rs - s;
        double dn = c1 * dp;
        const double t = c2 * rv;
        dn = dn + t;
        mk_store_stream(dnext + r, dn, nt);
        out[r] = ov + dn;
        if (!last) res[r] = rv;
    }
    __device__ void row(int64_t r, double s, double *) { step(r, s, dprev[r], res[r], out[r]); }
    // d_{j-1} IS the product's input: where the kernel holds x[r] already it passes it, and d_{j-1} is not loaded twice
    __device__ void row_x(int64_t r, double s, double xr, double *) { step(r, s, xr, res[r], out[r]); }
    // pipelined kernels (brick march): res[r], out[r] arrive as o[0], o[1], loaded at the top of the step
    static constexpr int NPF = 2;
    __device__ const double *pf_vec(int j) const { return j == 0 ? res : out; }
    __device__ void row_pf(int64_t r, double s, const double *o, double *) { step(r, s, dprev[r], o[0], o[1]); }
    __device__ void row_x_pf(int64_t r, double s, double xr, const double *o, double *) { step(r, s, xr, o[0], o[1]); }
};

// Gershgorin bound max_r sum_j |a_rj| (scaled: / |a_rr|) over the CSR arrays, each row added left to right in stored order
// by one lane; scaled, also dinv[r] = 1 / a_rr, and the smallest row without a usable diagonal goes into *status.  The
// maximum is taken on the bit patterns: the sums are >= +0.0, where the order of the patterns is the order of the values,
// and a NaN compares above every number, so it reaches the host and is refused there.
__global__ __launch_bounds__(MK_BLOCK) void mk_cheb_bound_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                const double *__restrict__ data, int64_t n, int scaled,
                                                                double *__restrict__ dinv, unsigned long long *bound, int *status) {
    __shared__ unsigned long long smax;
    if (threadIdx.x == 0) smax = 0ull;
    __syncthreads();
    unsigned long long mb = 0ull;
    for (int64_t r = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * MK_BLOCK) {
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
        if (scaled) {
            if (!have || arr == 0.0) {
                atomicMin(status, (int)r);
                continue;
            }
            dinv[r] = 1.0 / arr;
            s = s / fabs(arr);
        }
        const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(s));
        mb = b > mb ? b : mb;
    }
    atomicMax(&smax, mb);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(bound, smax);
}

__global__ void mk_cheb_words_init(unsigned long long *bound, int *status) {
    if (threadIdx.x == 0) {
        *bound = 0ull;
        *status = INT_MAX;
    }
}

// out = p_k(A) in (in == out allowed): one stream launch, then one product launch per step.  `q` = the solver's kernel
// counter (halt parity), or null for a standalone run.  Used by mk_cheb_apply and by the solvers'
// preconditioner sites (mk_solver.hip, mk_lls.hip).
int mk_cheb::enqueue(const double *in, double *out, hipStream_t st, int *flags, int64_t *q) const {
    if (n == 0) return MK_OK;
    const auto next = [&] { return halt(flags, q); };
    double *const nopart = nullptr;                              // (no fused dots: no partial sums are written)
    hipLaunchKernelGGL(mk_stream_kernel<MkOpChebInit>, dim3(mk_grid_stream(n)), dim3(MK_BLOCK), 0, st,
                       MkOpChebInit{in, d_dinv, d_res, d_d[0], out, c0}, n, next(), nopart);
    const int nt = mk_store_nt(A);
    for (int j = 1; j <= degree; ++j) {
        const MkChebEpi epi{d_d[(j - 1) & 1], d_dinv, d_res, d_d[j & 1], out, c1[j - 1], c2[j - 1], j == degree ? 1 : 0, nt};
        mk_spmv_launch_blocks(A, mk_grid_spmv_for(A), st, d_d[(j - 1) & 1], epi, MkNoGate(), next, nopart);
    }
    MK_HIP(hipGetLastError());
    return MK_OK;
}

mk_cheb::~mk_cheb() {
    if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
    hipFree(d_res);
    hipFree(d_d[0]);
    hipFree(d_d[1]);
    hipFree(d_dinv);
    hipFree(d_bound);
    if (A) mk_release_operand(A);
}

// ======================================================================================
// C ABI
// ======================================================================================
extern "C" int mk_cheb_create(const mk_csr *A, int32_t degree, double lmin, double lmax, int32_t scale_diag, mk_cheb **out) {
    MK_REQUIRE_INIT();
    MK_ARG(A && out);
    const char *fn = "mk_cheb_create";
    if (A->comp_kind || A->host_fn || A->alias || A->nops)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator holds no CSR arrays of its own (a composite, reduced, block, "
                       "composed or matrix-free operator): form its matrix with to_csr_arrays() and a CsrOperator", fn);
    if (A->ex.mode >= 0 || A->row_block)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator is row-partitioned (it carries an exchange plan); the "
                       "Chebyshev preconditioner is single-GPU", fn);
    if (A->nrows != A->ncols)
        return mk_fail(MK_ERR_ARG, "%s: the matrix must be square, got %lld x %lld", fn, (long long)A->nrows,
                       (long long)A->ncols);
    if (A->nrows >= ((int64_t)1 << 31))
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: %lld rows; the status word names a row in 32 bits (< 2^31)", fn,
                       (long long)A->nrows);
    if (degree < 1 || degree > MK_CHEB_MAX_DEGREE)
        return mk_fail(MK_ERR_ARG, "%s: degree %d is outside 1 .. %d", fn, (int)degree, MK_CHEB_MAX_DEGREE);
    if (!std::isfinite(lmin) || !std::isfinite(lmax))
        return mk_fail(MK_ERR_ARG, "%s: lmin = %g, lmax = %g must be finite", fn, lmin, lmax);
    if (lmin > 0.0 && lmax > 0.0 && lmin >= lmax)
        return mk_fail(MK_ERR_ARG, "%s: the interval needs 0 < lmin < lmax, got lmin = %g, lmax = %g", fn, lmin, lmax);
    const auto t0 = std::chrono::steady_clock::now();
    MkContext &c = mk_ctx();
    const int64_t n = A->nrows;
    mk_cheb *F = new mk_cheb();
    F->n = n;
    F->degree = degree;
    F->scaled = scale_diag ? 1 : 0;
    F->A = A;
    A->dependents += 1;
    const auto fail = [&](int code) {
        delete F;
        return code;
    };
    // (16 bytes of slack behind every vector, zeroed: the product kernels read their input in 16-byte pairs)
    const size_t vbytes = sizeof(double) * (size_t)(n > 0 ? n : 1) + 16;
    double **vecs[4] = {&F->d_res, &F->d_d[0], &F->d_d[1], &F->d_dinv};
    for (int k = 0; k < (F->scaled ? 4 : 3); ++k) {
        if (hipMalloc((void **)vecs[k], vbytes) != hipSuccess || hipMemsetAsync(*vecs[k], 0, vbytes, c.stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory for the vectors (%zu bytes each)", fn, vbytes));
        }
        F->bytes += vbytes;
    }
    if (hipMalloc((void **)&F->d_bound, 2 * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory", fn));
    }
    const int rc = F->init_nohalt(c.stream);
    if (rc != MK_OK) return fail(rc);
    F->bytes += 2 * sizeof(int) + 2 * sizeof(unsigned long long);    // (the two halt words; the bound and the status word)
    int *d_status = reinterpret_cast<int *>(F->d_bound + 1);
    hipLaunchKernelGGL(mk_cheb_words_init, dim3(1), dim3(64), 0, c.stream, F->d_bound, d_status);
    F->lmax_default = lmax > 0.0 ? 0 : 1;
    F->lmin_default = lmin > 0.0 ? 0 : 1;
    unsigned long long hb[2] = {0ull, 0ull};
    if (n > 0 && (F->scaled || F->lmax_default)) {
        const int64_t g = (n + MK_BLOCK - 1) / MK_BLOCK;
        hipLaunchKernelGGL(mk_cheb_bound_kernel, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(MK_BLOCK), 0, c.stream, A->d_indptr,
                           A->d_indices, A->d_data, n, F->scaled, F->d_dinv, F->d_bound, d_status);
    }
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hb, F->d_bound, sizeof(hb), hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
        hipStreamSynchronize(c.stream) != hipSuccess)
        return fail(mk_fail(MK_ERR_HIP, "%s: the set-up kernels failed", fn));
    int bad = INT_MAX;
    memcpy(&bad, &hb[1], sizeof(int));
    if (bad != INT_MAX)
        return fail(mk_fail(MK_ERR_ARG, "%s: row %d has no usable diagonal entry (none is stored, or a zero): scale_diag "
                            "divides by a_rr", fn, bad));
    if (F->lmax_default) {
        memcpy(&lmax, &hb[0], sizeof(double));
        if (!(std::isfinite(lmax) && lmax > 0.0))
            return fail(mk_fail(MK_ERR_ARG, "%s: the Gershgorin bound of the matrix is %g; give lmax", fn, lmax));
    }
    if (F->lmin_default) lmin = lmax / MK_CHEB_RATIO;
    if (!(lmin > 0.0 && lmin < lmax))
        return fail(mk_fail(MK_ERR_ARG, "%s: the interval needs 0 < lmin < lmax, got lmin = %g, lmax = %g", fn, lmin, lmax));
    F->lmin = lmin;
    F->lmax = lmax;
    // the coefficients (Saad Alg. 12.1), one rounding per operation, in exactly this order
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
    F->c0 = 1.0 / theta;
    double rho = 1.0 / sigma;
    F->c1.resize((size_t)degree);
    F->c2.resize((size_t)degree);
    for (int j = 1; j <= degree; ++j) {
        const double rho_j = 1.0 / (2.0 * sigma - rho);
        F->c1[j - 1] = rho_j * rho;
        F->c2[j - 1] = (2.0 * rho_j) / delta;
        rho = rho_j;
    }
    F->setup_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    *out = F;
    return MK_OK;
}

const MkDeviceOp *mk_cheb_as_op(const mk_cheb *F) { return F; }

extern "C" int mk_cheb_destroy(mk_cheb *F) {
    if (F) F->destroy();                                         // (while solvers still apply it: freed with the last of them)
    return MK_OK;
}

extern "C" int mk_cheb_apply(const mk_cheb *F, const double *in_dev, double *out_dev) {
    return MkDeviceOp::apply_standalone(F, in_dev, out_dev);
}

extern "C" int mk_cheb_info(const mk_cheb *F, int64_t *info, int32_t cap) {
    MK_ARG(F && (cap <= 0 || info));
    const int64_t v[MK_CHEB_INFO_LEN] = {F->n,
                                         F->degree,
                                         F->scaled,
                                         1 + (int64_t)F->degree,
                                         (int64_t)F->bytes,
                                         (int64_t)llround(F->setup_us),
                                         F->lmin_default,
                                         F->lmax_default};
    for (int32_t k = 0; k < cap && k < MK_CHEB_INFO_LEN; ++k) info[k] = v[k];
    return MK_OK;
}

extern "C" int mk_cheb_coefficients(const mk_cheb *F, double *host) {
    MK_ARG(F && host);
    host[0] = F->lmin;
    host[1] = F->lmax;
    host[2] = F->c0;
    for (int j = 0; j < F->degree; ++j) {
        host[3 + 2 * j] = F->c1[(size_t)j];
        host[4 + 2 * j] = F->c2[(size_t)j];
    }
    return MK_OK;
}

extern "C" int mk_solver_set_precon_cheb(mk_solver *s, const mk_cheb *F) {
    return mk_set_precon(s, -1, MkPrecon::object(F), "mk_solver_set_precon_cheb");
}

extern "C" int mk_solver_set_lls_precon_cheb(mk_solver *s, int side, const mk_cheb *F) {
    return mk_set_precon(s, side, MkPrecon::object(F), "mk_solver_set_lls_precon_cheb");
}
