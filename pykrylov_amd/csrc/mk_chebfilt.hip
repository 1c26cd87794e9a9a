// mk_chebfilt.hip -- scaled Chebyshev filter y = rho(A) x of a symmetric device CSR matrix (Zhou and Saad), the spectral
// transformation of the thick-restart Lanczos eigensolver (the block mk_params_filter, mk_trlan.hip).
//
// [a, b] is the UNWANTED interval and a0 a reference point strictly outside it, on the wanted side:
//     rho(t) = T_d((t - c) / e) / T_d((a0 - c) / e),    e = (b - a) / 2,  c = (b + a) / 2
// is at most 1 / T_d((a0 - c) / e) in modulus on [a, b], 1 at a0, positive and monotone beyond the end a0 lies at: the
// largest eigenvalues of rho(A) belong to A's most extreme ones on that side, and the gaps between them are stretched.
// The three-term recurrence with the scaling folded in (one rounding per operation, in this order, on the host):
//     sigma_1 = e / (a0 - c);  tau = 2.0 / sigma_1;  p_1 = sigma_1 / e;  q_1 = 0
//     j = 2..d:  sigma_j = 1.0 / (tau - sigma_{j-1});  p_j = (2.0 * sigma_j) / e;  q_j = sigma_{j-1} * sigma_j
//     y_0 = x;   y_j[r] = p_j * ((A y_{j-1})[r] - c * y_{j-1}[r]) - q_j * y_{j-2}[r]           (step 1: no y_{-1} term)
// An apply of degree d is d products of the matrix in whatever storage format it has; the step's vector work is the row
// epilogue of the product (MkChebFiltEpi): y_{j-1}[r] IS the product's input and y_{j-2}[r] the one prefetched operand, so a
// step moves the matrix plus 8 n bytes (none in step 1).  y_j is written over y_{j-2}: the same lane reads and writes row r
// and only y_{j-1} is gathered by other rows, so two owned vectors take the steps in turn and the last step writes `out`;
// `in` is never written.  Every operation rounds on its own (-ffp-contract=off); the row sum carries the bits of the plain
// product in every format, so the result does not depend on the format.
//
// An end of [a, b] that is not given comes from the Gershgorin interval [min_r (a_rr - off_r), max_r (a_rr + off_r)],
// off_r = sum_{j != r} |a_rj|, each row added left to right in stored order by one lane (cf_gershgorin_kernel).
#include <chrono>
#include <cmath>

#include "mk_solver.h"

struct mk_filter : MkDeviceOp {
    const mk_csr *A = nullptr;            // borrowed matrix (A->dependents counts this object)
    int degree = 0;
    double a = 0.0, b = 0.0, a0 = 0.0;    // the interval and the reference point as used
    int a_default = 0, b_default = 0;     // the end is the Gershgorin one
    double c = 0.0, e = 0.0;
    std::vector<double> p, q;             // p[j - 1], q[j - 1] of step j
    double *d_y[2] = {nullptr, nullptr};  // y_j, j < degree, lives in d_y[j & 1]
    unsigned long long *d_bound = nullptr;   // the keys of the Gershgorin interval: lower end, upper end
    double setup_us = 0.0;
    size_t bytes = 0;                     // device bytes owned
    ~mk_filter() override;
    const char *noun() const override { return "Chebyshev filter"; }
    int enqueue(const double *in, double *out, hipStream_t stream, int *flags, int64_t *q) const override;
};

// ------------------------------------------------------------------ kernels
// Row epilogue of step j.  ONE type for every step: the coefficients, the first step and the non-temporal store are
// launch-uniform run-time fields, because every epilogue type instantiates mk_spmv_kernel once per storage format
// (mk_device.h, "Compile-time budget").  Neither SYM_MARCH nor NO_MARCH, for MkChebEpi's reasons (mk_cheb.hip): on formats 9
// and 10 the step runs as the pipelined march kernel with y_{j-2}[r] prefetched, on format 11 and on a march matrix of a
// general geometry as the CSR gather kernel on the same arrays -- same row sums, same bits.
struct MkChebFiltEpi {
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *yin;          // y_{j-1}: the product's input
    const double *yprev;        // y_{j-2}; in the first step any readable vector of n entries (the march kernel loads it)
    double *ynext;              // y_j; the storage of y_{j-2} from the third step on
    double p, q, c;
    int first;                  // j == 1: y_{j-2} is neither loaded nor subtracted
    int nt;                     // y_j goes past the caches (vectors beyond the Infinity Cache; mk_store_stream)
    __device__ void prologue(double *) {}
    __device__ double xin(double v) const { return v; }
    __device__ __forceinline__ void step(int64_t r, double s, double xr, double yp) {
        const double u = c * xr;
        const double t = s - u;
        double yn = p * t;
        if (!first) {
            const double v = q * yp;
            yn = yn - v;
        }
        mk_store_stream(ynext + r, yn, nt);
    }
    __device__ void row(int64_t r, double s, double *) { step(r, s, yin[r], first ? 0.0 : yprev[r]); }
    // y_{j-1} IS the product's input: where the kernel holds x[r] already it passes it
    __device__ void row_x(int64_t r, double s, double xr, double *) { step(r, s, xr, first ? 0.0 : yprev[r]); }
    // pipelined kernels (brick march): y_{j-2}[r] arrives as o[0], loaded at the top of the step
    static constexpr int NPF = 1;
    __device__ const double *pf_vec(int) const { return yprev; }
    __device__ void row_pf(int64_t r, double s, const double *o, double *) { step(r, s, yin[r], o[0]); }
    __device__ void row_x_pf(int64_t r, double s, double xr, const double *o, double *) { step(r, s, xr, o[0]); }
};

// An integer key whose unsigned order is the order of the doubles (-inf < ... < -0.0 < +0.0 < ... < +inf): the minimum and
// the maximum over the rows are taken on the keys by integer atomics, so the result does not depend on the order in which
// the rows arrive.  A NaN lands beyond an infinity at one of the ends and is refused on the host.
__host__ __device__ static inline unsigned long long cf_key(double v) {
    unsigned long long u;
    memcpy(&u, &v, sizeof(u));
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
static inline double cf_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &u, sizeof(v));
    return v;
}

// bound[0] = min_r key(a_rr - off_r), bound[1] = max_r key(a_rr + off_r); one lane per row, the entries in stored order
// (entries on the diagonal are added up to a_rr, the moduli of the others to off_r, both from +0.0)
__global__ __launch_bounds__(MK_BLOCK) void cf_gershgorin_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                const double *__restrict__ data, int64_t n,
                                                                unsigned long long *bound) {
    __shared__ unsigned long long smin, smax;
    if (threadIdx.x == 0) {
        smin = ~0ull;
        smax = 0ull;
    }
    __syncthreads();
    unsigned long long lo = ~0ull, hi = 0ull;
    for (int64_t r = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * MK_BLOCK) {
        const int p1 = indptr[r + 1];
        double arr = 0.0, off = 0.0;
        for (int k = indptr[r]; k < p1; ++k) {
            const double v = data[k];
            if (indices[k] == r) arr = arr + v;
            else off = off + fabs(v);
        }
        const unsigned long long kl = cf_key(arr - off), kh = cf_key(arr + off);
        lo = kl < lo ? kl : lo;
        hi = kh > hi ? kh : hi;
    }
    atomicMin(&smin, lo);
    atomicMax(&smax, hi);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(bound, smin);
        atomicMax(bound + 1, smax);
    }
}

// out = rho(A) in (in != out; `in` is not written): one product launch per step.  `q` = the solver's kernel counter (halt
// parity), or null for a standalone run.  Used by the probe and by the filtered cycle of mk_trlan.hip.
int mk_filter::enqueue(const double *in, double *out, hipStream_t st, int *flags, int64_t *kq) const {
    if (n == 0) return MK_OK;
    if (in == out)
        return mk_fail(MK_ERR_ARG, "the Chebyshev filter: in == out; the filter gathers its input while it writes the result");
    const auto next = [&] { return halt(flags, kq); };
    double *const nopart = nullptr;                              // (no fused dots: no partial sums are written)
    const int nt = mk_store_nt(A);
    for (int j = 1; j <= degree; ++j) {
        const double *yin = j == 1 ? in : d_y[(j - 1) & 1];
        const double *yprev = j <= 2 ? in : d_y[j & 1];          // (y_0 = in; the first step only needs it readable)
        double *ynext = j == degree ? out : d_y[j & 1];
        const MkChebFiltEpi epi{yin, yprev, ynext, p[j - 1], q[j - 1], c, j == 1 ? 1 : 0, nt};
        mk_spmv_launch_blocks(A, mk_grid_spmv_for(A), st, yin, epi, MkNoGate(), next, nopart);
    }
    MK_HIP(hipGetLastError());
    return MK_OK;
}

mk_filter::~mk_filter() {
    if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
    hipFree(d_y[0]);
    hipFree(d_y[1]);
    hipFree(d_bound);
    if (A) mk_release_operand(A);
}

const MkDeviceOp *mk_filter_as_op(const mk_filter *F) { return F; }

void mk_filter_describe(const mk_filter *F, const mk_csr **A, int *degree, double *a, double *b, double *a0) {
    *A = F->A;
    *degree = F->degree;
    *a = F->a;
    *b = F->b;
    *a0 = F->a0;
}

// 5 + 2 degree + MK_FILTER_INFO_LEN doubles: a, b and a0 as used, c, e, then p_1, q_1, ..., p_d, q_d, then the info -- rows,
// degree, the wanted side (0 smallest, 1 largest), launches per apply, device bytes held, set-up time (us), whether a / b is
// the Gershgorin end
std::vector<double> mk_filter_table(const mk_filter *F) {
    std::vector<double> t = {F->a, F->b, F->a0, F->c, F->e};
    for (int j = 0; j < F->degree; ++j) {
        t.push_back(F->p[(size_t)j]);
        t.push_back(F->q[(size_t)j]);
    }
    const double info[MK_FILTER_INFO_LEN] = {(double)F->n, (double)F->degree, F->a0 > F->b ? 1.0 : 0.0, (double)F->degree,
                                             (double)F->bytes, (double)llround(F->setup_us), (double)F->a_default,
                                             (double)F->b_default};
    t.insert(t.end(), info, info + MK_FILTER_INFO_LEN);
    return t;
}

void mk_filter_free(mk_filter *F) {
    if (F) F->destroy();
}

// The object has no entry point of its own (the C ABI keeps its functions): a MK_TRLAN solver creates it from the tail of
// mk_params_filter (mk_solver_create) and owns it.
int mk_filter_create(const mk_csr *A, int32_t degree, double a, double b, double a0, mk_filter **out) {
    MK_REQUIRE_INIT();
    MK_ARG(A && out);
    const char *fn = "mk_solver_create: the Chebyshev filter";
    if (A->comp_kind || A->host_fn || A->alias || A->nops)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator holds no CSR arrays of its own (a composite, reduced, block, "
                       "composed or matrix-free operator): form its matrix with to_csr_arrays() and a CsrOperator", fn);
    if (A->ex.mode >= 0 || A->row_block)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator is row-partitioned (it carries an exchange plan or a row block); "
                       "the Chebyshev filter is single-GPU", fn);
    if (A->nrows != A->ncols)
        return mk_fail(MK_ERR_ARG, "%s: the matrix must be square, got %lld x %lld", fn, (long long)A->nrows,
                       (long long)A->ncols);
    if (degree < 1 || degree > MK_FILTER_MAX_DEGREE)
        return mk_fail(MK_ERR_ARG, "%s: degree %d is outside 1 .. %d", fn, (int)degree, MK_FILTER_MAX_DEGREE);
    if (!std::isfinite(a0)) return mk_fail(MK_ERR_ARG, "%s: the reference point a0 = %g must be finite", fn, a0);
    if (std::isinf(a) || std::isinf(b))
        return mk_fail(MK_ERR_ARG, "%s: the interval [%g, %g] must be finite (a NaN end selects the Gershgorin end)", fn, a, b);
    if (a >= b) return mk_fail(MK_ERR_ARG, "%s: the interval needs a < b, got a = %g, b = %g", fn, a, b);
    const auto t0 = std::chrono::steady_clock::now();
    MkContext &ctx = mk_ctx();
    const int64_t n = A->nrows;
    mk_filter *F = new mk_filter();
    F->n = n;
    F->degree = degree;
    F->A = A;
    A->dependents += 1;
    const auto fail = [&](int code) {
        delete F;
        return code;
    };
    // y_j for odd j < degree in d_y[1], for even j in d_y[0] (16 bytes of slack behind every vector, zeroed: the product
    // kernels read their input in 16-byte pairs)
    const size_t vbytes = sizeof(double) * (size_t)(n > 0 ? n : 1) + 16;
    for (int k = 0; k < 2; ++k) {
        if (degree < (k == 1 ? 2 : 3)) continue;
        if (hipMalloc((void **)&F->d_y[k], vbytes) != hipSuccess || hipMemsetAsync(F->d_y[k], 0, vbytes, ctx.stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory for the vectors (%zu bytes each)", fn, vbytes));
        }
        F->bytes += vbytes;
    }
    if (hipMalloc((void **)&F->d_bound, 2 * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory", fn));
    }
    const int rc = F->init_nohalt(ctx.stream);
    if (rc != MK_OK) return fail(rc);
    F->bytes += 2 * sizeof(int) + 2 * sizeof(unsigned long long);    // (the two halt words; the two keys)
    F->a_default = std::isnan(a) ? 1 : 0;
    F->b_default = std::isnan(b) ? 1 : 0;
    if (F->a_default || F->b_default) {
        if (n == 0) return fail(mk_fail(MK_ERR_ARG, "%s: the matrix has no rows: it has no Gershgorin interval", fn));
        unsigned long long hb[2] = {0ull, 0ull};
        const int64_t g = (n + MK_BLOCK - 1) / MK_BLOCK;
        if (hipMemsetAsync(F->d_bound, 0xff, sizeof(unsigned long long), ctx.stream) != hipSuccess ||
            hipMemsetAsync(F->d_bound + 1, 0, sizeof(unsigned long long), ctx.stream) != hipSuccess)
            return fail(mk_fail(MK_ERR_HIP, "%s: the set-up failed", fn));
        hipLaunchKernelGGL(cf_gershgorin_kernel, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(MK_BLOCK), 0, ctx.stream, A->d_indptr,
                           A->d_indices, A->d_data, n, F->d_bound);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hb, F->d_bound, sizeof(hb), hipMemcpyDeviceToHost, ctx.stream) != hipSuccess ||
            hipStreamSynchronize(ctx.stream) != hipSuccess)
            return fail(mk_fail(MK_ERR_HIP, "%s: the set-up kernel failed", fn));
        const double glo = cf_unkey(hb[0]), ghi = cf_unkey(hb[1]);
        if (!std::isfinite(glo) || !std::isfinite(ghi))
            return fail(mk_fail(MK_ERR_ARG, "%s: the Gershgorin interval of the matrix is [%g, %g]; give both ends", fn, glo, ghi));
        if (F->a_default) a = glo;
        if (F->b_default) b = ghi;
    }
    if (!(a < b)) return fail(mk_fail(MK_ERR_ARG, "%s: the interval needs a < b, got a = %g, b = %g", fn, a, b));
    if (a0 >= a && a0 <= b)
        return fail(mk_fail(MK_ERR_ARG, "%s: the reference point a0 = %g lies inside the unwanted interval [%g, %g]; it must "
                            "lie strictly outside, on the wanted side", fn, a0, a, b));
    F->a = a;
    F->b = b;
    F->a0 = a0;
    // the coefficients, one rounding per operation, in exactly this order
    const double e = 0.5 * (b - a), c = 0.5 * (b + a);
    double sigma = e / (a0 - c);
    const double tau = 2.0 / sigma;
    F->e = e;
    F->c = c;
    F->p.resize((size_t)degree);
    F->q.resize((size_t)degree);
    F->p[0] = sigma / e;
    F->q[0] = 0.0;
    for (int j = 2; j <= degree; ++j) {
        const double sigma_j = 1.0 / (tau - sigma);
        F->p[j - 1] = (2.0 * sigma_j) / e;
        F->q[j - 1] = sigma * sigma_j;
        sigma = sigma_j;
    }
    for (int j = 0; j < degree; ++j)
        if (!std::isfinite(F->p[(size_t)j]) || !std::isfinite(F->q[(size_t)j]))
            return fail(mk_fail(MK_ERR_ARG, "%s: the coefficients of step %d are not finite (an interval or a reference point "
                                "beyond the range of the format)", fn, j + 1));
    F->setup_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    *out = F;
    return MK_OK;
}
