// mk_ilu.hip -- incomplete factorizations ILU(0) / IC(0) on the pattern of a device CSR matrix, and their
// level-scheduled triangular solves (the preconditioner `precon * r` of mk_solver_set_precon_ilu).
//
// The factor keeps A's pattern (borrowed d_indptr / d_indices) and owns one value array over it:
//   ILU(0): L (unit lower, the entries left of the diagonal) and U (diagonal and right of it), Saad Alg. 10.4 (IKJ);
//   IC(0):  L on the lower pattern and the diagonal, mirrored into the upper positions (U = L^T), so that both
//           sweeps of either kind are row-oriented over the same index set.
// Row i of the forward sweep depends on the rows k < i it stores; of the backward sweep on the stored j > i.  The host
// analysis (O(nnz), once) groups the rows of each sweep into levels; a level's rows are independent.  Every row is
// summed by ONE lane, left to right in column order, with one rounding per multiply and per subtraction
// (-ffp-contract=off): the bits do not depend on how rows are grouped into levels or launches.
//
// Launch plan per sweep: a level with more than `fuse` rows is one launch over its rows; a run of consecutive levels
// with at most `fuse` rows each is ONE workgroup that walks the levels with __syncthreads() in between (no workgroup ever
// waits for another).  MK_ILU_FUSE_ROWS (read when a factor is created) sets `fuse`; 0 = one launch per level.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>

#include "mk_solver.h"

constexpr int MK_ILU_FUSE_DEFAULT = 256;   // rows per level a single workgroup takes in a fused run
constexpr int MK_ILU_RUN_MAX = 2048;       // levels of one fused run (their offsets are staged in LDS)

struct MkIluLaunch {
    int lev0, lev1;    // levels [lev0, lev1) of the sweep
    int grid;          // workgroups (1 for a fused run)
};

struct MkIluSweep {    // one sweep's row lists: rows of level L are rows[lev[L] .. lev[L + 1])
    int32_t *d_rows = nullptr;
    int32_t *d_lev = nullptr;
    int levels = 0;
    int64_t widest = 0;
    std::vector<MkIluLaunch> plan;
};

struct mk_ilu : MkDeviceOp {
    const mk_csr *A = nullptr;     // borrowed pattern (A->dependents counts this factor)
    int kind = 0;                  // 0 ILU(0), 1 IC(0)
    int64_t nnz = 0;
    double *d_val = nullptr;       // factor values on A's pattern (nnz + MK_CSR_PAD)
    int32_t *d_diag = nullptr;     // position of the diagonal entry of each row
    MkIluSweep fw, bw;
    int fuse = MK_ILU_FUSE_DEFAULT;
    int *d_status = nullptr;       // smallest failing row of the factorization (INT_MAX: none)
    double analysis_us = 0.0, factor_us = 0.0;
    size_t bytes = 0;              // device bytes owned by the factor
    ~mk_ilu() override;
    const char *noun() const override { return "incomplete factorization"; }
    int enqueue(const double *in, double *out, hipStream_t stream, int *flags, int64_t *q) const override;
};

struct MkIluView {                 // what a kernel reads of a factor and one sweep
    const int32_t *indptr, *indices, *diag, *rows, *lev;
    double *val;
};

enum { MK_ILU_FWD = 0, MK_ILU_FWD_DIV = 1, MK_ILU_BWD = 2, MK_ILU_FACT = 3, MK_ILU_FACT_IC = 4 };

// Levels [lev0, lev1) of a sweep.  MODE:
//   MK_ILU_FWD      out_i = in_i - sum_{j<i} L_ij out_j                     (ILU(0): unit L)
//   MK_ILU_FWD_DIV  out_i = (in_i - sum_{j<i} L_ij out_j) / L_ii            (IC(0))
//   MK_ILU_BWD      out_i = (out_i - sum_{j>i} U_ij out_j) / U_ii           (in place)
//   MK_ILU_FACT     row i of ILU(0) (IKJ), zero pivots into *status by atomic min
//   MK_ILU_FACT_IC  row i of IC(0), breakdowns likewise
// The applies obey the loop's halt words like every kernel of a solver pass (the factorization runs with the object's own).
template <int MODE>
__global__ __launch_bounds__(MK_BLOCK) void mk_ilu_kernel(MkIluView F, int lev0, int lev1, const double *in, double *out,
                                                         int *status, MkHalt halt) {
    __shared__ int offs[MK_ILU_RUN_MAX + 1];
    const bool halted = halt.in();
    if (blockIdx.x == 0 && threadIdx.x == 0) halt.out(halted);
    if (halted) return;
    const int nl = lev1 - lev0;
    for (int t = threadIdx.x; t <= nl; t += MK_BLOCK) offs[t] = F.lev[lev0 + t];
    __syncthreads();
    for (int L = 0; L < nl; ++L) {
        const int end = offs[L + 1];
        for (int idx = offs[L] + (int)(blockIdx.x * MK_BLOCK + threadIdx.x); idx < end; idx += (int)(gridDim.x * MK_BLOCK)) {
            const int i = F.rows[idx];
            if constexpr (MODE == MK_ILU_FWD || MODE == MK_ILU_FWD_DIV) {
                const int pd = F.diag[i];
                double s = in[i];
                for (int p = F.indptr[i]; p < pd; ++p) s = s - F.val[p] * out[F.indices[p]];
                if constexpr (MODE == MK_ILU_FWD_DIV) s = s / F.val[pd];
                out[i] = s;
            } else if constexpr (MODE == MK_ILU_BWD) {
                const int pd = F.diag[i], p1 = F.indptr[i + 1];
                double s = out[i];
                for (int p = pd + 1; p < p1; ++p) s = s - F.val[p] * out[F.indices[p]];
                out[i] = s / F.val[pd];
            } else if constexpr (MODE == MK_ILU_FACT) {
                // w = row i; for each stored k < i: w_k /= u_kk, then w_j -= w_k u_kj for the stored j > k of both rows
                const int p0 = F.indptr[i], pd = F.diag[i], p1 = F.indptr[i + 1];
                for (int pk = p0; pk < pd; ++pk) {
                    const int k = F.indices[pk];
                    const int dk = F.diag[k];
                    const double wk = F.val[pk] / F.val[dk];
                    F.val[pk] = wk;
                    int p = pk + 1, q = dk + 1;
                    const int qe = F.indptr[k + 1];
                    while (p < p1 && q < qe) {
                        const int cj = F.indices[p], ck = F.indices[q];
                        if (cj == ck) {
                            F.val[p] = F.val[p] - wk * F.val[q];
                            ++p;
                            ++q;
                        } else if (cj < ck) {
                            ++p;
                        } else {
                            ++q;
                        }
                    }
                }
                if (F.val[pd] == 0.0) atomicMin(status, i);
            } else {                                           // MK_ILU_FACT_IC
                // l_ik = (a_ik - sum_{j<k} l_ij l_kj) / l_kk over the stored j of both rows; l_ii = sqrt(a_ii - sum l_ij^2)
                const int p0 = F.indptr[i], pd = F.diag[i];
                for (int pk = p0; pk < pd; ++pk) {
                    const int k = F.indices[pk];
                    const int dk = F.diag[k];
                    double s = F.val[pk];
                    int p = p0, q = F.indptr[k];
                    while (p < pk && q < dk) {
                        const int cj = F.indices[p], ck = F.indices[q];
                        if (cj == ck) {
                            s = s - F.val[p] * F.val[q];
                            ++p;
                            ++q;
                        } else if (cj < ck) {
                            ++p;
                        } else {
                            ++q;
                        }
                    }
                    F.val[pk] = s / F.val[dk];
                }
                double d = F.val[pd];
                for (int p = p0; p < pd; ++p) d = d - F.val[p] * F.val[p];
                if (!(d > 0.0)) atomicMin(status, i);
                F.val[pd] = sqrt(d);
            }
        }
        if (L + 1 < nl) __syncthreads();                       // the next level reads what this one wrote (same workgroup)
    }
}

// IC(0): the upper positions take the values of their mirrored lower ones (U = L^T)
__global__ __launch_bounds__(MK_BLOCK) void mk_ilu_mirror_kernel(double *val, const int32_t *tmap, int64_t nnz) {
    for (int64_t p = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * MK_BLOCK) {
        const int32_t t = tmap[p];
        if (t >= 0) val[p] = val[t];
    }
}

__global__ void mk_ilu_status_init(int *status) {
    if (threadIdx.x == 0) *status = INT_MAX;
}

static MkIluView mk_ilu_view(const mk_ilu *F, const MkIluSweep &S) {
    return MkIluView{F->A->d_indptr, F->A->d_indices, F->d_diag, S.d_rows, S.d_lev, F->d_val};
}

// every launch of one sweep; `q` = the solver's kernel counter (halt parity), or null for a standalone run
template <int MODE>
static void mk_ilu_sweep(const mk_ilu *F, const MkIluSweep &S, const double *in, double *out, hipStream_t st, int *flags,
                         int64_t *q) {
    const MkIluView v = mk_ilu_view(F, S);
    for (const MkIluLaunch &l : S.plan) {
        hipLaunchKernelGGL(mk_ilu_kernel<MODE>, dim3(l.grid), dim3(MK_BLOCK), 0, st, v, l.lev0, l.lev1, in, out,
                           F->d_status, F->halt(flags, q));
    }
}

// out = M^-1 in (in == out allowed).  Used by mk_ilu_apply and by the solver's preconditioner sites (mk_solver.hip).
int mk_ilu::enqueue(const double *in, double *out, hipStream_t st, int *flags, int64_t *q) const {
    if (n == 0) return MK_OK;
    if (kind == 0) mk_ilu_sweep<MK_ILU_FWD>(this, fw, in, out, st, flags, q);
    else mk_ilu_sweep<MK_ILU_FWD_DIV>(this, fw, in, out, st, flags, q);
    mk_ilu_sweep<MK_ILU_BWD>(this, bw, out, out, st, flags, q);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

mk_ilu::~mk_ilu() {
    if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
    hipFree(d_val);
    hipFree(d_diag);
    hipFree(fw.d_rows);
    hipFree(fw.d_lev);
    hipFree(bw.d_rows);
    hipFree(bw.d_lev);
    hipFree(d_status);
    if (A) mk_release_operand(A);
}

// ------------------------------------------------------------------ host analysis
// levels of one sweep: lev(i) = 1 + max lev(k) over the stored k on the sweep's side of the diagonal (forward: k < i,
// rows ascending; backward: k > i, rows descending); rows listed by level, then by row
static void mk_ilu_levels(const std::vector<int32_t> &ip, const std::vector<int32_t> &ix, const std::vector<int32_t> &dg,
                          bool forward, std::vector<int32_t> &rows, std::vector<int32_t> &off) {
    const int64_t n = (int64_t)dg.size();
    std::vector<int32_t> lev((size_t)n);
    int32_t top = 0;
    for (int64_t s = 0; s < n; ++s) {
        const int64_t i = forward ? s : n - 1 - s;
        int32_t m = 0;
        if (forward) {
            for (int32_t p = ip[i]; p < dg[i]; ++p) m = lev[ix[p]] > m ? lev[ix[p]] : m;
        } else {
            for (int32_t p = dg[i] + 1; p < ip[i + 1]; ++p) m = lev[ix[p]] > m ? lev[ix[p]] : m;
        }
        lev[i] = m + 1;
        top = lev[i] > top ? lev[i] : top;
    }
    off.assign((size_t)top + 1, 0);                              // level L (1-based) -> off[L - 1] .. off[L]
    for (int64_t i = 0; i < n; ++i) off[lev[i]] += 1;
    for (int32_t L = 1; L <= top; ++L) off[L] += off[L - 1];
    rows.resize((size_t)n);
    std::vector<int32_t> pos(off.begin(), off.end() - 1);
    for (int64_t i = 0; i < n; ++i) rows[pos[lev[i] - 1]++] = (int32_t)i;
}

static void mk_ilu_plan(MkIluSweep &S, const std::vector<int32_t> &off, int fuse) {
    S.levels = (int)off.size() - 1;
    S.widest = 0;
    S.plan.clear();
    int L = 0;
    while (L < S.levels) {
        const int64_t cnt = off[L + 1] - off[L];
        S.widest = cnt > S.widest ? cnt : S.widest;
        if (fuse > 0 && cnt <= fuse) {                           // a run of thin levels: one workgroup
            int e = L + 1;
            while (e < S.levels && e - L < MK_ILU_RUN_MAX && off[e + 1] - off[e] <= fuse) {
                S.widest = (off[e + 1] - off[e]) > S.widest ? off[e + 1] - off[e] : S.widest;
                ++e;
            }
            S.plan.push_back({L, e, 1});
            L = e;
        } else {
            const int64_t g = (cnt + MK_BLOCK - 1) / MK_BLOCK;
            S.plan.push_back({L, L + 1, (int)(g > 0 ? g : 1)});
            ++L;
        }
    }
}

template <class T>
static int mk_ilu_upload(T **dst, const std::vector<T> &src, size_t *bytes) {
    const size_t b = sizeof(T) * (src.size() > 0 ? src.size() : 1);
    MK_HIP(hipMalloc((void **)dst, b));
    if (!src.empty()) MK_HIP(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    *bytes += b;
    return MK_OK;
}

static int mk_ilu_create(const mk_csr *A, int kind, mk_ilu **out) {
    MK_REQUIRE_INIT();
    MK_ARG(A && out);
    const char *fn = kind ? "mk_ic0_create" : "mk_ilu0_create";
    if (A->comp_kind || A->host_fn || A->alias || A->nops)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator holds no CSR arrays of its own (a composite, reduced, block, "
                       "composed or matrix-free operator): form its matrix with to_csr_arrays() and a CsrOperator to "
                       "factor it", fn);
    if (A->ex.mode >= 0 || A->row_block)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: the operator is row-partitioned (it carries an exchange plan); the "
                       "factorizations are single-GPU", fn);
    if (A->nrows != A->ncols)
        return mk_fail(MK_ERR_ARG, "%s: the matrix must be square, got %lld x %lld", fn, (long long)A->nrows,
                       (long long)A->ncols);
    if (A->nnz >= ((int64_t)1 << 31))
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: %lld nonzeros; the factor's positions are 32-bit (< 2^31)", fn,
                       (long long)A->nnz);
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = A->nrows, nnz = A->nnz;
    std::vector<int32_t> ip((size_t)n + 1), ix((size_t)(nnz > 0 ? nnz : 1));
    MkContext &c = mk_ctx();
    MK_HIP(hipStreamSynchronize(c.stream));
    MK_HIP(hipMemcpy(ip.data(), A->d_indptr, sizeof(int32_t) * (size_t)(n + 1), hipMemcpyDeviceToHost));
    if (nnz > 0) MK_HIP(hipMemcpy(ix.data(), A->d_indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost));
    std::vector<int32_t> dg((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        int32_t p = ip[i];
        while (p < ip[i + 1] && ix[p] < i) ++p;
        if (p == ip[i + 1] || ix[p] != i)
            return mk_fail(MK_ERR_ARG, "%s: row %lld stores no diagonal entry (every row must store its diagonal)", fn,
                           (long long)i);
        dg[i] = p;
    }
    std::vector<int32_t> tmap;
    if (kind) {                                                  // IC(0): upper position -> its mirrored lower position
        tmap.assign((size_t)(nnz > 0 ? nnz : 1), -1);
        for (int64_t i = 0; i < n; ++i)
            for (int32_t p = dg[i] + 1; p < ip[i + 1]; ++p) {
                const int32_t j = ix[p];
                const int32_t *b = ix.data() + ip[j], *e = ix.data() + dg[j];
                const int32_t *f = std::lower_bound(b, e, (int32_t)i);
                if (f == e || *f != i)
                    return mk_fail(MK_ERR_ARG, "%s: the pattern is not symmetric: (%lld, %lld) is stored, (%lld, %lld) is "
                                   "not", fn, (long long)i, (long long)j, (long long)j, (long long)i);
                tmap[p] = (int32_t)(f - ix.data());
            }
        int64_t lower = 0, upper = 0;                            // (i, j) -> (j, i) is one to one: equal counts make it onto
        for (int64_t i = 0; i < n; ++i) {
            lower += dg[i] - ip[i];
            upper += ip[i + 1] - dg[i] - 1;
        }
        if (lower != upper)
            return mk_fail(MK_ERR_ARG, "%s: the pattern is not symmetric (%lld entries below the diagonal, %lld above)", fn,
                           (long long)lower, (long long)upper);
    }
    mk_ilu *F = new mk_ilu();
    F->kind = kind;
    F->n = n;
    F->nnz = nnz;
    static_assert(mk_switch_table[MK_SW_ILU_FUSE_ROWS].dflt == MK_ILU_FUSE_DEFAULT, "one default");
    F->fuse = (int)mk_switch_int<MK_SW_ILU_FUSE_ROWS>();     // (read at every creation: tests switch it)
    std::vector<int32_t> rows_f, off_f, rows_b, off_b;
    mk_ilu_levels(ip, ix, dg, true, rows_f, off_f);
    mk_ilu_levels(ip, ix, dg, false, rows_b, off_b);
    mk_ilu_plan(F->fw, off_f, F->fuse);
    mk_ilu_plan(F->bw, off_b, F->fuse);
    F->A = A;
    A->dependents += 1;
    int32_t *d_tmap = nullptr;
    size_t tbytes = 0;
    int rc = MK_OK;
    const auto fail = [&](int code) {
        hipFree(d_tmap);
        delete F;
        return code;
    };
    if ((rc = mk_ilu_upload(&F->d_diag, dg, &F->bytes)) != MK_OK || (rc = mk_ilu_upload(&F->fw.d_rows, rows_f, &F->bytes)) != MK_OK ||
        (rc = mk_ilu_upload(&F->fw.d_lev, off_f, &F->bytes)) != MK_OK ||
        (rc = mk_ilu_upload(&F->bw.d_rows, rows_b, &F->bytes)) != MK_OK ||
        (rc = mk_ilu_upload(&F->bw.d_lev, off_b, &F->bytes)) != MK_OK || (kind && (rc = mk_ilu_upload(&d_tmap, tmap, &tbytes)) != MK_OK))
        return fail(rc);
    const size_t vbytes = sizeof(double) * (size_t)(nnz + MK_CSR_PAD);
    if (hipMalloc((void **)&F->d_val, vbytes) != hipSuccess || hipMalloc((void **)&F->d_status, sizeof(int)) != hipSuccess)
        return fail(mk_fail(MK_ERR_HIP, "%s: out of device memory for the factor", fn));
    if ((rc = F->init_nohalt(c.stream)) != MK_OK) return fail(rc);
    F->bytes += vbytes + 3 * sizeof(int);                        // (the status word and the two halt words)
    const auto t1 = std::chrono::steady_clock::now();
    F->analysis_us = std::chrono::duration<double, std::micro>(t1 - t0).count();
    // factorization: the values of A, then one launch per forward level (or fused run) in level order
    if (hipMemcpyAsync(F->d_val, A->d_data, sizeof(double) * (size_t)(nnz + MK_CSR_PAD), hipMemcpyDeviceToDevice, c.stream) != hipSuccess)
        return fail(mk_fail(MK_ERR_HIP, "%s: copying the matrix values failed", fn));
    hipLaunchKernelGGL(mk_ilu_status_init, dim3(1), dim3(64), 0, c.stream, F->d_status);
    if (kind) mk_ilu_sweep<MK_ILU_FACT_IC>(F, F->fw, nullptr, nullptr, c.stream, nullptr, nullptr);
    else mk_ilu_sweep<MK_ILU_FACT>(F, F->fw, nullptr, nullptr, c.stream, nullptr, nullptr);
    if (kind && nnz > 0) {
        int64_t g = (nnz + MK_BLOCK - 1) / MK_BLOCK;
        hipLaunchKernelGGL(mk_ilu_mirror_kernel, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(MK_BLOCK), 0, c.stream, F->d_val,
                           d_tmap, nnz);
    }
    int bad = INT_MAX;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, F->d_status, sizeof(int), hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
        hipStreamSynchronize(c.stream) != hipSuccess)
        return fail(mk_fail(MK_ERR_HIP, "%s: the factorization kernels failed", fn));
    F->factor_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count();
    hipFree(d_tmap);
    d_tmap = nullptr;
    if (bad != INT_MAX) {
        delete F;
        return kind ? mk_fail(MK_ERR_STATE, "%s: breakdown in row %d (the pivot is not positive)", fn, bad)
                    : mk_fail(MK_ERR_STATE, "%s: zero pivot in row %d", fn, bad);
    }
    *out = F;
    return MK_OK;
}

// ======================================================================================
// C ABI
// ======================================================================================
extern "C" int mk_ilu0_create(const mk_csr *A, mk_ilu **out) { return mk_ilu_create(A, 0, out); }

extern "C" int mk_ic0_create(const mk_csr *A, mk_ilu **out) { return mk_ilu_create(A, 1, out); }

extern "C" int mk_ilu_destroy(mk_ilu *F) {
    if (F) F->destroy();                                         // (while solvers still apply it: freed with the last of them)
    return MK_OK;
}

extern "C" int mk_solver_set_precon_ilu(mk_solver *s, const mk_ilu *F) {
    return mk_set_precon(s, -1, MkPrecon::object(F), "mk_solver_set_precon_ilu");
}

extern "C" int mk_solver_set_lls_precon_ilu(mk_solver *s, int side, const mk_ilu *F) {
    return mk_set_precon(s, side, MkPrecon::object(F), "mk_solver_set_lls_precon_ilu");
}

extern "C" int mk_ilu_apply(const mk_ilu *F, const double *in_dev, double *out_dev) {
    return MkDeviceOp::apply_standalone(F, in_dev, out_dev);
}

extern "C" int mk_ilu_info(const mk_ilu *F, int64_t *info, int32_t cap) {
    MK_ARG(F && (cap <= 0 || info));
    const int64_t v[MK_ILU_INFO_LEN] = {F->kind,
                                        F->n,
                                        F->nnz,
                                        F->fw.levels,
                                        F->bw.levels,
                                        (int64_t)F->fw.plan.size(),
                                        (int64_t)F->bw.plan.size(),
                                        F->fw.widest > F->bw.widest ? F->fw.widest : F->bw.widest,
                                        (int64_t)F->bytes,
                                        F->fuse,
                                        (int64_t)llround(F->analysis_us),
                                        (int64_t)llround(F->factor_us)};
    for (int32_t k = 0; k < cap && k < MK_ILU_INFO_LEN; ++k) info[k] = v[k];
    return MK_OK;
}

extern "C" int mk_ilu_download(const mk_ilu *F, double *values_host, int32_t *diag_host) {
    MK_ARG(F);
    MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    if (values_host && F->nnz > 0)
        MK_HIP(hipMemcpy(values_host, F->d_val, sizeof(double) * (size_t)F->nnz, hipMemcpyDeviceToHost));
    if (diag_host && F->n > 0) MK_HIP(hipMemcpy(diag_host, F->d_diag, sizeof(int32_t) * (size_t)F->n, hipMemcpyDeviceToHost));
    return MK_OK;
}
