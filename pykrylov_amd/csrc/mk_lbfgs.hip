// mk_lbfgs.hip -- limited-memory BFGS operators resident in HBM (reference pykrylov/linop/lbfgs.py).
//
// The object keeps two rings of `npairs` columns (S, Y; column k at k * ld, ld = n rounded up to even: 16-byte aligned
// columns), the scalars ys[k], alpha[k] and gamma in device memory, its OWN partial-sum slots (an apply runs between the
// kernels of a solver, whose partial sums may still be pending) and, on the host, the Gram entries s_k.s_l and s_k.y_l
// that the compact forward form needs (computed once, when pair k is stored).  Slots fill from 0 and a rejected pair does
// not advance `insert`, so the stored pairs are always the slots 0 .. count-1 and oldest to newest is
// (insert - count + i) mod npairs.
//
//   apply (lbfgs.py:97-127)  the two-loop recursion as a chain of 2p + 1 mk_stream_kernel launches over the working vector
//                            `out`: every launch totals the previous launch's partial sums in its prologue (alpha_k or
//                            beta), applies that update to its pair of elements and accumulates the next dot in the same
//                            sweep.  The scalars never leave the device.
//   multi-dot                one vector against up to MK_LBFGS_GROUP columns per launch; every dot with the lane assignment,
//                            grid rule and reduction tree of mk_stream_kernel<MkOpDot>, then mk_total.
//   combine (lbfgs.py:249-252)  r = v / gamma; r -= (b_i / gamma) s_k; r -= b_{p+i} y_k: one read of v, one write of out.
#include <cmath>
#include <limits>

#include "mk_solver.h"

constexpr int MK_LBFGS_GROUP = 8;                     // columns of one multi-dot launch (their accumulators stay in registers)
constexpr int MK_LBFGS_SLOTS = 2 + MK_LBFGS_GROUP;    // partial-sum slots: 0 / 1 the apply chain, 2 .. the multi-dot

struct mk_lbfgs : MkDeviceOp {
    int64_t ld = 0;
    int npairs = 0, scaling = 0;
    double *d_S = nullptr, *d_Y = nullptr;     // the rings: npairs columns of ld doubles each
    double *d_sc = nullptr;                    // ys[npairs], alpha[npairs], gamma
    double *d_part = nullptr;                  // MK_LBFGS_SLOTS * MK_MAXP partial sums of its own
    double *d_res = nullptr;                   // totals of a multi-dot (2 npairs + 3)
    double *d_coef = nullptr;                  // coefficients of a combine (2 npairs)
    // host mirror of what `store` decided (store synchronises; it is not inside any loop)
    std::vector<double> ys, yy;                // s_k.y_k, y_k.y_k per slot
    std::vector<double> ss, sy;                // Gram caches by slot, row major: ss[k][l] = s_k.s_l, sy[k][l] = s_k.y_l (k newer than l)
    int insert = 0, count = 0;
    double gamma = 1.0;                        // ys_last / yy_last when scaling is on and a pair is stored, else 1
    int64_t stores = 0, rejected = 0;
    size_t bytes = 0;
    mutable int64_t last_launches = 0, applies = 0;
    ~mk_lbfgs() override;
    const char *noun() const override { return "L-BFGS operator"; }
    int enqueue(const double *in, double *out, hipStream_t stream, int *flags, int64_t *q) const override;
    const double *S(int k) const { return d_S + (size_t)k * (size_t)ld; }
    const double *Y(int k) const { return d_Y + (size_t)k * (size_t)ld; }
    int oldest(int i) const { return ((insert - count + i) % npairs + npairs) % npairs; }   // i-th stored pair, oldest first
};

// ------------------------------------------------------------------ the apply chain
enum { MK_LB_FIRST = 0, MK_LB_LOOP1 = 1, MK_LB_TURN = 2, MK_LB_LOOP2 = 3, MK_LB_LAST = 4 };

// One launch of the two-loop recursion.  `w` is the working vector (q, then r).  MODE:
//   FIRST  w = in;                                             acc += s_next . w      (lbfgs.py:104,112)
//   LOOP1  alpha_prev = tot / ys_prev;  w -= alpha_prev y_prev;  acc += s_next . w      (:112-113)
//   TURN   alpha_prev likewise;  w -= alpha_prev y_prev;  w *= gamma (scaling);  acc += y_prev . w   (:113,120,125)
//   LOOP2  beta = tot / ys_prev;  w += (alpha_prev - beta) s_prev;  acc += y_next . w   (:125-126)
//   LAST   beta likewise;  w += (alpha_prev - beta) s_prev                              (:126)
// tot = the previous launch's partial sums (slot SLOT ^ 1); this launch writes slot SLOT.
template <int MODE, int SLOT>
struct MkOpLbfgs {
    static constexpr int NACC = MODE == MK_LB_LAST ? 0 : 1, SLOT0 = SLOT;
    const double *part;
    int np;
    double *sc;
    int kprev, npairs, scale;
    const double *u;             // column of the update (y_prev / s_prev)
    const double *d;             // column of the dot (s_next / y_next; TURN: u again)
    const double *src;
    double *dst;
    double c, g;
    MkTotalRegs tr;
    double ys_in, al_in;
    __device__ void early() {
        if constexpr (MODE != MK_LB_FIRST) {
            mk_total_issue(part, np, tr);
            ys_in = sc[kprev];
            if constexpr (MODE == MK_LB_LOOP2 || MODE == MK_LB_LAST) al_in = sc[npairs + kprev];
            if constexpr (MODE == MK_LB_TURN) g = sc[2 * npairs];
        }
    }
    __device__ bool prologue(double *s4, bool lead) {
        if constexpr (MODE != MK_LB_FIRST) {
            const double t = mk_total_finish(tr, np, s4) / ys_in;
            if constexpr (MODE == MK_LB_LOOP1 || MODE == MK_LB_TURN) {
                c = t;                                        // alpha_k
                if (lead) sc[npairs + kprev] = t;
            } else {
                c = al_in - t;                                // alpha_k - beta
            }
        }
        return false;
    }
    __device__ bool skip() const { return false; }
    struct Regs {
        double2 w, uv, dv;
    };
    __device__ void load2(int64_t i, Regs &r) const {
        r.w = mk_ld2(src, i);
        if constexpr (MODE != MK_LB_FIRST) r.uv = mk_ld2(u, i);
        if constexpr (MODE == MK_LB_FIRST || MODE == MK_LB_LOOP1 || MODE == MK_LB_LOOP2) r.dv = mk_ld2(d, i);
    }
    __device__ double step(double w, double uv) const {
        if constexpr (MODE == MK_LB_LOOP1) w = w - c * uv;
        if constexpr (MODE == MK_LB_TURN) {
            w = w - c * uv;
            if (scale) w = w * g;
        }
        if constexpr (MODE == MK_LB_LOOP2 || MODE == MK_LB_LAST) w = w + c * uv;
        return w;
    }
    __device__ void apply2(Regs &r, double *acc) const {
        r.w.x = step(r.w.x, r.uv.x);
        r.w.y = step(r.w.y, r.uv.y);
        if constexpr (MODE == MK_LB_TURN) {
            acc[0] += r.uv.x * r.w.x;
            acc[0] += r.uv.y * r.w.y;
        } else if constexpr (MODE != MK_LB_LAST) {
            acc[0] += r.dv.x * r.w.x;
            acc[0] += r.dv.y * r.w.y;
        }
    }
    __device__ void store2(int64_t i, const Regs &r) const {
        if (MODE != MK_LB_FIRST || dst != src) mk_st2(dst, i, r.w);
    }
    __device__ void one(int64_t i, double *acc) {
        const double uv = MODE != MK_LB_FIRST ? u[i] : 0.0;
        const double w = step(src[i], uv);
        if (MODE != MK_LB_FIRST || dst != src) dst[i] = w;
        if constexpr (MODE == MK_LB_TURN) acc[0] += uv * w;
        else if constexpr (MODE != MK_LB_LAST) acc[0] += d[i] * w;
    }
};

template <int MODE, int SLOT>
static void mk_lbfgs_launch1(const mk_lbfgs *F, int kprev, const double *u, const double *d, const double *src, double *dst,
                             hipStream_t st, const MkHalt &h) {
    using Op = MkOpLbfgs<MODE, SLOT>;
    Op op{};
    op.np = mk_grid_stream(F->n);
    op.part = F->d_part + (size_t)(SLOT ^ 1) * MK_MAXP;
    op.sc = F->d_sc;
    op.kprev = kprev;
    op.npairs = F->npairs;
    op.scale = F->scaling;
    op.u = u;
    op.d = d;
    op.src = src;
    op.dst = dst;
    hipLaunchKernelGGL(mk_stream_kernel<Op>, dim3(op.np), dim3(MK_BLOCK), 0, st, op, F->n, h, F->d_part);
}

template <int MODE>
static void mk_lbfgs_launch(const mk_lbfgs *F, int j, int kprev, const double *u, const double *d, const double *src,
                            double *dst, hipStream_t st, const MkHalt &h) {
    if (j & 1) mk_lbfgs_launch1<MODE, 1>(F, kprev, u, d, src, dst, st, h);
    else mk_lbfgs_launch1<MODE, 0>(F, kprev, u, d, src, dst, st, h);
}

// out = H in by the two-loop recursion (in == out allowed): 2p + 1 launches for p stored pairs; with none a copy, or nothing
// when in == out.  `q` = the solver's kernel counter (each launch takes the halt word flags[(*q)++ & 1]), or null for a
// standalone run.  Used by mk_lbfgs_apply and by the solver's preconditioner sites (mk_solver.hip).
int mk_lbfgs::enqueue(const double *in, double *out, hipStream_t st, int *flags, int64_t *q) const {
    const mk_lbfgs *F = this;
    const auto halt = [&] { return F->halt(flags, q); };
    const int p = F->count;
    F->applies += 1;
    if (p == 0) {
        F->last_launches = 0;
        if (in != out) {
            hipLaunchKernelGGL(mk_stream_kernel<MkOpCopy>, dim3(mk_grid_stream(F->n)), dim3(MK_BLOCK), 0, st,
                               MkOpCopy{in, out}, F->n, halt(), F->d_part);
            F->last_launches = 1;
        }
        MK_HIP(hipGetLastError());
        return MK_OK;
    }
    const auto newest = [&](int i) { return F->oldest(p - 1 - i); };       // loop 1 walks newest -> oldest
    int j = 0;
    mk_lbfgs_launch<MK_LB_FIRST>(F, j, 0, nullptr, F->S(newest(0)), in, out, st, halt());
    for (j = 1; j < p; ++j) {
        const int kp = newest(j - 1);
        mk_lbfgs_launch<MK_LB_LOOP1>(F, j, kp, F->Y(kp), F->S(newest(j)), out, out, st, halt());
    }
    {
        const int kp = newest(p - 1);                                        // = oldest(0): last of loop 1, first of loop 2
        mk_lbfgs_launch<MK_LB_TURN>(F, j, kp, F->Y(kp), nullptr, out, out, st, halt());
        ++j;
    }
    for (int i = 1; i < p; ++i, ++j) {
        const int kp = F->oldest(i - 1);
        mk_lbfgs_launch<MK_LB_LOOP2>(F, j, kp, F->S(kp), F->Y(F->oldest(i)), out, out, st, halt());
    }
    {
        const int kp = F->oldest(p - 1);
        mk_lbfgs_launch<MK_LB_LAST>(F, j, kp, F->S(kp), nullptr, out, out, st, halt());
        ++j;
    }
    F->last_launches = j;
    MK_HIP(hipGetLastError());
    return MK_OK;
}

// ------------------------------------------------------------------ multi-dot
struct MkMultiDot {
    const double *a;             // the vector
    const double *b;             // a second vector, or null: then b = a / div (use_div) or a
    double div;
    int use_div;
    int ncol;
    unsigned selb;               // bit c: column c is multiplied with b instead of a
    const double *col[MK_LBFGS_GROUP];
};

// acc_c = sum (a or b)_i col_c,i for up to MK_LBFGS_GROUP columns with ONE read of a (and b): lane g of S lanes adds the
// elements 2q, 2q + 1 for q = g, g + S, ... in order, the odd tail goes to lane (n / 2) % S, then mk_block_sum -- per column
// exactly what mk_stream_kernel<MkOpDot> computes.  Partial sums into the slots 2 + c.
__global__ __launch_bounds__(MK_BLOCK) void mk_multidot_kernel(MkMultiDot M, int64_t n, double *__restrict__ partials) {
    __shared__ double s4[4];
    const int64_t S = (int64_t)gridDim.x * MK_BLOCK;
    const int64_t g = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
    const int64_t npair = n >> 1;
    double acc[MK_LBFGS_GROUP];
#pragma unroll
    for (int c = 0; c < MK_LBFGS_GROUP; ++c) acc[c] = 0.0;
    for (int64_t q = g; q < npair; q += S) {
        const double2 av = mk_ld2(M.a, 2 * q);
        double2 bv = av;
        if (M.b) bv = mk_ld2(M.b, 2 * q);
        double2 cv[MK_LBFGS_GROUP];
#pragma unroll
        for (int c = 0; c < MK_LBFGS_GROUP; ++c)
            if (c < M.ncol) cv[c] = mk_ld2(M.col[c], 2 * q);
        if (!M.b && M.use_div) {
            bv.x = av.x / M.div;
            bv.y = av.y / M.div;
        }
#pragma unroll
        for (int c = 0; c < MK_LBFGS_GROUP; ++c)
            if (c < M.ncol) {
                const double2 x = ((M.selb >> c) & 1u) ? bv : av;
                acc[c] += cv[c].x * x.x;
                acc[c] += cv[c].y * x.y;
            }
    }
    if ((n & 1) && g == (npair % S)) {
        const double a1 = M.a[n - 1];
        const double b1 = M.b ? M.b[n - 1] : (M.use_div ? a1 / M.div : a1);
#pragma unroll
        for (int c = 0; c < MK_LBFGS_GROUP; ++c)
            if (c < M.ncol) acc[c] += M.col[c][n - 1] * (((M.selb >> c) & 1u) ? b1 : a1);
    }
#pragma unroll
    for (int c = 0; c < MK_LBFGS_GROUP; ++c)
        if (c < M.ncol) {                                         // (launch uniform: every lane meets the barriers)
            const double tot = mk_block_sum(acc[c], s4);
            if (threadIdx.x == 0) partials[(2 + c) * MK_MAXP + blockIdx.x] = tot;
        }
}

// res[c] = mk_total of slot 2 + c (one workgroup)
__global__ __launch_bounds__(MK_BLOCK) void mk_lbfgs_total_kernel(const double *part, int np, int ncol, double *res) {
    __shared__ double s4[4];
    for (int c = 0; c < ncol; ++c) {
        const double t = mk_total(part + (size_t)(2 + c) * MK_MAXP, np, s4);
        if (threadIdx.x == 0) res[c] = t;
    }
}

struct MkDotCol {
    const double *col;
    int with_b;
};

// the dots of `a` (and `b`) with every column of `cols`, in groups of MK_LBFGS_GROUP, totals to the host
static int mk_lbfgs_multidot(const mk_lbfgs *F, const double *a, const double *b, double div, int use_div,
                             const std::vector<MkDotCol> &cols, double *res_host) {
    if (cols.empty()) return MK_OK;
    hipStream_t st = mk_ctx().stream;
    const int grid = mk_grid_stream(F->n);
    for (size_t c0 = 0; c0 < cols.size(); c0 += MK_LBFGS_GROUP) {
        MkMultiDot M{};
        M.a = a;
        M.b = b;
        M.div = div;
        M.use_div = use_div;
        M.ncol = (int)(cols.size() - c0 < (size_t)MK_LBFGS_GROUP ? cols.size() - c0 : (size_t)MK_LBFGS_GROUP);
        for (int c = 0; c < MK_LBFGS_GROUP; ++c) {
            M.col[c] = c < M.ncol ? cols[c0 + c].col : a;
            if (c < M.ncol && cols[c0 + c].with_b) M.selb |= 1u << c;
        }
        hipLaunchKernelGGL(mk_multidot_kernel, dim3(grid), dim3(MK_BLOCK), 0, st, M, F->n, F->d_part);
        hipLaunchKernelGGL(mk_lbfgs_total_kernel, dim3(1), dim3(MK_BLOCK), 0, st, F->d_part, grid, M.ncol, F->d_res + c0);
    }
    MK_HIP(hipGetLastError());
    MK_HIP(hipMemcpyAsync(res_host, F->d_res, sizeof(double) * cols.size(), hipMemcpyDeviceToHost, st));
    MK_HIP(hipStreamSynchronize(st));
    return MK_OK;
}

// ------------------------------------------------------------------ combine
// out = v / div (use_div), then for the stored pairs oldest to newest: out -= cs_i s_k; out -= cy_i y_k, every update a
// separate multiply and subtraction (lbfgs.py:249-252).  coef = {cs_0 .. cs_{p-1}, cy_0 .. cy_{p-1}}.
__global__ __launch_bounds__(MK_BLOCK) void mk_lbfgs_combine_kernel(const double *v, double *out, const double *Sr, const double *Yr,
                                                                   int64_t ld, int first, int p, int npairs,
                                                                   const double *__restrict__ coef, double div, int use_div,
                                                                   int64_t n) {
    const int64_t S = (int64_t)gridDim.x * MK_BLOCK;
    const int64_t g = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
    const int64_t npair = n >> 1;
    for (int64_t q = g; q < npair; q += S) {
        double2 r = mk_ld2(v, 2 * q);
        if (use_div) {
            r.x = r.x / div;
            r.y = r.y / div;
        }
        for (int i0 = 0; i0 < p; i0 += 4) {
            double2 sv[4], yv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (i0 + t < p) {
                    const size_t k = (size_t)((first + i0 + t) % npairs);
                    sv[t] = mk_ld2(Sr + k * (size_t)ld, 2 * q);
                    yv[t] = mk_ld2(Yr + k * (size_t)ld, 2 * q);
                }
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (i0 + t < p) {
                    const double cs = coef[i0 + t], cy = coef[p + i0 + t];
                    r.x = r.x - cs * sv[t].x;
                    r.y = r.y - cs * sv[t].y;
                    r.x = r.x - cy * yv[t].x;
                    r.y = r.y - cy * yv[t].y;
                }
        }
        mk_st2(out, 2 * q, r);
    }
    if ((n & 1) && g == (npair % S)) {
        double r = v[n - 1];
        if (use_div) r = r / div;
        for (int i = 0; i < p; ++i) {
            const size_t k = (size_t)((first + i) % npairs);
            r = r - coef[i] * Sr[k * (size_t)ld + (size_t)(n - 1)];
            r = r - coef[p + i] * Yr[k * (size_t)ld + (size_t)(n - 1)];
        }
        out[n - 1] = r;
    }
}

// ys[k] (NaN marks an empty slot for no reader: the stored slots are 0 .. count-1) and gamma, by one lane
__global__ void mk_lbfgs_set_kernel(double *sc, int k, double ys, int kg, double gamma) {
    if (threadIdx.x == 0) {
        if (k >= 0) sc[k] = ys;
        sc[kg] = gamma;
    }
}

// ------------------------------------------------------------------ lifetime
mk_lbfgs::~mk_lbfgs() {
    if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
    hipFree(d_S);
    hipFree(d_Y);
    hipFree(d_sc);
    hipFree(d_part);
    hipFree(d_res);
    hipFree(d_coef);
}

// ======================================================================================
// C ABI
// ======================================================================================
extern "C" int mk_lbfgs_create(int64_t n, int32_t npairs, int32_t scaling, mk_lbfgs **out) {
    MK_REQUIRE_INIT();
    MK_ARG(out != nullptr);
    if (n < 1) return mk_fail(MK_ERR_ARG, "mk_lbfgs_create: n must be at least 1, got %lld", (long long)n);
    if (npairs < 1 || npairs > MK_LBFGS_MAX_PAIRS)
        return mk_fail(MK_ERR_ARG, "mk_lbfgs_create: npairs must be in 1 .. %d, got %d", MK_LBFGS_MAX_PAIRS, (int)npairs);
    mk_lbfgs *F = new mk_lbfgs();
    F->n = n;
    F->ld = (n + 1) & ~(int64_t)1;
    F->npairs = npairs;
    F->scaling = scaling ? 1 : 0;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    F->ys.assign((size_t)npairs, nan);
    F->yy.assign((size_t)npairs, nan);
    F->ss.assign((size_t)npairs * npairs, nan);
    F->sy.assign((size_t)npairs * npairs, nan);
    const size_t ring = sizeof(double) * (size_t)npairs * (size_t)F->ld;
    const size_t nsc = sizeof(double) * (size_t)(2 * npairs + 2), npart = sizeof(double) * MK_LBFGS_SLOTS * MK_MAXP;
    const size_t nres = sizeof(double) * (size_t)(2 * npairs + 4);
    if (hipMalloc((void **)&F->d_S, ring) != hipSuccess || hipMalloc((void **)&F->d_Y, ring) != hipSuccess ||
        hipMalloc((void **)&F->d_sc, nsc) != hipSuccess || hipMalloc((void **)&F->d_part, npart) != hipSuccess ||
        hipMalloc((void **)&F->d_res, nres) != hipSuccess || hipMalloc((void **)&F->d_coef, nres) != hipSuccess ||
        F->init_nohalt(mk_ctx().stream) != MK_OK) {
        (void)hipGetLastError();
        delete F;
        return mk_fail(MK_ERR_HIP, "mk_lbfgs_create: out of device memory for 2 x %d columns of %lld doubles", (int)npairs,
                       (long long)n);
    }
    F->bytes = 2 * ring + nsc + npart + 2 * nres + 2 * sizeof(int);   // (the last term: the two halt words)
    hipStream_t st = mk_ctx().stream;
    MK_HIP(hipMemsetAsync(F->d_S, 0, ring, st));                 // (empty slots download as zeros)
    MK_HIP(hipMemsetAsync(F->d_Y, 0, ring, st));
    MK_HIP(hipMemsetAsync(F->d_sc, 0, nsc, st));
    MK_HIP(hipMemsetAsync(F->d_part, 0, npart, st));
    hipLaunchKernelGGL(mk_lbfgs_set_kernel, dim3(1), dim3(64), 0, st, F->d_sc, -1, 0.0, 2 * npairs, 1.0);
    MK_HIP(hipGetLastError());
    *out = F;
    return MK_OK;
}

extern "C" int mk_lbfgs_destroy(mk_lbfgs *F) {
    if (F) F->destroy();                                         // (while solvers still apply it: freed with the last of them)
    return MK_OK;
}

extern "C" int mk_solver_set_precon_lbfgs(mk_solver *s, const mk_lbfgs *F) {
    return mk_set_precon(s, -1, MkPrecon::object(F), "mk_solver_set_precon_lbfgs");
}

extern "C" int mk_solver_set_lls_precon_bfgs(mk_solver *s, int side, const mk_lbfgs *F) {
    return mk_set_precon(s, side, MkPrecon::object(F), "mk_solver_set_lls_precon_bfgs");
}

extern "C" int mk_lbfgs_store(mk_lbfgs *F, const double *s_dev, const double *y_dev, double threshold, int32_t *accepted) {
    MK_REQUIRE_INIT();
    MK_ARG(F && s_dev && y_dev);
    MK_ARG(MK_ALIGNED16(s_dev) && MK_ALIGNED16(y_dev));
    // one read of the new pair: s.y, y.y, s.s and the new row of the Gram caches (s against every column that stays)
    const int ins = F->insert, np = F->npairs;
    std::vector<MkDotCol> cols = {{y_dev, 0}, {y_dev, 1}, {s_dev, 0}};
    std::vector<int> slots;
    for (int l = 0; l < F->count; ++l)
        if (l != ins) {
            slots.push_back(l);
            cols.push_back({F->S(l), 0});
            cols.push_back({F->Y(l), 0});
        }
    std::vector<double> res(cols.size());
    const int rc = mk_lbfgs_multidot(F, s_dev, y_dev, 1.0, 0, cols, res.data());
    if (rc != MK_OK) return rc;
    const double ys = res[0];
    if (ys <= threshold) {                                       // lbfgs.py:78-80
        F->rejected += 1;
        if (accepted) *accepted = 0;
        return MK_OK;
    }
    hipStream_t st = mk_ctx().stream;
    const size_t col = sizeof(double) * (size_t)F->n;
    MK_HIP(hipMemcpyAsync(const_cast<double *>(F->S(ins)), s_dev, col, hipMemcpyDeviceToDevice, st));   // lbfgs.py:83-84
    MK_HIP(hipMemcpyAsync(const_cast<double *>(F->Y(ins)), y_dev, col, hipMemcpyDeviceToDevice, st));
    F->ys[ins] = ys;                                             // lbfgs.py:85
    F->yy[ins] = res[1];
    F->ss[(size_t)ins * np + ins] = res[2];
    for (size_t t = 0; t < slots.size(); ++t) {
        F->ss[(size_t)ins * np + slots[t]] = res[3 + 2 * t];
        F->sy[(size_t)ins * np + slots[t]] = res[4 + 2 * t];
    }
    if (F->count < np) F->count += 1;
    F->insert = (ins + 1) % np;                                  // lbfgs.py:86-87
    F->gamma = F->scaling ? ys / res[1] : 1.0;                   // lbfgs.py:119 (the newest pair's)
    hipLaunchKernelGGL(mk_lbfgs_set_kernel, dim3(1), dim3(64), 0, st, F->d_sc, ins, ys, 2 * np, F->gamma);
    MK_HIP(hipGetLastError());
    MK_HIP(hipStreamSynchronize(st));                            // (the caller may free or overwrite s_dev / y_dev now)
    F->stores += 1;
    if (accepted) *accepted = 1;
    return MK_OK;
}

extern "C" int mk_lbfgs_restart(mk_lbfgs *F) {
    MK_REQUIRE_INIT();
    MK_ARG(F != nullptr);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    F->ys.assign(F->ys.size(), nan);                             // lbfgs.py:91-94
    F->yy.assign(F->yy.size(), nan);
    F->ss.assign(F->ss.size(), nan);
    F->sy.assign(F->sy.size(), nan);
    F->insert = 0;
    F->count = 0;
    F->gamma = 1.0;
    hipLaunchKernelGGL(mk_lbfgs_set_kernel, dim3(1), dim3(64), 0, mk_ctx().stream, F->d_sc, -1, 0.0, 2 * F->npairs, 1.0);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

extern "C" int mk_lbfgs_apply(const mk_lbfgs *F, const double *in_dev, double *out_dev) {
    return MkDeviceOp::apply_standalone(F, in_dev, out_dev);
}

extern "C" int mk_lbfgs_forward_dots(const mk_lbfgs *F, const double *in_dev, int32_t use_gamma, double *a_host) {
    MK_REQUIRE_INIT();
    MK_ARG(F && in_dev && (F->count == 0 || a_host));
    MK_ARG(MK_ALIGNED16(in_dev));
    std::vector<MkDotCol> cols;
    for (int i = 0; i < F->count; ++i) cols.push_back({F->S(F->oldest(i)), 1});      // (v / gamma) . s_k   lbfgs.py:211,217
    for (int i = 0; i < F->count; ++i) cols.push_back({F->Y(F->oldest(i)), 0});      // v . y_k             lbfgs.py:224
    const double g = use_gamma ? F->gamma : 1.0;
    return mk_lbfgs_multidot(F, in_dev, nullptr, g, g != 1.0, cols, a_host);          // (x / 1.0 == x: the division is skipped)
}

extern "C" int mk_lbfgs_forward_combine(const mk_lbfgs *F, const double *in_dev, int32_t use_gamma, const double *coef_host,
                                        double *out_dev) {
    MK_REQUIRE_INIT();
    MK_ARG(F && in_dev && out_dev && (F->count == 0 || coef_host));
    MK_ARG(MK_ALIGNED16(in_dev) && MK_ALIGNED16(out_dev));
    const int p = F->count;
    const double g = use_gamma ? F->gamma : 1.0;
    hipStream_t st = mk_ctx().stream;
    if (p > 0) {
        std::vector<double> coef((size_t)2 * p);
        for (int i = 0; i < p; ++i) {
            coef[i] = coef_host[i] / g;                          // lbfgs.py:251
            coef[p + i] = coef_host[p + i];                      // lbfgs.py:252
        }
        MK_HIP(hipMemcpyAsync(F->d_coef, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice, st));
        MK_HIP(hipStreamSynchronize(st));                        // (`coef` leaves scope)
    }
    hipLaunchKernelGGL(mk_lbfgs_combine_kernel, dim3(mk_grid_stream(F->n)), dim3(MK_BLOCK), 0, st, in_dev, out_dev, F->d_S,
                       F->d_Y, F->ld, F->oldest(0), p, F->npairs, F->d_coef, g, (int)(g != 1.0), F->n);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

extern "C" int mk_lbfgs_gram(const mk_lbfgs *F, double *ss_host, double *sy_host, double *ys_host, double *yy_host) {
    MK_ARG(F != nullptr);
    const size_t np = (size_t)F->npairs;
    if (ss_host) memcpy(ss_host, F->ss.data(), sizeof(double) * np * np);
    if (sy_host) memcpy(sy_host, F->sy.data(), sizeof(double) * np * np);
    if (ys_host) memcpy(ys_host, F->ys.data(), sizeof(double) * np);
    if (yy_host) memcpy(yy_host, F->yy.data(), sizeof(double) * np);
    return MK_OK;
}

extern "C" int mk_lbfgs_info(const mk_lbfgs *F, int64_t *info, int32_t cap) {
    MK_ARG(F && (cap <= 0 || info));
    const int64_t v[MK_LBFGS_INFO_LEN] = {F->n,      F->npairs,        F->scaling,  F->insert,  F->count,           F->last_launches,
                                          F->applies, F->stores,        F->rejected, (int64_t)F->bytes, F->ld, MK_LBFGS_MAX_PAIRS};
    for (int32_t k = 0; k < cap && k < MK_LBFGS_INFO_LEN; ++k) info[k] = v[k];
    return MK_OK;
}

extern "C" int mk_lbfgs_download(const mk_lbfgs *F, double *s_host, double *y_host) {
    MK_REQUIRE_INIT();
    MK_ARG(F != nullptr);
    MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    const size_t col = sizeof(double) * (size_t)F->n;
    for (int k = 0; k < F->npairs; ++k) {                        // slot k -> row k of an (npairs, n) array
        if (s_host) MK_HIP(hipMemcpy(s_host + (size_t)k * (size_t)F->n, F->S(k), col, hipMemcpyDeviceToHost));
        if (y_host) MK_HIP(hipMemcpy(y_host + (size_t)k * (size_t)F->n, F->Y(k), col, hipMemcpyDeviceToHost));
    }
    return MK_OK;
}
