// mk_multicol.h -- stream ops over several stored columns per launch, shared by the solvers that keep blocks of vectors
// (GMRES' basis, mk_gmres.hip; IDR's P, G and U, mk_idr.hip; the Lanczos basis of mk_trlan.hip; the two bases of mk_trsvd.hip).  A launch takes GM_GROUP columns, so that the vector they are
// taken against is read once per group instead of once per column.
#pragma once
#include "mk_solver.h"

#ifdef __HIPCC__
constexpr int GM_GROUP = 8;                         // columns per launch

struct GmCols {
    const double *col[GM_GROUP];
};

// Partial sums of <v_c, w> for the columns c0 .. c0 + ncol - 1 into the slots c0 + c of a bank (`partials` of the launch
// points at slot c0).  Per column the additions of MkOpDot in its order.
struct GmOpMultiDot {
    static constexpr int NACC = GM_GROUP, SLOT0 = 0;
    const double *w;
    GmCols v;
    int ncol;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        const double2 wv = mk_ld2(w, i);
        double2 cv[GM_GROUP];
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) cv[c] = mk_ld2(v.col[c], i);
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) {
                acc[c] += cv[c].x * wv.x;
                acc[c] += cv[c].y * wv.y;
            }
    }
    __device__ void one(int64_t i, double *acc) {
        const double wv = w[i];
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) acc[c] += v.col[c][i] * wv;
    }
};

// U: w = w - h_c v_c for the columns of one group, ascending, each term a multiply and a subtraction; h_c is the total of
// the group's slots in `bank`.  The lead lane files the coefficients in the column (`add`: on top of the first
// orthogonalisation's).  WW: <w, w> of the result goes into the slot `partials` of the launch points at.
template <bool WW>
struct GmOpUpdate {
    static constexpr int NACC = WW ? 1 : 0, SLOT0 = 0;
    const double *bank;          // at the group's first slot
    int np;
    double *h;                   // at the group's first coefficient
    int add;
    double *w;
    GmCols v;
    int ncol;
    double coef[GM_GROUP];
    __device__ bool prologue(double *s4, bool lead) {
        for (int c = 0; c < ncol; ++c) {                       // (launch uniform: every lane meets the barriers)
            coef[c] = mk_total(bank + (size_t)c * MK_MAXP, np, s4);
            if (lead) h[c] = add ? h[c] + coef[c] : coef[c];
        }
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        double2 wv = mk_ld2(w, i);
        double2 cv[GM_GROUP];
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) cv[c] = mk_ld2(v.col[c], i);
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) {
                wv.x = wv.x - coef[c] * cv[c].x;
                wv.y = wv.y - coef[c] * cv[c].y;
            }
        mk_st2(w, i, wv);
        if constexpr (WW) {
            acc[0] += wv.x * wv.x;
            acc[0] += wv.y * wv.y;
        }
    }
    __device__ void one(int64_t i, double *acc) {
        double wv = w[i];
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) wv = wv - coef[c] * v.col[c][i];
        w[i] = wv;
        if constexpr (WW) acc[0] += wv * wv;
    }
};

// A: U with given coefficients: w = w - y_c v_c for the columns of one group, ascending, each term a multiply and a
// subtraction, the y_c read from a device array (the arrow of a restarted bidiagonalisation: the first step of a one-sided
// cycle of mk_trsvd.hip).  WW: <w, w> of the result goes into the slot `partials` of the launch points at.
template <bool WW>
struct GmOpUpdateGiven {
    static constexpr int NACC = WW ? 1 : 0, SLOT0 = 0;
    const double *y;             // at the group's first coefficient
    double *w;
    GmCols v;
    int ncol;
    double coef[GM_GROUP];
    __device__ bool prologue(double *, bool) {
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c) coef[c] = c < ncol ? y[c] : 0.0;
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        double2 wv = mk_ld2(w, i);
        double2 cv[GM_GROUP];
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) cv[c] = mk_ld2(v.col[c], i);
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) {
                wv.x = wv.x - coef[c] * cv[c].x;
                wv.y = wv.y - coef[c] * cv[c].y;
            }
        mk_st2(w, i, wv);
        if constexpr (WW) {
            acc[0] += wv.x * wv.x;
            acc[0] += wv.y * wv.y;
        }
    }
    __device__ void one(int64_t i, double *acc) {
        double wv = w[i];
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) wv = wv - coef[c] * v.col[c][i];
        w[i] = wv;
        if constexpr (WW) acc[0] += wv * wv;
    }
};

// C: u = u + y_c v_c for the columns of one group, ascending (`first`: u starts from zero)
struct GmOpCombine {
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *y;             // at the group's first coefficient
    double *u;
    GmCols v;
    int ncol, first;
    double coef[GM_GROUP];
    __device__ bool prologue(double *, bool) {
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c) coef[c] = c < ncol ? y[c] : 0.0;
        return false;
    }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 uv{0.0, 0.0};
        if (!first) uv = mk_ld2(u, i);
        double2 cv[GM_GROUP];
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) cv[c] = mk_ld2(v.col[c], i);
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) {
                uv.x = uv.x + coef[c] * cv[c].x;
                uv.y = uv.y + coef[c] * cv[c].y;
            }
        mk_st2(u, i, uv);
    }
    __device__ void one(int64_t i, double *) {
        double uv = first ? 0.0 : u[i];
#pragma unroll
        for (int c = 0; c < GM_GROUP; ++c)
            if (c < ncol) uv = uv + coef[c] * v.col[c][i];
        u[i] = uv;
    }
};
#endif
