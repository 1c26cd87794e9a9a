// mk_multicol.h -- stream ops over several stored columns per launch, shared by the solvers that keep blocks of vectors
// (GMRES' basis, mk_gmres.hip; IDR's P, G and U, mk_idr.hip).  A launch takes GM_GROUP columns, so that the vector they are
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
#endif
