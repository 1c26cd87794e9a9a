// mk_rotate.h -- what the eigensolvers share at the end of a cycle or an iteration (thick-restart Lanczos, mk_trlan.hip;
// LOBPCG, mk_lobpcg.hip): the rotation kernel W = V Y of a block of stored columns, and the host solver of the small symmetric
// eigenproblem.  Both are restated operation by operation in tests/_trlan_ref.py (rotate, jacobi_eigh).
#pragma once
#include <algorithm>
#include <cmath>

#include "mk_solver.h"

constexpr int TR_MAXM = MK_TRLAN_MAX_NCV;                    // rows of a rotation's coefficient block (columns of V read)
constexpr int TR_SWEEPS = 30;

#ifdef __HIPCC__
// R: W[:, j] = sum_c Y[c, j] V[:, c] for the nj <= NJ columns of one group, from +0.0, c ascending, each term a multiply and
// an add.  Y (m x NJ, zero beyond nj) is staged in LDS once per workgroup and read as a broadcast; lane g of the grid owns
// the row pairs g, g + S, ... as the stream kernels do, the odd tail row goes to lane (n / 2) % S.  W may be columns of V:
// a row's results are stored after the whole row has been read, by the only lane that touches it.
template <int NJ>
__global__ __launch_bounds__(MK_BLOCK) void tr_rotate_kernel(const double *V, int64_t ld, int m, const double *__restrict__ Y,
                                                             int nj, double *W, int64_t n) {
    __shared__ double y[TR_MAXM * NJ];
    for (int k = (int)threadIdx.x; k < m * NJ; k += MK_BLOCK) y[k] = Y[k];
    __syncthreads();
    const int64_t S = (int64_t)gridDim.x * MK_BLOCK;
    const int64_t g = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
    const int64_t npair = n >> 1;
    for (int64_t q = g; q < npair; q += S) {
        double2 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = double2{0.0, 0.0};
        const double *vp = V + 2 * q;
#pragma unroll 4
        for (int c = 0; c < m; ++c) {
            const double2 v = *reinterpret_cast<const double2 *>(vp + (size_t)c * (size_t)ld);
            const double *yc = y + c * NJ;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const double f = yc[j];
                acc[j].x = acc[j].x + f * v.x;
                acc[j].y = acc[j].y + f * v.y;
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (j < nj) mk_st2(W + (size_t)j * (size_t)ld, 2 * q, acc[j]);
    }
    if ((n & 1) && g == (npair % S)) {
        double acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = 0.0;
        for (int c = 0; c < m; ++c) {
            const double v = V[(size_t)c * (size_t)ld + (size_t)(n - 1)];
            const double *yc = y + c * NJ;
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = acc[j] + yc[j] * v;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (j < nj) W[(size_t)j * (size_t)ld + (size_t)(n - 1)] = acc[j];
    }
}
#endif

// The small eigenproblem: cyclic Jacobi on the symmetric m x m matrix `a` (row major, both triangles kept), row-cyclic pairs
// (p, q), p < q, Rutishauser's formulas.  A pair whose entry is zero is skipped; an entry with g = 100 |a_pq| that changes
// neither |a_pp| nor |a_qq| when added to them is set to zero without a rotation.  Ends after a sweep without rotations;
// `s` (row major) gets the eigenvectors in its columns, `order` the columns by ascending eigenvalue, ties by index.  Returns
// the sweeps, or -1 after TR_SWEEPS sweeps that all rotated.  Restated operation by operation in tests/_trlan_ref.py
// (jacobi_eigh).
static inline int tr_jacobi(int m, double *a, double *s, int *order) {
    for (int i = 0; i < m; ++i)
        for (int k = 0; k < m; ++k) s[(size_t)i * m + k] = i == k ? 1.0 : 0.0;
    for (int sweep = 1; sweep <= TR_SWEEPS; ++sweep) {
        int rotations = 0;
        for (int p = 0; p < m - 1; ++p) {
            for (int q = p + 1; q < m; ++q) {
                const double apq = a[(size_t)p * m + q];
                if (apq == 0.0) continue;
                const double app = a[(size_t)p * m + p], aqq = a[(size_t)q * m + q];
                const double g = 100.0 * std::fabs(apq);
                if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
                    a[(size_t)p * m + q] = a[(size_t)q * m + p] = 0.0;
                    continue;
                }
                double h = aqq - app, t;
                if (std::fabs(h) + g == std::fabs(h)) {
                    t = apq / h;
                } else {
                    const double th = 0.5 * h / apq;
                    t = 1.0 / (std::fabs(th) + std::sqrt(1.0 + th * th));
                    if (th < 0.0) t = -t;
                }
                const double c = 1.0 / std::sqrt(1.0 + t * t);
                const double sn = t * c;
                const double tau = sn / (1.0 + c);
                h = t * apq;
                a[(size_t)p * m + p] = app - h;
                a[(size_t)q * m + q] = aqq + h;
                a[(size_t)p * m + q] = a[(size_t)q * m + p] = 0.0;
                for (int r = 0; r < m; ++r) {
                    if (r != p && r != q) {
                        const double gv = a[(size_t)r * m + p], hv = a[(size_t)r * m + q];
                        const double np_ = gv - sn * (hv + gv * tau), nq_ = hv + sn * (gv - hv * tau);
                        a[(size_t)r * m + p] = a[(size_t)p * m + r] = np_;
                        a[(size_t)r * m + q] = a[(size_t)q * m + r] = nq_;
                    }
                    const double gs = s[(size_t)r * m + p], hs = s[(size_t)r * m + q];
                    s[(size_t)r * m + p] = gs - sn * (hs + gs * tau);
                    s[(size_t)r * m + q] = hs + sn * (gs - hs * tau);
                }
                rotations += 1;
            }
        }
        if (rotations == 0) {
            for (int i = 0; i < m; ++i) order[i] = i;
            std::stable_sort(order, order + m, [&](int x, int y) { return a[(size_t)x * m + x] < a[(size_t)y * m + y]; });
            return sweep;
        }
    }
    return -1;
}
