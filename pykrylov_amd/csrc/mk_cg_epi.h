// mk_cg_epi.h -- the product epilogue of the conjugate-gradient loops: Ap = A p with the partial sums of <p, Ap> formed in the
// row epilogue.  Shared by CG (mk_cg.hip) and PCG (mk_pcg.hip), so that both run the same product kernels in every storage
// format, with the same summation order.  The type stays in an unnamed namespace, as it was in mk_cg.hip: each unit
// instantiates the product kernels it launches, under the names they always had.
#pragma once
#include "mk_solver.h"

#ifdef __HIPCC__
namespace {

template <bool NTY>
struct CgSpmvEpiT {
    static constexpr int NACC = 1, SLOT0 = 0;
    static constexpr bool SYM_MARCH = true;                  // (CG's matrices are symmetric: format 11, mk_device.h MkSymMarch)
    const double *p;
    double *Ap;
    double pr;
    __device__ void prologue(double *) {}
    __device__ double xin(double v) const { return v; }
    __device__ void pre(int64_t r) { pr = p[r]; }          // issued at the top of the tile
    __device__ void row(int64_t r, double s, double *acc) {
        if constexpr (NTY) __builtin_nontemporal_store(s, Ap + r);
        else Ap[r] = s;
        acc[0] += pr * s;
    }
    // (NTY: the product vector goes past the caches -- mk_store_nt, mk_device.h)
    // p is the product's input vector: where the kernel has p[r] at hand (pattern format: the tile's LDS window) it
    // passes it instead of `pre` loading it again -- one stream of n doubles less per product
    __device__ void row_x(int64_t r, double s, double xr, double *acc) {
        if constexpr (NTY) __builtin_nontemporal_store(s, Ap + r);
        else Ap[r] = s;
        acc[0] += xr * s;
    }
    // the brick march on a general geometry (mk_spmv_fmt9.h, GEN): rows r, r + 1 where they exist -- a row that does not is
    // stored into the dump row and adds +0.0 (the running sum is never -0.0: unchanged bit for bit)
    __device__ void row2_m(int64_t r, mk_d2 s, mk_d2 xr, bool oka, bool okb, double *dump, double *acc) {
        mk_d2u *d = reinterpret_cast<mk_d2u *>(okb ? Ap + r : dump);
        if constexpr (NTY) __builtin_nontemporal_store(s, d);
        else *d = s;
        if (oka && !okb) Ap[r] = s.x;
        const double ta = xr.x * s.x, tb = xr.y * s.y;
        acc[0] += oka ? ta : 0.0;
        acc[0] += okb ? tb : 0.0;
    }
};
using CgSpmvEpi = CgSpmvEpiT<false>;

}  // namespace
#endif
