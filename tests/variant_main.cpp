// variant_main.cpp -- stand-alone host program for tests/test_variants.py: includes ONLY the library's variant header.
//   variant_main --table   one line per kernel variant: number storage min_blocks xw_alias carry gen
//   variant_main           the header against the rules it replaced, restated below as they stood in mk_device.h before the
//                          table existed (namespace old: the oracle, never the header), over a full sweep; prints the number of
//                          cases and every mismatch (exit status 1 if there is one)
#include <stdio.h>
#include <string.h>

#include "../pykrylov_amd/csrc/mk_variant.h"

namespace old {
constexpr int BLOCK = 256, SPMV_TILE = 2048, PROD_LDS = 8 * (BLOCK + 1);
constexpr int PEN_OCC = 2, PEN_RS = 132, PEN_LDS = 3 * 6 * PEN_RS + BLOCK, PEN_VB = 6 * 128 + 4 * PEN_RS, PEN_LDS_SYM = PEN_LDS + 2 * PEN_VB;

int min_blocks(int FMT) {
    return (FMT == 0 || FMT == 3 || FMT == 10) ? 8 : ((FMT >= 11 && FMT <= 16) ? PEN_OCC : ((FMT == 7 || FMT == 9) ? 4 : (FMT >= 4 ? 7 : 4)));
}
bool xw_alias(int FMT) { return FMT == 2 || (FMT >= 4 && FMT != 10); }
bool carry(int FMT) { return FMT == 10; }
bool fmt_march(int fmt) { return fmt >= 9 && fmt <= 11; }

struct View {
    int fmt, nt, rt_reg, tiles, pen_gen, wchunks, allwin, npat, pmax, rt_cap;
};
struct Flags {
    bool NM, SM, MO, PROG;                                   // MkNoMarch, MkSymMarch, MkMarchOnly of the epilogue; the row program
};
constexpr int ERROR = -1, NOTHING = -2;                      // the march-only error; a path that ends without a launch
struct Launch {
    int variant;
    size_t lds;
};
// the launcher's static_assert: instantiating it for such an epilogue does not compile
bool rejected(const Flags &f) { return f.MO && !(f.SM && !f.NM && !f.PROG); }

// mk_spmv_launch_fmt, every `if constexpr` as an `if` and every hipLaunchKernelGGL reduced to (template value, lds)
Launch launch(const View &v, const Flags &f) {
    size_t lds = sizeof(double) * (size_t)(PROD_LDS + (v.fmt == 1 ? 128 * v.wchunks + 2 : 0));
    if (v.fmt == 2) {
        const size_t w = sizeof(double) * (size_t)(128 * v.wchunks + 2) + sizeof(unsigned) * (SPMV_TILE + 16);
        lds = w > lds ? w : lds;
    }
    if (f.MO) {
        if (!fmt_march(v.fmt)) return {ERROR, 0};
    } else if (fmt_march(v.fmt) && (f.NM || ((v.fmt == 11 || v.pen_gen == 2) && !f.SM))) {
        return {0, lds};                                     // (w.fmt = 0)
    }
    if (fmt_march(v.fmt)) {
        if (f.SM) {
            if (v.pen_gen) {
                if (v.fmt == 9) {
                    lds = sizeof(double) * (size_t)PEN_LDS + 64 * (size_t)v.npat;
                    return {14, lds};
                } else if (v.fmt == 10) {
                    lds = sizeof(double) * (size_t)PEN_LDS;
                    return {15, lds};
                } else {
                    lds = sizeof(double) * (size_t)PEN_LDS_SYM;
                    return {16, lds};
                }
            }
        }
        if (!f.NM) {
            if (v.fmt == 9) {
                lds = sizeof(double) * (size_t)PEN_LDS + 64 * (size_t)v.npat;
                return {11, lds};
            } else if (v.fmt == 10) {
                lds = sizeof(double) * (size_t)PEN_LDS;
                return {12, lds};
            } else if (f.SM) {
                lds = sizeof(double) * (size_t)PEN_LDS_SYM;
                return {13, lds};
            }
        }
        return {NOTHING, 0};
    }
    if (!f.MO) {
        if (v.fmt == 4) {
            size_t wtop = (size_t)(128 * v.wchunks + 2);
            if (!v.allwin && wtop < (size_t)PROD_LDS) wtop = (size_t)PROD_LDS;
            lds = sizeof(double) * (wtop + BLOCK) + 16 * (size_t)(v.npat * v.pmax + 1);
            return {4, lds};
        } else if (v.fmt == 5) {
            size_t wtop = (size_t)(128 * v.wchunks + 2);
            if (!v.allwin && wtop < (size_t)PROD_LDS) wtop = (size_t)PROD_LDS;
            lds = sizeof(double) * (wtop + BLOCK) + 4 * (size_t)(v.npat * v.pmax + 4);
            if (v.nt) return {6, lds};
            else return {5, lds};
        } else if (v.fmt >= 6) {
            size_t wtop = (size_t)(128 * v.wchunks + 2);
            if (!v.allwin && wtop < (size_t)PROD_LDS) wtop = (size_t)PROD_LDS;
            lds = sizeof(double) * (wtop + BLOCK) + 4 * (size_t)((v.fmt == 7 ? v.npat * v.pmax : 0) + 4);
            if (v.fmt == 8) return {8, lds};
            else if (v.nt) return {9, lds};
            else return {7, lds};
        } else if (v.fmt == 3) {
            lds = (size_t)v.rt_cap * 12;
            if (v.rt_reg && !v.tiles) return {10, lds};
            else return {3, lds};
        } else if (v.fmt == 2) return {2, lds};
        else if (v.fmt == 1) return {1, lds};
        else return {0, lds};
    }
    return {NOTHING, 0};
}
// ... and which of its launches the `if constexpr` nest instantiates for an epilogue class
void compiled(const Flags &f, bool (&c)[17]) {
    for (bool &b : c) b = false;
    if (rejected(f)) return;
    if (!f.MO) c[0] = true;                                  // (the fallback)
    if (f.SM) c[14] = c[15] = c[16] = true;
    if (!f.NM) {
        c[11] = c[12] = true;
        if (f.SM) c[13] = true;
    }
    if (!f.MO)
        for (int k = 0; k <= 10; ++k) c[k] = true;
}
bool march_kernel_for(int fmt, int pen_gen, const Flags &f) {
    if (!fmt_march(fmt) || f.NM) return false;
    return f.SM || (fmt != 11 && pen_gen != 2);
}
// mk_grid_spmv_for: workgroups per CU of storage 4, 5 and of storage 6 .. 8 (P->covered != A->ntiles is !allwin)
long per_cu(int fmt, int wchunks, int allwin, int npat, int pmax) {
    if (fmt == 4 || fmt == 5) {
        long top = 128 * (long)wchunks + 2;
        if (!allwin && top < PROD_LDS) top = PROD_LDS;
        const long lds = 8 * (top + BLOCK) + (fmt == 4 ? 16 : 4) * (long)(npat * pmax + 4) + 2560;
        long per_cu = (160 * 1024) / lds;
        per_cu = per_cu > 7 ? 7 : (per_cu < 1 ? 1 : per_cu);
        return per_cu;
    }
    long top = 128 * (long)wchunks + 2;
    if (!allwin && top < PROD_LDS) top = PROD_LDS;
    const long lds = 8 * (top + BLOCK) + 4 * (long)((fmt == 7 ? npat * pmax : 0) + 4) + 2560;
    long per_cu = (160 * 1024) / lds;
    const long top_cu = (fmt == 8) ? 7 : 4;
    per_cu = per_cu > top_cu ? top_cu : (per_cu < 1 ? 1 : per_cu);
    return per_cu;
}
}  // namespace old

static long bad = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            if (++bad <= 40) {               \
                printf("MISMATCH " __VA_ARGS__); \
                printf("\n");                \
            }                                \
        }                                    \
    } while (0)

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--table")) {
        for (int k = 0; k < MK_FMT_COUNT; ++k) {
            const MkVariantRow &r = mk_variant_table[k];
            printf("%d %d %d %d %d %d\n", k, r.storage, r.min_blocks, r.xw_alias ? 1 : 0, r.carry ? 1 : 0, r.gen ? 1 : 0);
        }
        return 0;
    }
    long cases = 0;
    static_assert(MK_FMT_COUNT == 17 && MK_ST_COUNT == 12, "17 kernel variants, storage formats 0 .. 11");
    static_assert(MK_BLOCK == old::BLOCK && MK_SPMV_TILE == old::SPMV_TILE && MK_PROD_LDS == old::PROD_LDS && MK_PEN_OCC == old::PEN_OCC &&
                  MK_PEN_LDS == old::PEN_LDS && MK_PEN_LDS_SYM == old::PEN_LDS_SYM, "the sizes the header took over");
    for (int k = 0; k < 17; ++k) {
        const MkVariantRow &r = mk_variant_table[k];
        CHECK(r.min_blocks == old::min_blocks(k), "min_blocks of variant %d: %d, was %d", k, r.min_blocks, old::min_blocks(k));
        CHECK(r.xw_alias == old::xw_alias(k), "xw of variant %d", k);
        CHECK(r.carry == old::carry(k), "carry of variant %d", k);
        CHECK(mk_variant_march(k) == (k >= 11 && k <= 16), "march-ness of variant %d", k);
        ++cases;
    }
    for (int fmt = 0; fmt <= 11; ++fmt) CHECK(mk_fmt_march(fmt) == old::fmt_march(fmt), "mk_fmt_march(%d)", fmt);
    const int wchunks_of[] = {1, 2, 7, 8, 16, 17, 32, 64}, rt_cap_of[] = {256, 4096, 13312};
    const int pat_of[][2] = {{0, 0}, {1, 1}, {1, 7}, {8, 8}, {255, 27}};      // npat * pmax = 0, 1, 7, 64, 255 * 27
    for (int fl = 0; fl < 16; ++fl) {
        const old::Flags f{(fl & 1) != 0, (fl & 2) != 0, (fl & 4) != 0, (fl & 8) != 0};
        bool want_c[17];
        old::compiled(f, want_c);
        for (int k = 0; k < 17; ++k) {
            CHECK(mk_variant_compiled(k, f.NM, f.SM, f.MO, f.PROG) == want_c[k], "compiled: variant %d NM %d SM %d MO %d PROG %d (was %d)", k,
                  f.NM, f.SM, f.MO, f.PROG, want_c[k]);
            ++cases;
        }
        if (old::rejected(f)) continue;                      // no launcher exists for such an epilogue: nothing else to compare
        for (int fmt = 0; fmt <= 11; ++fmt)
        for (int bits = 0; bits < 16; ++bits)
        for (int pen_gen = 0; pen_gen <= 2; ++pen_gen) {
            const int nt = bits & 1, rt_reg = (bits >> 1) & 1, tiles = (bits >> 2) & 1, allwin = (bits >> 3) & 1;
            const int k = mk_spmv_variant(fmt, nt, rt_reg, tiles != 0, pen_gen, f.NM, f.SM, f.MO);
            CHECK(mk_variant_march(mk_spmv_variant(fmt, 0, 0, false, pen_gen, f.NM, f.SM, f.MO)) == old::march_kernel_for(fmt, pen_gen, f),
                  "march_kernel_for: fmt %d pen_gen %d flags %d", fmt, pen_gen, fl);
            for (int wchunks : wchunks_of)
            for (const auto &pat : pat_of)
            for (int rt_cap : rt_cap_of) {
                const old::View v{fmt, nt, rt_reg, tiles, pen_gen, wchunks, allwin, pat[0], pat[1], rt_cap};
                const old::Launch want = old::launch(v, f);
                ++cases;
                CHECK(want.variant != old::NOTHING, "the old chain launches nothing: fmt %d flags %d", fmt, fl);
                CHECK(k == want.variant, "variant: fmt %d nt %d rt_reg %d tiles %d pen_gen %d flags %d: %d, was %d", fmt, nt, rt_reg, tiles,
                      pen_gen, fl, k, want.variant);
                if (k < 0 || k != want.variant) continue;
                CHECK(mk_variant_compiled(k, f.NM, f.SM, f.MO, f.PROG), "variant %d is chosen for flags %d, which have no such kernel", k, fl);
                const size_t lds = mk_spmv_lds_bytes(k, fmt, wchunks, allwin, pat[0], pat[1], rt_cap);
                CHECK(lds == want.lds, "bytes: variant %d fmt %d wchunks %d allwin %d npat %d pmax %d rt_cap %d: %zu, was %zu", k, fmt, wchunks,
                      allwin, pat[0], pat[1], rt_cap, lds, want.lds);
                const int st = mk_variant_table[k].storage;
                CHECK(st == fmt || (k == MK_FMT_CSR && old::fmt_march(fmt)) || (st == MK_ST_WIDE_SLOT && fmt == MK_ST_WIDE_PAT),
                      "storage of variant %d: %d, launched on %d", k, st, fmt);
                if (fmt >= 4 && fmt <= 8) {
                    const long pc = mk_spmv_per_cu(fmt, wchunks, allwin, pat[0], pat[1]), was = old::per_cu(fmt, wchunks, allwin, pat[0], pat[1]);
                    CHECK(pc == was, "per_cu: fmt %d wchunks %d allwin %d npat %d pmax %d: %ld, was %ld", fmt, wchunks, allwin, pat[0], pat[1], pc, was);
                }
            }
        }
    }
    printf("cases %ld mismatches %ld\n", cases, bad);
    return bad ? 1 : 0;
}
