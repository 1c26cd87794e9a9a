// mk_variant.h -- the storage formats of a matrix, the instantiation families ("variants") of mk_spmv_kernel, and the one table
// that says how a product gets from the first to the second: which variant, how many workgroups per CU, how much dynamic LDS
// and how it is laid out (plain C++, no HIP: a host program can include it, tests/variant_main.cpp does).  DESIGN.md 3.1 has
// the same table in words.
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define MK_HD __host__ __device__
#else
#define MK_HD
#endif

// Storage format of a plan (MkPlan::fmt, MkCsrView::fmt, mk_csr_set_format, MK_SPMV_FORMAT): public integers.
enum MkStorage {
    MK_ST_CSR = 0,             // plain CSR: x through gathers
    MK_ST_WIN = 1,             // windows of x in LDS + one uint16 LDS slot per nonzero
    MK_ST_DICT = 2,            // windows + one packed word per nonzero {slot, index into a dictionary of <= 256 values}
    MK_ST_RESIDENT = 3,        // plain CSR with the tile resident in LDS and the gathers ordered by column block
    MK_ST_PAT = 4,             // windows + dictionary + one pattern byte per row instead of a word per nonzero
    MK_ST_PAT_STREAM = 5,      // windows + pattern byte per row + the raw values streamed in tile-sliced ELL order
    MK_ST_WIDE_SLOT = 6,       // wide tiles (rows <= 32 entries, <= 32 chunks): slots + values streamed
    MK_ST_WIDE_PAT = 7,        // wide tiles: pattern byte per row + values streamed
    MK_ST_WIDE_DICT = 8,       // wide tiles: pattern byte per row + dictionary
    MK_ST_MARCH = 9,           // z-marching bricks of a 7-point-class matrix: pattern byte per row + dictionary (mk_spmv_fmt9.h)
    MK_ST_MARCH_STREAM = 10,   // the same march with seven streamed value arrays (no dictionary)
    MK_ST_MARCH_SYM = 11,      // ... of a matrix symmetric bit for bit: the diagonal and the upper values only
    MK_ST_COUNT
};
constexpr bool mk_fmt_march(int fmt) { return fmt == MK_ST_MARCH || fmt == MK_ST_MARCH_STREAM || fmt == MK_ST_MARCH_SYM; }
constexpr bool mk_fmt_wide(int fmt) { return fmt == MK_ST_WIDE_SLOT || fmt == MK_ST_WIDE_PAT || fmt == MK_ST_WIDE_DICT; }
// a row is one pattern byte: no per-nonzero words, no row pointers for the windowed tiles
constexpr bool mk_fmt_pattern(int fmt) { return fmt == MK_ST_PAT || fmt == MK_ST_PAT_STREAM || mk_fmt_wide(fmt); }
// tiles with windows of x in LDS (tiles the cover could not serve take the gather path)
constexpr bool mk_fmt_windowed(int fmt) { return fmt == MK_ST_WIN || fmt == MK_ST_DICT || mk_fmt_pattern(fmt); }
// the plain CSR arrays are all the kernel reads
constexpr bool mk_fmt_plain(int fmt) { return fmt == MK_ST_CSR || fmt == MK_ST_RESIDENT; }

// Kernel variant: the FMT template value of mk_spmv_kernel (an int, so that the kernels' symbol names do not depend on this enum).
enum MkVariant {
    MK_FMT_CSR = 0, MK_FMT_WIN = 1, MK_FMT_DICT = 2, MK_FMT_RESIDENT = 3, MK_FMT_PAT = 4, MK_FMT_PAT_STREAM = 5,
    MK_FMT_PAT_STREAM_NT = 6,          // storage 5 with non-temporal loads of the value stream
    MK_FMT_WIDE = 7,                   // storage 6 and 7: streamed values
    MK_FMT_WIDE_DICT = 8,              // storage 8: values from the dictionary
    MK_FMT_WIDE_NT = 9,                // MK_FMT_WIDE with non-temporal loads of the streams
    MK_FMT_PAIR = 10,                  // storage 3 with a second tile per workgroup in registers (rows <= 5 entries)
    MK_FMT_PENCIL = 11, MK_FMT_PENCIL_STREAM = 12, MK_FMT_PENCIL_SYM = 13,         // storage 9 / 10 / 11 on whole aligned bricks
    MK_FMT_PENCIL_G = 14, MK_FMT_PENCIL_STREAM_G = 15, MK_FMT_PENCIL_SYM_G = 16,   // ... on a general geometry (mk_spmv_fmt9.h, GEN)
    MK_FMT_COUNT,
    MK_FMT_NONE = -1                   // a march-only epilogue met a storage format without a march: the launch is an error
};

// LDS geometry shared with the kernels (doubles unless it says bytes)
constexpr int MK_BLOCK = 256;                        // 4 wave64 per workgroup
constexpr int MK_SPMV_TILE = 2048;                   // products the gather path stages in LDS per pass (16 KiB)
constexpr int MK_PROD_LD = MK_BLOCK + 1;             // (product staging buffer of the SpMV kernels, mk_device.h)
constexpr int MK_PROD_LDS = 8 * MK_PROD_LD;          // doubles reserved for products (>= MK_SPMV_TILE of the gather path)
constexpr int MK_PEN_OCC = 2;                        // march: workgroups per CU the register budget is cut for (profiles/r05_pencil_variants.txt)
constexpr int MK_PEN_RS = 132;                       // march, LDS row: [0] pad, [1] west edge, [2..129] rows, [130] east edge, [131] pad
constexpr int MK_PEN_LDS = 3 * 6 * MK_PEN_RS + MK_BLOCK;     // two plane images of 6 rows + the dump rows (lanes without an edge row
                                                             // store there, at the same buffer offset as the others)
constexpr int MK_PEN_VB = 6 * 128 + 4 * MK_PEN_RS;   // per buffer of the symmetric march's value image: 5 lines of +L values (halo
                                                     // line, four brick lines) + a dump line, 4 lines of +1 values
constexpr int MK_PEN_LDS_SYM = MK_PEN_LDS + 2 * MK_PEN_VB;

struct MkVariantRow {
    int storage;        // the storage format it serves (MK_FMT_WIDE / _NT: MK_ST_WIDE_PAT too)
    int min_blocks;     // workgroups per CU the kernel is compiled for (__launch_bounds__) and the grid may count on
    bool xw_alias;      // the x windows start at the base of the dynamic LDS, where the gather path of a tile without windows
                        // stages its products (never live together); false: behind the MK_PROD_LDS doubles of the staging area
    bool carry;         // a product of many steps runs as several launches: the fused dots' accumulators travel through A.carry
    bool gen;           // a march on a general geometry
};
constexpr MkVariantRow mk_variant_table[MK_FMT_COUNT] = {
    /* MK_FMT_CSR             */ {MK_ST_CSR, 8, false, false, false},
    /* MK_FMT_WIN             */ {MK_ST_WIN, 4, false, false, false},
    /* MK_FMT_DICT            */ {MK_ST_DICT, 4, true, false, false},
    /* MK_FMT_RESIDENT        */ {MK_ST_RESIDENT, 8, false, false, false},
    /* MK_FMT_PAT             */ {MK_ST_PAT, 7, true, false, false},
    /* MK_FMT_PAT_STREAM      */ {MK_ST_PAT_STREAM, 7, true, false, false},
    /* MK_FMT_PAT_STREAM_NT   */ {MK_ST_PAT_STREAM, 7, true, false, false},
    /* MK_FMT_WIDE            */ {MK_ST_WIDE_SLOT, 4, true, false, false},      // (128 registers)
    /* MK_FMT_WIDE_DICT       */ {MK_ST_WIDE_DICT, 7, true, false, false},      // (no values in registers)
    /* MK_FMT_WIDE_NT         */ {MK_ST_WIDE_SLOT, 4, true, false, false},
    /* MK_FMT_PAIR            */ {MK_ST_RESIDENT, 8, false, true, false},
    /* MK_FMT_PENCIL          */ {MK_ST_MARCH, MK_PEN_OCC, true, false, false},
    /* MK_FMT_PENCIL_STREAM   */ {MK_ST_MARCH_STREAM, MK_PEN_OCC, true, false, false},
    /* MK_FMT_PENCIL_SYM      */ {MK_ST_MARCH_SYM, MK_PEN_OCC, true, false, false},
    /* MK_FMT_PENCIL_G        */ {MK_ST_MARCH, MK_PEN_OCC, true, false, true},
    /* MK_FMT_PENCIL_STREAM_G */ {MK_ST_MARCH_STREAM, MK_PEN_OCC, true, false, true},
    /* MK_FMT_PENCIL_SYM_G    */ {MK_ST_MARCH_SYM, MK_PEN_OCC, true, false, true},
};
constexpr bool mk_variant_march(int k) { return k >= 0 && k < MK_FMT_COUNT && mk_fmt_march(mk_variant_table[k].storage); }

// The brick-march kernels (unrolled, software-pipelined) are by far the most expensive instantiations, so an epilogue says
// where it can never meet them (mk_device.h): NO_MARCH (the least-squares loops), SYM_MARCH (plain products and CG: the few that
// may meet the symmetric twin and a general geometry), MARCH_ONLY (CG's fuse hooks: the six marches and nothing else, no row
// program; the launcher asserts that it comes with SYM_MARCH and without NO_MARCH).  Is variant k compiled for such an epilogue?
constexpr bool mk_variant_compiled(int k, bool no_march, bool sym_march, bool march_only, bool prog) {
    if (march_only && (!sym_march || no_march || prog)) return false;
    if (!mk_variant_march(k)) return !march_only;
    if (mk_variant_table[k].gen) return sym_march;           // (NO_MARCH with SYM_MARCH: no epilogue says both)
    return !no_march && (sym_march || k != MK_FMT_PENCIL_SYM);
}

// Storage format and the launch's flags -> kernel variant.  nt: non-temporal loads of the streams; rt_reg: the plan pairs
// tiles; tile_list: the launch covers a list of tiles; pen_gen: 0 whole aligned bricks, 1 aligned with leftover planes, 2 general.
constexpr int mk_spmv_variant(int fmt, int nt, int rt_reg, bool tile_list, int pen_gen, bool no_march, bool sym_march,
                              bool march_only) {
    if (!mk_fmt_march(fmt)) {
        if (march_only) return MK_FMT_NONE;
        switch (fmt) {
        case MK_ST_WIN: return MK_FMT_WIN;
        case MK_ST_DICT: return MK_FMT_DICT;
        case MK_ST_RESIDENT: return (rt_reg && !tile_list) ? MK_FMT_PAIR : MK_FMT_RESIDENT;
        case MK_ST_PAT: return MK_FMT_PAT;
        case MK_ST_PAT_STREAM: return nt ? MK_FMT_PAT_STREAM_NT : MK_FMT_PAT_STREAM;
        case MK_ST_WIDE_SLOT:
        case MK_ST_WIDE_PAT: return nt ? MK_FMT_WIDE_NT : MK_FMT_WIDE;
        case MK_ST_WIDE_DICT: return MK_FMT_WIDE_DICT;
        default: return MK_FMT_CSR;
        }
    }
    // a march format on an epilogue without that march (only a format forced by hand brings it about): the CSR gather kernel
    // on the same arrays -- over all rows, same row sums bit for bit
    if (!march_only && (no_march || ((fmt == MK_ST_MARCH_SYM || pen_gen == 2) && !sym_march))) return MK_FMT_CSR;
    const bool gen = sym_march && pen_gen;                   // (its masked last round also takes an aligned launch's leftover planes)
    if (fmt == MK_ST_MARCH) return gen ? MK_FMT_PENCIL_G : MK_FMT_PENCIL;
    if (fmt == MK_ST_MARCH_STREAM) return gen ? MK_FMT_PENCIL_STREAM_G : MK_FMT_PENCIL_STREAM;
    return gen ? MK_FMT_PENCIL_SYM_G : MK_FMT_PENCIL_SYM;
}

// Doubles of the dynamic LDS in front of what must outlive a tile: the windows (wchunks chunks of 128 doubles + 2), or the
// gather path's product staging where a tile without windows may run (allwin: no tile ever does)
MK_HD constexpr int mk_spmv_wtop(int wchunks, int allwin) {
    const int wtop = 128 * wchunks + 2;
    return (!allwin && wtop < MK_PROD_LDS) ? MK_PROD_LDS : wtop;
}

// Variant and sizes -> bytes of dynamic LDS of the launch (fmt: MK_FMT_WIDE serves two storage formats).
constexpr size_t mk_spmv_lds_bytes(int k, int fmt, int wchunks, int allwin, int npat, int pmax, int rt_cap) {
    const size_t staging = sizeof(double) * (size_t)MK_PROD_LDS, windows = sizeof(double) * (size_t)(128 * wchunks + 2);
    const size_t top = sizeof(double) * (size_t)(mk_spmv_wtop(wchunks, allwin) + MK_BLOCK);   // windows or products, 256 zeros
    const size_t ntab = (size_t)(npat * pmax);
    switch (k) {
    case MK_FMT_WIN: return staging + windows;
    case MK_FMT_DICT: {                                      // windows + packed words, or the gather path's products
        const size_t w = windows + sizeof(unsigned) * (MK_SPMV_TILE + 16);
        return w > staging ? w : staging;
    }
    case MK_FMT_RESIDENT:
    case MK_FMT_PAIR: return (size_t)rt_cap * 12;            // the tile's values and columns
    case MK_FMT_PAT: return top + 16 * (ntab + 1);           // ... + table of {offset, value} entries
    case MK_FMT_PAT_STREAM:
    case MK_FMT_PAT_STREAM_NT: return top + 4 * (ntab + 4);  // ... + offset table
    case MK_FMT_WIDE:
    case MK_FMT_WIDE_NT: return top + 4 * ((fmt == MK_ST_WIDE_PAT ? ntab : 0) + 4);   // ... + pattern words
    case MK_FMT_WIDE_DICT: return top + 4 * 4;
    case MK_FMT_PENCIL:
    case MK_FMT_PENCIL_G: return sizeof(double) * (size_t)MK_PEN_LDS + 64 * (size_t)npat;   // plane images + pattern table
    case MK_FMT_PENCIL_STREAM:
    case MK_FMT_PENCIL_STREAM_G: return sizeof(double) * (size_t)MK_PEN_LDS;
    case MK_FMT_PENCIL_SYM:
    case MK_FMT_PENCIL_SYM_G: return sizeof(double) * (size_t)MK_PEN_LDS_SYM;               // ... + the image of the plane's values
    default: return staging;                                 // MK_FMT_CSR
    }
}

// Workgroups per CU of the windowed pattern and wide formats (storage 4 .. 8): as many as the variant is compiled for and
// the 160 KiB of LDS hold.
constexpr int MK_LDS_STATIC = 2560;                          // bytes allowed for a kernel's static LDS arrays
constexpr int MK_LDS_PAT_GRID = 48;                          // storage 4: the grid rule has always counted three table entries more
                                                             // than the launch asks for; kept so that no grid changes, it is no
                                                             // truth about the kernel
constexpr int mk_spmv_per_cu(int fmt, int wchunks, int allwin, int npat, int pmax) {
    const int k = mk_spmv_variant(fmt, 0, 0, false, 0, false, false, false);
    const long lds = (long)mk_spmv_lds_bytes(k, fmt, wchunks, allwin, npat, pmax, 0) + MK_LDS_STATIC + (fmt == MK_ST_PAT ? MK_LDS_PAT_GRID : 0);
    const long per_cu = (160 * 1024) / lds, top = mk_variant_table[k].min_blocks;
    return (int)(per_cu > top ? top : (per_cu < 1 ? 1 : per_cu));
}
