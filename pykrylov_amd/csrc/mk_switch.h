// mk_switch.h -- every environment variable libmikrylov reads and the one parser they share (plain C++, no HIP: a host
// program can include it, tests/switch_main.cpp does).  The same table, with the Python-side variables, is in README.md.
#pragma once
#include <errno.h>
#include <limits.h>
#include <stdlib.h>

enum MkSwitch {
    MK_SW_CG_FUSE, MK_SW_CG_XDEFER, MK_SW_ILU_FUSE_ROWS, MK_SW_SPMV_FORMAT, MK_SW_SPMV_NT, MK_SW_PENCIL_MIN_ROWS, MK_SW_PEN_GEN,
    MK_SW_RT_PHASES, MK_SW_COLBLOCK_KB, MK_SW_GRID_STREAM, MK_SW_GRID_SPMV, MK_SW_COPY_THREADS, MK_SW_DEBUG_PLAN, MK_SW_COUNT
};
// kind 'i': an integer clamped to [lo, hi] ('f': a flag, set by its mere presence).  dflt: what an unset or unparsable variable
// gives; "auto" in the text: the site chooses while the variable is not set.  once: read at the first query in a process and
// kept (true), or read again at every query (false: tests switch these between solves).
struct MkSwitchRow {
    const char *name;
    char kind;
    long dflt, lo, hi;
    bool once;
    const char *what;
};
constexpr MkSwitchRow mk_switch_table[MK_SW_COUNT] = {
    {"MK_CG_FUSE", 'i', 1, INT_MIN, INT_MAX, false, "0: CG keeps its three-kernel pass on brick-march matrices"},
    {"MK_CG_XDEFER", 'i', 0, 1, 32, false, "fused CG sweeps x once per m passes (auto: 1 up to 256 MiB per vector, beyond it the deepest m <= 32 whose ring fits an eighth of the free memory)"},
    {"MK_ILU_FUSE_ROWS", 'i', 256, 0, INT_MAX, false, "ILU / IC levels of at most this many rows share a launch (0: one launch per level)"},
    {"MK_SPMV_FORMAT", 'i', 11, 0, 11, true, "highest storage format the builder may choose"},
    {"MK_SPMV_NT", 'i', 0, INT_MIN, INT_MAX, true, "non-temporal value loads and product stores (auto: on where a vector exceeds 256 MiB)"},
    {"MK_PENCIL_MIN_ROWS", 'i', 1L << 21, 0, LONG_MAX, true, "smallest matrix the brick march is chosen for automatically"},
    {"MK_PEN_GEN", 'i', 0, INT_MIN, INT_MAX, true, "1: the general-geometry march kernels on aligned geometries too"},
    {"MK_RT_PHASES", 'i', 0, 0, 64, true, "column phases of the resident-tile format (0 = auto: by the length of x)"},
    {"MK_COLBLOCK_KB", 'i', 0, 0, LONG_MAX / 1024, true, "column-block size in KiB of x, 0 = never (auto: long rows over a long x)"},
    {"MK_GRID_STREAM", 'i', 512, 1, 2048, true, "workgroup cap of the streaming kernels"},
    {"MK_GRID_SPMV", 'i', 1024, 1, 2048, true, "workgroup cap of the product kernels; set: it replaces the per-format grids"},
    {"MK_COPY_THREADS", 'i', 4, 0, 8, false, "host threads staging large pageable transfers (fewer than 2: plain copies)"},
    {"MK_DEBUG_PLAN", 'f', 0, 0, 1, false, "print what the format builder decided and why"},
};

struct MkSwitchVal {
    bool set;                                                // the variable is there and (kind 'i') starts with a number a long holds
    long v;
};
inline MkSwitchVal mk_switch_parse(const MkSwitchRow &r, const char *text) {
    if (!text) return {false, r.dflt};
    if (r.kind == 'f') return {true, 1};
    char *end = nullptr;
    errno = 0;
    const long v = strtol(text, &end, 10);                   // (one call: whatever follows the number is ignored, as atoi did)
    if (end == text || errno == ERANGE) return {false, r.dflt};
    return {true, v < r.lo ? r.lo : (v > r.hi ? r.hi : v)};
}
template <MkSwitch S>
inline MkSwitchVal mk_switch() {
    constexpr MkSwitchRow r = mk_switch_table[S];
    if constexpr (r.once) {
        static const MkSwitchVal v = mk_switch_parse(r, getenv(r.name));
        return v;
    } else {
        return mk_switch_parse(r, getenv(r.name));
    }
}
template <MkSwitch S>
inline long mk_switch_int() { return mk_switch<S>().v; }
template <MkSwitch S>
inline bool mk_switch_flag() { return mk_switch<S>().set; }
