// mk_ringdepth.h -- how deep CG's ring of directions is (the m of the deferred x update, mk_cg.hip), as pure functions of byte
// counts (plain C++, no HIP: a host program can include it, tests/ringdepth_main.cpp does).
//
// Fused CG keeps the last m + 1 directions in a ring and sweeps x once per m passes: x costs 8 n + 16 n / m bytes per pass, so
// a deeper ring is less traffic, and each step of m is one more vector of device memory.  The first two buffers -- the pair a
// fused pass alternates between -- are the solver's own; every buffer beyond them counts as EXTRA, and all extras together may
// take an eighth of the device memory that was free before the first of them.
#pragma once
#include <stddef.h>

constexpr int MK_XD_MAX = 32;                                // cap of MK_CG_XDEFER: the ring holds at most MK_XD_MAX + 1 directions
constexpr size_t MK_XD_MIN_BYTES = (size_t)256 << 20;        // a vector up to here stays in the Infinity Cache: nothing to defer for

// The deepest m the memory rule serves: `held` buffers are in the ring already (they are not free any more: the extras among
// them are added back), each of vec_bytes.  At least 1: the pair is not subject to the rule.
inline int mk_ring_fit(size_t vec_bytes, size_t free_bytes, int held) {
    if (vec_bytes == 0) return MK_XD_MAX;
    const size_t held_extra = held > 2 ? (size_t)(held - 2) : 0;
    // extras = floor((free + held_extra vec) / (8 vec)) = floor((floor(free / vec) + held_extra) / 8): no product that could overflow
    const size_t q = free_bytes / vec_bytes;
    if (q >= (size_t)8 * MK_XD_MAX) return MK_XD_MAX;
    const size_t extras = (q + held_extra) / 8;
    return extras >= (size_t)(MK_XD_MAX - 1) ? MK_XD_MAX : 1 + (int)extras;
}

// The m of a set-up when MK_CG_XDEFER does not say: 1 where a vector is at most 256 MiB, beyond that the deepest m <= cap the
// memory rule serves.  cap: 0 = MK_XD_MAX.
inline int mk_ring_depth(size_t vec_bytes, size_t free_bytes, int held, int cap) {
    const int top = (cap < 1 || cap > MK_XD_MAX) ? MK_XD_MAX : cap;
    if (vec_bytes <= MK_XD_MIN_BYTES) return 1;
    const int fit = mk_ring_fit(vec_bytes, free_bytes, held);
    return fit < top ? fit : top;
}
