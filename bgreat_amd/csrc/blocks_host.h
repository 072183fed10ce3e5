// blocks_host.h -- the part of haplotype blocks that is plain C++ (bgr_block_entry in include/bgreat_gpu.h has the definition): how a bubble record
// reads as a node, when a phase record is a decided link (the kernels call both), the checks of the two lists before any device work, and the
// header and line of the file.  No chaining in here: that is the kernels' (blocks_kernels.h), and tests/blocks_ref.py is the definition.  No HIP:
// the host sanitizer program compiles it alone.
#ifndef BGREAT_AMD_BLOCKS_HOST_H
#define BGREAT_AMD_BLOCKS_HOST_H

#include <stdint.h>

#include <string>

#include "../../include/bgreat_gpu.h"
#include "phase_host.h"

namespace bgr {

// node x = 2 i + r is bubble record i read as given (r = 0) or as its mate (r = 1): (s, t, b0, b1) -> (-t, -s, -b0, -b1).  Negating both branches
// keeps their (|id|, id < 0) order, as |b0| < |b1| (blocks_check), so a branch keeps its index under mating
BGR_HD int32_t blocks_source(const bgr_bubble& b, uint32_t r) { return r ? -b.sink : b.source; }
BGR_HD int32_t blocks_sink(const bgr_bubble& b, uint32_t r) { return r ? -b.source : b.sink; }
BGR_HD int32_t blocks_branch(const bgr_bubble& b, uint32_t r, uint32_t i) { return r ? -b.branch[i] : b.branch[i]; }

// -> whether |(n11 + n22) - (n12 + n21)| >= min_phase; *parity = 0 when cis is the larger, 1 when trans.  The sums as 65-bit numbers {carry, low
// word}: four full 64-bit counts do not wrap (phase_call's 128-bit sums, in words the device has too)
BGR_HD bool blocks_decided(const uint64_t count[4], uint64_t min_phase, uint32_t* parity) {
    const uint64_t cl = count[0] + count[3], tl = count[1] + count[2];
    const uint64_t ch = cl < count[0] ? 1u : 0u, th = tl < count[1] ? 1u : 0u;
    const bool trans = th > ch || (th == ch && tl > cl);
    const uint64_t bh = trans ? th : ch, bl = trans ? tl : cl, sh = trans ? ch : th, sl = trans ? cl : tl;   // big - small, which is >= 0
    const uint64_t dl = bl - sl, dh = bh - sh - (bl < sl ? 1u : 0u);
    *parity = trans ? 1u : 0u;
    return dh != 0 || dl >= min_phase;
}

inline bool blocks_id_ok(int32_t x, uint64_t n_unitigs) { return phase_id_ok(x) && (uint64_t)bubbles_abs(x) <= n_unitigs; }

// -> 0, or what is wrong with the input before any device work; *bad = the record:
//   1  a bubble names an id that is 0, beyond 2^30 or beyond n_unitigs      2  a bubble whose four ids are not four unitigs, or whose branches are not in
//   (|id|, id < 0) order                3  a bubble that is not the canonical reading of (s, t) and (-t, -s)     4  the bubbles are not strictly
//   ascending by (|source|, source < 0)                5  a phase record names such an id, or its via is not positive      6  the phase records are
//   not strictly ascending by via       7  more bubbles than 2^30 - 1 (a node index and a flag share a word)
inline int blocks_check(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_phase* phase, uint64_t n_phase, uint64_t n_unitigs, uint64_t* bad) {
    *bad = n_bubbles;
    if (n_bubbles >= 0x40000000ull) return 7;
    for (uint64_t i = 0; i < n_bubbles; ++i) {
        const bgr_bubble& b = bubbles[i];
        *bad = i;
        if (!blocks_id_ok(b.source, n_unitigs) || !blocks_id_ok(b.sink, n_unitigs) || !blocks_id_ok(b.branch[0], n_unitigs) || !blocks_id_ok(b.branch[1], n_unitigs)) return 1;
        const uint32_t s = bubbles_abs(b.source), t = bubbles_abs(b.sink), x = bubbles_abs(b.branch[0]), y = bubbles_abs(b.branch[1]);
        if (s == t || s == x || s == y || t == x || t == y || x >= y) return 2;
        if (t < s) return 3;   // ((|s|, s < 0, |t|, t < 0) against (|t|, t > 0, |s|, s > 0): |s| != |t| decides, as in bubble_at)
        if (i && !bubbles_id_less(bubbles[i - 1].source, b.source)) return 4;
    }
    for (uint64_t i = 0; i < n_phase; ++i) {
        const bgr_phase& p = phase[i];
        *bad = i;
        const int32_t ids[7] = {p.via, p.source, p.in[0], p.in[1], p.out[0], p.out[1], p.sink};
        for (int32_t x : ids) if (!blocks_id_ok(x, n_unitigs)) return 5;
        if (p.via < 0) return 5;
        if (i && phase[i - 1].via >= p.via) return 6;
    }
    return 0;
}

// -> whether the entries are ones the writer can print over `n_bubbles` records: *bad = the first that is not
inline bool blocks_entries_ok(const bgr_block_entry* e, uint64_t n, uint64_t n_bubbles, uint64_t* bad) {
    for (uint64_t i = 0; i < n; ++i) {
        *bad = i;
        if (e[i].bubble >= n_bubbles || e[i].flags > 15u || e[i].block == 0 || e[i].index >= e[i].size) return false;
    }
    return true;
}

// ---- the lines of the file ----------------------------------------------------------------------------------------------------------------
inline const char* blocks_header() { return "#block\tindex\tsize\tbubble\tsource\tsink\thapA\thapB\tstrand\tring\n"; }
// `b` is the record the entry names: the ids as the block's reading orients them, haplotype A's branch first
inline void blocks_line(const bgr_block_entry& e, const bgr_bubble& b, std::string* buf) {
    const uint32_t r = e.flags & BGR_BLOCK_REVERSED ? 1u : 0u, hap = e.flags & BGR_BLOCK_HAP ? 1u : 0u;
    *buf += std::to_string(e.block); *buf += '\t'; *buf += std::to_string(e.index); *buf += '\t'; *buf += std::to_string(e.size); *buf += '\t';
    *buf += std::to_string((uint64_t)e.bubble + 1); *buf += '\t';
    *buf += std::to_string(blocks_source(b, r)); *buf += '\t'; *buf += std::to_string(blocks_sink(b, r)); *buf += '\t';
    *buf += std::to_string(blocks_branch(b, r, hap)); *buf += '\t'; *buf += std::to_string(blocks_branch(b, r, 1u - hap)); *buf += '\t';
    *buf += r ? '-' : '+'; *buf += '\t';
    *buf += e.flags & BGR_BLOCK_CONFLICT ? "conflict" : (e.flags & BGR_BLOCK_CIRCULAR ? "circular" : "."); *buf += '\n';
}

}  // namespace bgr

#endif
