// haplotypes_host.h -- the part of spelling the haplotypes that is plain C++ (bgr_haplotype in include/bgreat_gpu.h has the definition): the oriented
// ids of a block entry (the kernels call them too), the checks of the two lists before any device work, and the walk and header line of the file.
// No spelling in here: that is the kernels' (haplotypes_kernels.h), and tests/haplotypes_ref.py is the definition.  No HIP: the host sanitizer
// program compiles it alone.
#ifndef BGREAT_AMD_HAPLOTYPES_HOST_H
#define BGREAT_AMD_HAPLOTYPES_HOST_H

#include <stdint.h>

#include <string>

#include "../../include/bgreat_gpu.h"
#include "blocks_host.h"

namespace bgr {

// the ids bgr_write_blocks prints: the bubble as the block's reading orients it; `which` = 0 for haplotype A's branch, 1 for B's
BGR_HD uint32_t hap_reversed(const bgr_block_entry& e) { return e.flags & BGR_BLOCK_REVERSED ? 1u : 0u; }
BGR_HD int32_t hap_src(const bgr_block_entry& e, const bgr_bubble& b) { return blocks_source(b, hap_reversed(e)); }
BGR_HD int32_t hap_snk(const bgr_block_entry& e, const bgr_bubble& b) { return blocks_sink(b, hap_reversed(e)); }
BGR_HD int32_t hap_branch(const bgr_block_entry& e, const bgr_bubble& b, uint32_t which) { return blocks_branch(b, hap_reversed(e), ((e.flags >> 1) & 1u) ^ (which & 1u)); }
BGR_HD uint32_t hap_ring(const bgr_block_entry& e) { return e.flags & (BGR_BLOCK_CIRCULAR | BGR_BLOCK_CONFLICT); }

// -> 0, or what is wrong with the input before any device work; *bad = the record:
//   1  a bubble names an id that is 0, beyond 2^30 or beyond n_unitigs     2  an entry that blocks_entries_ok refuses     3  the entries do not come
//   block after block in chain order (an index that does not follow, a block that ends early or late, a size, number or ring flag that changes
//   inside a block, block numbers that do not ascend)     4  an entry's source is not the sink of the entry before it in its block (no decided link
//   joins the two)     5  more entries than 2^30 - 1
inline int haplotypes_check(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* e, uint64_t n, uint64_t n_unitigs, uint64_t* bad) {
    *bad = n;
    if (n >= 0x40000000ull) return 5;
    for (uint64_t i = 0; i < n_bubbles; ++i) {
        *bad = i;
        const bgr_bubble& b = bubbles[i];
        if (!blocks_id_ok(b.source, n_unitigs) || !blocks_id_ok(b.sink, n_unitigs) || !blocks_id_ok(b.branch[0], n_unitigs) || !blocks_id_ok(b.branch[1], n_unitigs)) return 1;
    }
    if (!blocks_entries_ok(e, n, n_bubbles, bad)) return 2;
    for (uint64_t i = 0; i < n; ++i) {
        *bad = i;
        if (e[i].index == 0) {
            if (i && (e[i - 1].index + 1 != e[i - 1].size || e[i].block <= e[i - 1].block)) return 3;
        } else {
            if (i == 0 || e[i].index != e[i - 1].index + 1 || e[i].block != e[i - 1].block || e[i].size != e[i - 1].size || hap_ring(e[i]) != hap_ring(e[i - 1])) return 3;
            if (hap_src(e[i], bubbles[e[i].bubble]) != hap_snk(e[i - 1], bubbles[e[i - 1].bubble])) return 4;
        }
        if (i + 1 == n && e[i].index + 1 != e[i].size) return 3;
    }
    return 0;
}

// ---- the lines of the file ----------------------------------------------------------------------------------------------------------------
inline void hap_walk_id(int32_t id, std::string* buf) { *buf += id < 0 ? '<' : '>'; *buf += std::to_string(bubbles_abs(id)); }
// the walk of haplotype `which` of the block whose `size` entries begin at e, in GAF notation: src_0, then branch and sink of every entry
inline void hap_walk(const bgr_block_entry* e, uint64_t size, const bgr_bubble* bubbles, uint32_t which, std::string* buf) {
    hap_walk_id(hap_src(e[0], bubbles[e[0].bubble]), buf);
    for (uint64_t i = 0; i < size; ++i) {
        hap_walk_id(hap_branch(e[i], bubbles[e[i].bubble], which), buf);
        hap_walk_id(hap_snk(e[i], bubbles[e[i].bubble]), buf);
    }
}
// the header line of record h, whose block's entries begin at e
inline void hap_header(const bgr_haplotype& h, const bgr_block_entry* e, const bgr_bubble* bubbles, std::string* buf) {
    *buf += ">block"; *buf += std::to_string(h.block); *buf += h.hap ? "_B" : "_A";
    *buf += " bubbles="; *buf += std::to_string(h.size);
    *buf += " length="; *buf += std::to_string(h.length);
    *buf += " ring="; *buf += h.flags & BGR_BLOCK_CONFLICT ? "conflict" : (h.flags & BGR_BLOCK_CIRCULAR ? "circular" : ".");
    *buf += " walk="; hap_walk(e, h.size, bubbles, h.hap, buf);
    *buf += '\n';
}

// -> whether the records are the ones the kept blocks of `e` give (block, hap, size, ring flags, A before B, in block order) and lie back to back in
// seq_bytes bytes; first[i] = the entry that heads record i's block; *bad = the first record that is not
inline bool hap_records_ok(const bgr_haplotype* h, uint64_t n, const bgr_block_entry* e, uint64_t n_entries, uint64_t seq_bytes, uint64_t* first, uint64_t* bad) {
    uint64_t at = 0, off = 0;
    for (uint64_t i = 0; i < n; ++i) {
        *bad = i;
        if (h[i].hap != (i & 1u)) return false;
        if (!(i & 1u)) {
            while (at < n_entries && !(e[at].index == 0 && e[at].block == h[i].block)) ++at;
            if (at >= n_entries) return false;
        } else if (h[i].block != h[i - 1].block) return false;
        if (e[at].size != h[i].size || hap_ring(e[at]) != h[i].flags || h[i].offset != off || h[i].length > seq_bytes - off) return false;
        first[i] = at;
        off += h[i].length;
    }
    *bad = n;
    return off == seq_bytes;
}

}  // namespace bgr

#endif
