// recompact_host.h -- the part of the re-compaction that is plain C++ (bgr_chain in include/bgreat_gpu.h has the definition): the keep bytes of a
// run, the check of a result before it is written, and the header line of the file.  No compaction in here: that is the kernels'
// (recompact_kernels.h), and tests/recompact_ref.py is the definition.  No HIP: the host sanitizer program compiles it alone.
#ifndef BGREAT_AMD_RECOMPACT_HOST_H
#define BGREAT_AMD_RECOMPACT_HOST_H

#include <stdint.h>

#include <string>

#include "../../include/bgreat_gpu.h"

namespace bgr {

// the run-level rule: keep[u] = (reads[u] >= min_reads); min_reads 0 keeps everything
inline void recompact_keep(const bgr_unitig_abundance* rows, uint64_t n, uint64_t min_reads, uint8_t* keep) {
    for (uint64_t i = 0; i < n; ++i) keep[i] = rows[i].reads >= min_reads ? 1 : 0;
}

// the CLI's --min-reads: digits only, one to nine of them (0 is allowed) -> whether it is one
inline bool recompact_parse_min_reads(const char* text, uint64_t* out) {
    if (!text || !*text) return false;
    uint64_t v = 0;
    int digits = 0;
    for (const char* p = text; *p; ++p) {
        if (*p < '0' || *p > '9' || ++digits > 9) return false;
        v = v * 10 + (uint64_t)(*p - '0');
    }
    *out = v;
    return true;
}

// -> whether the records lie back to back in walk_n ints and seq_bytes bytes, every chain has a unitig and at least k characters, only the circular
// flag is set, and every walk id is one of the graph's; *bad = the first record that is not so (n: the totals do not add up)
inline bool recompact_records_ok(const bgr_chain* c, uint64_t n, const int32_t* walk, uint64_t walk_n, uint64_t seq_bytes, uint64_t n_unitigs, uint32_t k, uint64_t* bad) {
    uint64_t w = 0, s = 0;
    for (uint64_t i = 0; i < n; ++i) {
        *bad = i;
        if (c[i].walk_off != w || c[i].seq_off != s || c[i].n_unitigs == 0 || c[i].n_unitigs > walk_n - w || c[i].seq_len < k || c[i].seq_len > seq_bytes - s) return false;
        if (c[i].flags & ~BGR_CHAIN_CIRCULAR) return false;
        for (uint64_t j = 0; j < c[i].n_unitigs; ++j) {
            const int64_t id = walk[w + j];
            const uint64_t a = (uint64_t)(id < 0 ? -id : id);
            if (a == 0 || a > n_unitigs) return false;
        }
        w += c[i].n_unitigs;
        s += c[i].seq_len;
    }
    *bad = n;
    return w == walk_n && s == seq_bytes;
}

// the header line of chain `ordinal` (from 1), whose walk begins at w
inline void recompact_header(uint64_t ordinal, const bgr_chain& c, const int32_t* w, std::string* buf) {
    *buf += '>'; *buf += std::to_string(ordinal);
    *buf += " LN:i:"; *buf += std::to_string(c.seq_len);
    *buf += " unitigs="; *buf += std::to_string(c.n_unitigs);
    *buf += " ring="; *buf += c.flags & BGR_CHAIN_CIRCULAR ? "circular" : ".";
    *buf += " walk=";
    for (uint32_t j = 0; j < c.n_unitigs; ++j) {
        const int64_t id = w[j];
        *buf += id < 0 ? '<' : '>';
        *buf += std::to_string(id < 0 ? -id : id);
    }
    *buf += '\n';
}

}  // namespace bgr

#endif
