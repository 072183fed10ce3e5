// haplotag_host.h -- the part of haplotags that is plain C++ (bgr_read_tag in include/bgreat_gpu.h has the definition): the tag table built from a
// run's structs or from the lines of a --blocks file, with every check, the tag of one row as the host formatter computes it (the twin of the
// device function in haplotag_device.h) and the fields a GAF line gains.  tests/haplotag_ref.py is the definition.  No HIP and no object of the
// C-ABI: the host sanitizer program compiles it alone, and pipeline.cpp includes it without needing a symbol of the library.
#ifndef BGREAT_AMD_HAPLOTAG_HOST_H
#define BGREAT_AMD_HAPLOTAG_HOST_H

#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/bgreat_gpu.h"
#include "blocks_host.h"

namespace bgr {

// |id| in 64 bits: INT32_MIN is 2^31, merely beyond every graph
inline uint64_t haplotag_abs(int64_t x) { return (uint64_t)(x < 0 ? -x : x); }

// table[|id|] = tag, or what is wrong with it in *msg (false): an id that is 0 or beyond n_unitigs, a unitig that has another tag already
inline bool haplotag_put(uint32_t* table, uint64_t n_unitigs, int64_t id, uint32_t tag, std::string* msg) {
    const uint64_t u = haplotag_abs(id);
    if (u == 0 || u > n_unitigs) { *msg = "unitig " + std::to_string(id) + " is not one of 1 .. " + std::to_string(n_unitigs); return false; }
    if (table[u] && table[u] != tag) { *msg = "unitig " + std::to_string(u) + " would receive two different tags"; return false; }
    table[u] = tag;
    return true;
}
// one bubble of one block: haplotype A's branch and B's
inline bool haplotag_pair(uint32_t* table, uint64_t n_unitigs, int64_t block, int64_t a, int64_t b, std::string* msg) {
    if (block < 1 || block >= (1ll << 31)) { *msg = "block " + std::to_string(block) + " is not one of 1 .. 2^31 - 1"; return false; }
    if (haplotag_abs(a) == haplotag_abs(b)) { *msg = "one unitig (" + std::to_string(a) + ") on both haplotypes"; return false; }
    return haplotag_put(table, n_unitigs, a, (uint32_t)block << 1, msg) && haplotag_put(table, n_unitigs, b, ((uint32_t)block << 1) | 1u, msg);
}
inline uint64_t haplotag_count(const uint32_t* table, uint64_t n_unitigs) {
    uint64_t n = 0;
    for (uint64_t u = 1; u <= n_unitigs; ++u) n += table[u] != 0;
    return n;
}

// The table (n_unitigs + 1 words, zeroed here) from the entries of the blocks with size >= min_block; false with *msg: an entry that names no
// bubble, or what haplotag_pair refuses
inline bool haplotag_table_of(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries, uint64_t n_entries, uint64_t n_unitigs, uint64_t min_block,
                              uint32_t* table, std::string* msg) {
    memset(table, 0, (n_unitigs + 1) * sizeof(uint32_t));
    for (uint64_t i = 0; i < n_entries; ++i) {
        const bgr_block_entry& e = entries[i];
        if (e.size < min_block) continue;
        std::string m;
        bool ok = e.bubble < n_bubbles;
        if (!ok) m = "it names no bubble of the list";
        else {
            const uint32_t h = (e.flags & BGR_BLOCK_HAP) ? 1u : 0u;
            ok = haplotag_pair(table, n_unitigs, e.block, bubbles[e.bubble].branch[h], bubbles[e.bubble].branch[1 - h], &m);
        }
        if (!ok) { *msg = "entry " + std::to_string(i) + ": " + m; return false; }
    }
    return true;
}

// a field that is a decimal integer -- an optional '-', then digits only -> its value; one beyond 2^58 reads as +-2^62 (an overlong number is beyond every graph)
inline bool haplotag_dec(const char* p, const char* e, int64_t* v) {
    const bool neg = p < e && *p == '-';
    if (neg) ++p;
    if (p == e) return false;
    uint64_t u = 0;
    for (; p < e; ++p) {
        if (*p < '0' || *p > '9') return false;
        if (u > (1ull << 58)) u = 1ull << 62;   // (and stays there: beyond every id and block, and the product below never wraps)
        else u = u * 10 + (uint64_t)(*p - '0');
    }
    *v = neg ? -(int64_t)u : (int64_t)u;
    return true;
}

// The table from the bytes of a --blocks file (the header bgr_write_blocks writes, then lines of ten tab-separated fields; the last line may lack
// its newline).  Every block of the file tags.  false with *msg, which names the line.
inline bool haplotag_table_of_text(const char* data, uint64_t bytes, uint64_t n_unitigs, uint32_t* table, std::string* msg) {
    memset(table, 0, (n_unitigs + 1) * sizeof(uint32_t));
    const char* header = blocks_header();
    const uint64_t hl = strlen(header);
    if (bytes < hl || memcmp(data, header, hl) != 0) { *msg = "line 1 is not the header of a blocks file"; return false; }
    uint64_t line = 1;
    for (const char *p = data + hl, *end = data + bytes; p < end;) {
        ++line;
        const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
        const char* e = nl ? nl : end;
        const char* f[11];   // where the fields start; f[i + 1] - 1 ends field i
        uint32_t nf = 0;
        f[nf++] = p;
        for (const char* q = p; q < e; ++q)
            if (*q == '\t') { if (nf < 11) f[nf] = q + 1; ++nf; if (nf > 10) break; }
        const std::string where = "line " + std::to_string(line) + ": ";
        if (nf != 10) { *msg = where + "not ten tab-separated fields"; return false; }
        f[10] = e + 1;
        int64_t block = 0, a = 0, b = 0;
        if (!haplotag_dec(f[0], f[1] - 1, &block) || !haplotag_dec(f[6], f[7] - 1, &a) || !haplotag_dec(f[7], f[8] - 1, &b)) {
            *msg = where + "block, hapA and hapB are decimal integers";
            return false;
        }
        std::string m;
        if (!haplotag_pair(table, n_unitigs, block, a, b, &m)) { *msg = where + m; return false; }
        p = nl ? nl + 1 : end;
    }
    return true;
}

// The tag of one row's ids id_1 .. id_n (the row without its offset), as the device computes it: the smallest block among the votes, its votes for A
// and for B, the votes for other blocks
inline bgr_read_tag haplotag_row(const uint32_t* table, uint64_t n_unitigs, const int32_t* ids, uint64_t n) {
    bgr_read_tag t = {0, 0, 0, 0};
    uint32_t best = 0xFFFFFFFFu, votes = 0;
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t u = haplotag_abs(ids[j]);
        const uint32_t v = u >= 1 && u <= n_unitigs ? table[u] : 0u;
        if (v) { ++votes; if ((v >> 1) < best) best = v >> 1; }
    }
    if (!votes) return t;
    t.block = best;
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t u = haplotag_abs(ids[j]);
        const uint32_t v = u >= 1 && u <= n_unitigs ? table[u] : 0u;
        if (v && (v >> 1) == best) { if (v & 1u) ++t.b; else ++t.a; }
    }
    t.others = votes - t.a - t.b;
    return t;
}

// what a GAF line gains in front of its newline (nothing for block 0)
inline uint32_t haplotag_hp(const bgr_read_tag& t) { return t.a > t.b ? 1u : t.b > t.a ? 2u : 0u; }
inline void haplotag_suffix(const bgr_read_tag& t, std::string* out) {
    if (!t.block) return;
    *out += "\tPS:i:"; *out += std::to_string(t.block);
    *out += "\tHP:i:"; *out += std::to_string(haplotag_hp(t));
    *out += "\tha:i:"; *out += std::to_string(t.a);
    *out += "\thb:i:"; *out += std::to_string(t.b);
    *out += "\tho:i:"; *out += std::to_string(t.others);
}

}  // namespace bgr

#endif
