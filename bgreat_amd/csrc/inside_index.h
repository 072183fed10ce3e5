// inside_index.h -- the inside index: an exact hash table over a sample of the k-mers of every unitig, for the reads greedy mode leaves
// without an anchor because they lie wholly inside one unitig (no overlap (k-1)-mer of the graph occurs in them).  Built on the host
// (inside_index.cpp), read on the device by bgr_align_inside_kernel (inside_kernels.hip).  Shared by g++ and hipcc; no HIP types in here.
//
// k-mer word: the 2k-bit word of the graph's 2-bit code (graph_layout.h), first base most significant; k <= 32.  canonical = the smaller of
// the word and the word of its reverse complement; a k-mer that is its own reverse complement is never in the index.  A k-mer is SELECTED
// when bgr_jump_selects(bgr_mix64(canonical)) holds -- the one-in-BGR_JUMP_STRIDE rule of the jump index, a function of the k-mer alone, so
// a read knows without touching memory which of its windows can be in the index.
// For every unitig id and every offset 0 <= j <= len - k whose k-mer is selected the index holds canonical -> (id, j, "the forward window is
// the canonical one"); where a k-mer occurs more than once (any unitig set that is no compacted de Bruijn graph) the smallest (id, j) wins.
// The table is exact: open addressing with linear probing over {key, value} entries of 16 bytes, membership decided by comparing the key,
// nothing dropped.  slots = twice the selected windows (repeats counted), so the load is at most 0.5: a quarter of the graph's k-mers at
// 32 bytes each = AT MOST 8 BYTES PER GRAPH BASE, reached by long unitigs (measured: 45 MB = 5.2 bytes per base on an 8.6 M-base graph whose
// unitigs of 87 bases hold 57 k-mers each; about 3 GB at 390 M bases).
// Where an entry starts probing: bgr_jump_selects fixes bits 40 and 41 of m = bgr_mix64(canonical) of every selected k-mer, and the high
// bits of m decide a multiplicative slot choice -- of a table beyond 2^22 slots three slots in four could then never be a first choice.
// So the slot comes from a second multiply of m (bgr_inside_slot), whose high bits depend on all of m.
#ifndef BGREAT_AMD_INSIDE_INDEX_H
#define BGREAT_AMD_INSIDE_INDEX_H

#include <stdint.h>

#include "graph_layout.h"

typedef struct {
    uint64_t key;   // the canonical k-mer; BGR_EMPTY_KEY: an empty slot (T^32 is never canonical, its reverse complement is 0)
    uint64_t val;   // id << 33 | j << 1 | (the forward window is the canonical one): ordered as (id, j)
} BgrInsideEntry;   // 16 B
#define BGR_INSIDE_FWD_CANON 1ull

BGR_HD uint64_t bgr_inside_val(uint32_t id, uint32_t j, bool fwd_canon) { return ((uint64_t)id << 33) | ((uint64_t)j << 1) | (fwd_canon ? 1ull : 0ull); }
BGR_HD uint32_t bgr_inside_id(uint64_t val) { return (uint32_t)(val >> 33); }
BGR_HD uint32_t bgr_inside_off(uint64_t val) { return (uint32_t)(val >> 1); }
// the slot where the probe sequence of a k-mer with m = bgr_mix64(canonical) starts, 0 .. slots - 1
BGR_HD uint64_t bgr_inside_slot(uint64_t m, uint64_t slots) {
    const uint64_t h = (m ^ (m >> 29)) * 0xBF58476D1CE4E5B9ULL;
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(h, slots);
#else
    return (uint64_t)(((unsigned __int128)h * slots) >> 64);
#endif
}

#ifdef __cplusplus
#include <string>

namespace bgr {

struct InsideIndex {
    BgrInsideEntry* tab = nullptr;   // `slots` entries (malloc)
    uint64_t slots = 0, entries = 0; // entries: distinct k-mers placed
    double build_seconds = 0;
    InsideIndex() = default;
    InsideIndex(const InsideIndex&) = delete;
    InsideIndex& operator=(const InsideIndex&) = delete;
    ~InsideIndex() { release(); }
    void release();
    uint64_t bytes() const { return slots * sizeof(BgrInsideEntry); }
};

// Builds the index of the graph whose blob lies at `base` with T threads.  0: built; 1: the graph cannot have one (k > 32, exception planes), err
// says why; 2: no memory, nothing left allocated.
int build_inside_index(const BgrBlobHeader* h, const uint8_t* base, unsigned T, InsideIndex& out, std::string& err);
// The entry of a k-mer word (either strand): true and *val when the index holds its canonical form.
bool inside_lookup(const InsideIndex& ix, uint32_t k, uint64_t kmer, uint64_t* val);

}  // namespace bgr
#endif

#endif
