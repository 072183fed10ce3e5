// triples_kernels.h -- launch interface of triples_kernels.hip: the unitig triples (three consecutive ids) that the rows of a greedy or anchors
// launch thread, counted into an open-addressed hash table in HBM (bgr_triple in include/bgreat_gpu.h has the definition), the packing of a
// triple into the table's two key words, and the table's size.
#ifndef BGREAT_AMD_TRIPLES_KERNELS_H
#define BGREAT_AMD_TRIPLES_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "graph_layout.h"
#include "links_kernels.h"

namespace bgr {

const uint32_t kTriplesLanes = 16;            // lanes that share one read (one triple of a pass of sixteen each)
const uint64_t kTriplesMinCapacity = 1024;    // slots of the smallest table in HBM
const uint32_t kTriplesSlotWords = 3;         // {k0, k1, count}
const uint32_t kTriplesTailWords = 2;         // behind the slots: [0] = traversals that found no place, [1] = used slots (= distinct triples)

// ---- the key -----------------------------------------------------------------------------------------------------------------------------------
// A triple (a, b, c) of signed 1-based ids is 3 x (30 + 1) = 93 bits: two words.  k0 = links_pack(a, b) -- (|a|, a < 0, |b|, b < 0), first field
// most significant -- and k1 = |c| << 1 | (c < 0).  The order of the pairs (k0, k1), compared word by word, IS the order of the tuples
// (|a|, a < 0, |b|, b < 0, |c|, c < 0) that the definition sorts by.  |a| >= 1 and |c| >= 1: neither word of a key is 0, which marks the empty word.
struct TripleKey { uint64_t k0, k1; };
BGR_HD uint64_t triples_pack1(int32_t c) {
    const uint64_t uc = (uint64_t)(c < 0 ? -(int64_t)c : (int64_t)c);
    return (uc << 1) | (uint64_t)(c < 0);
}
// (a, b, c) and (-c, -b, -a) are one triple read from the two strands: the one with the smaller (k0, k1) stands for both.  They always differ
// (b != -b), and so do their k0 or their k1.
BGR_HD TripleKey triples_canonical(int32_t a, int32_t b, int32_t c) {
    const TripleKey x = {links_pack(a, b), triples_pack1(c)}, y = {links_pack(-c, -b), triples_pack1(-a)};
    return (x.k0 < y.k0 || (x.k0 == y.k0 && x.k1 < y.k1)) ? x : y;
}
BGR_HD int32_t triples_key_to(uint64_t k1) { const int32_t v = (int32_t)(k1 >> 1); return k1 & 1 ? -v : v; }
// where a key's probe sequence starts (the table's capacity is a power of two; linear probing from there)
BGR_HD uint64_t triples_hash(uint64_t k0, uint64_t k1) { return links_hash(k0 ^ (k1 * 0x9E3779B97F4A7C15ULL)); }

// ---- the table's size ----------------------------------------------------------------------------------------------------------------------------
// How many distinct canonical triples the rows of any launch on this graph can hold, from the host blob alone.  A walk glues a unitig to the one
// before it only where the two overlap in exactly k-1 characters -- whatever half record and slot delivered the neighbour.  So in a triple
// (a, u, c) the oriented a ENDS with the first (k-1)-mer of the oriented u and the oriented c BEGINS with its last one.  Of a triple and its strand
// mate (-c, -u, -a) exactly one has its middle id positive, so the canonical triples are counted once each by their readings with u > 0:
//     distinct triples <= sum over the unitigs u of  E(first (k-1)-mer of u) x B(last (k-1)-mer of u)
// with B(S) = oriented unitigs that begin with S and E(S) = oriented unitigs that end with S = B(reverse complement of S).  B comes from one
// counting pass over the metas: unitig v begins with its `beg` and -v with the reverse complement of its `end`; rec_beg / rec_end name the
// (k-1)-mer's canonical form and the BGR_META_CANON_* flags say which of the two spellings the unitig carries (both for a (k-1)-mer that is its
// own reverse complement, which then counts under either spelling -- they are one string).  The count is over the unitigs themselves, not over the
// slots of a half record: the reference's slot-4 overwrite (aligner.cpp:466-533) drops unitigs from a full half, and a count that leaned on the
// slots would miss a neighbour that is reachable from its other side only.  On a graph with exception planes the reverse complement of a non-ACGT
// character is 'A' (utils.cpp:66-73) and the two strands of a junction need not agree on the spelling a unitig carries: every end counts under
// both spellings there, as links_bound_of_blob counts every slot twice.
// -> 0 for a graph without a host blob.
uint64_t triples_bound_of_blob(const BgrBlobHeader* h, const uint8_t* base);
// slots of the table for a bound: the power of two that is at least twice the bound (the table never gets more than half full: probe sequences stay short)
inline uint64_t triples_capacity(uint64_t bound) {
    uint64_t cap = kTriplesMinCapacity;
    while (cap < 2 * bound && cap < (1ull << 62)) cap <<= 1;
    return cap;
}

// table: u64[3 * capacity] = {k0, k1, count} per slot, then u64[kTriplesTailWords].  arena_ints: ints the arena buffer holds (a row that would
// end beyond it is skipped).  One form: every traversal is an insert into the table in HBM (no table in LDS in front of it: on a graph of a
// handful of triples all adds of a launch meet in a few addresses and serialise, as the links kernel's form A does there).  Launches nothing for
// zero reads.
inline uint64_t triples_table_bytes(uint64_t capacity) { return (kTriplesSlotWords * capacity + kTriplesTailWords) * 8; }
hipError_t launch_triples(uint64_t n_unitigs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n_reads, unsigned long long* table, uint64_t capacity,
                          uint32_t num_cus, hipStream_t stream);

}  // namespace bgr

#endif
