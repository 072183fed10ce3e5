// links_kernels.h -- launch interface of links_kernels.hip: the links (consecutive unitig pairs) that the rows of a greedy or anchors launch
// cross, counted into an open-addressed hash table in HBM (bgr_link in include/bgreat_gpu.h has the definition), the packing of a link into
// the table's 64-bit key, the table's size, and the choice between the kernel's two forms.
#ifndef BGREAT_AMD_LINKS_KERNELS_H
#define BGREAT_AMD_LINKS_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "graph_layout.h"

namespace bgr {

const uint32_t kLinksFormGlobal = 1;   // form A: every traversal is an insert into the table in HBM (64-bit atomicCAS on the key, no-return 64-bit atomicAdd on the count)
const uint32_t kLinksFormLds = 2;      // form B: a small table per workgroup in LDS (64-bit keys, 32-bit counts), flushed once into the table in HBM
const uint32_t kLinksLanes = 16;       // lanes that share one read (one pair of a pass of sixteen each)
const uint32_t kLinksLdsSlots = 2048;  // form B's table: 2048 x (8 + 4) bytes = 24 KB per workgroup, two workgroups of 1024 threads per CU
const uint32_t kLinksLdsProbes = 16;   // slots form B looks at before it hands a traversal to the table in HBM (its table is full, or nearly)
const uint32_t kLinksLdsBytes = kLinksLdsSlots * 12 + 8;   // the kernel's static arrays: keys, counts, and two words of flags
const uint64_t kLinksMinCapacity = 1024;   // slots of the smallest table in HBM

// ---- the key -----------------------------------------------------------------------------------------------------------------------------------
// A link (a, b) of signed 1-based ids packs into (|a|, a < 0, |b|, b < 0) = 30 + 1 + 30 + 1 bits, first field most significant, so that the order
// of the 64-bit integers IS the order of the tuples that the definition sorts by.  |a| >= 1: no key is 0, which marks the empty slot.
BGR_HD uint64_t links_pack(int32_t a, int32_t b) {
    const uint64_t ua = (uint64_t)(a < 0 ? -(int64_t)a : (int64_t)a), ub = (uint64_t)(b < 0 ? -(int64_t)b : (int64_t)b);
    return (ua << 33) | ((uint64_t)(a < 0) << 32) | (ub << 1) | (uint64_t)(b < 0);
}
// (a, b) and (-b, -a) are one link: the one with the smaller key stands for both
BGR_HD uint64_t links_canonical(int32_t a, int32_t b) {
    const uint64_t x = links_pack(a, b), y = links_pack(-b, -a);
    return x < y ? x : y;
}
BGR_HD int32_t links_key_from(uint64_t key) { const int32_t v = (int32_t)(key >> 33); return (key >> 32) & 1 ? -v : v; }
BGR_HD int32_t links_key_to(uint64_t key) { const int32_t v = (int32_t)((key >> 1) & 0x7FFFFFFFu); return key & 1 ? -v : v; }
// where a key's probe sequence starts (the table's capacity is a power of two; linear probing from there)
BGR_HD uint64_t links_hash(uint64_t key) {
    key ^= key >> 33; key *= 0xFF51AFD7ED558CCDULL;
    key ^= key >> 33; key *= 0xC4CEB9FE1A85EC53ULL;
    return key ^ (key >> 33);
}

// ---- the table's size ----------------------------------------------------------------------------------------------------------------------------
// How many distinct canonical links the rows of any launch on this graph can hold, from the host blob alone.  A walk reaches a neighbour in one way
// only: it stands on a unitig u, leaves it through one of its two ends, and takes a slot of the half record that this end's (k-1)-mer names:
// key meta[u].rec_end / rec_beg, and of its two halves the one that the query's direction and canonical flag select (graph_build.cpp, "the walk
// goes LEFT exactly when c == side").  The walk to the right out of u's end and the walk to the left out of the reverse complement's are the
// same junction on the two strands: their queries are each other's reverse complement (c and !c), they read the SAME half, and a slot answers
// them with its two orientation bits, F0 for c = 1 and F1 for c = 0.  For a slot with one of the bits the two answers are strand mates -- (u, v)
// and (-v, -u): one canonical link; a slot with both (a hairpin: the unitig begins with the key and ends with its reverse complement) gives two.
// An end whose (k-1)-mer is its own reverse complement is canonical both ways and reads either half, depending on the direction.  So
//     distinct links <= sum over the 2 x n_unitigs ends of w(the half it reads)      w(half) = slots of the half + those of them with F0 and F1
// (both halves for a palindromic end; on a graph with exception planes, where the strands need not agree, every slot counts twice).  Every link is reached from an end, so none is missed; one that both of its ends reach is counted twice,
// which is kept: the reference's slot-4 overwrite (aligner.cpp:466-533) drops unitigs from a full half, so a link can be reachable from one side only.
// On a graph without such halves this is at most the sum over the keys of (left slots + right slots)^2 / 2 + hairpins.
// -> 0 for a graph without a host blob.
uint64_t links_bound_of_blob(const BgrBlobHeader* h, const uint8_t* base);
// slots of the table for a bound: the power of two that is at least twice the bound (the table never gets more than half full: probe sequences stay short)
inline uint64_t links_capacity(uint64_t bound) {
    uint64_t cap = kLinksMinCapacity;
    while (cap < 2 * bound) cap <<= 1;
    return cap;
}

// ---- the forms ---------------------------------------------------------------------------------------------------------------------------------------
// Automatic choice: form B exactly where the graph cannot fill a workgroup's table beyond a half -- links_bound <= kLinksLdsSlots / 2.  There B never
// falls through, a workgroup sends each of its distinct links to HBM once, and the atomics of the launch drop from one per traversal to at most
// (workgroups x distinct links); those are the graphs on which A serialises, a few addresses taking every add of the launch.  Beyond that
// bound the traversals of a workgroup (64 reads in flight, a few thousand per workgroup and launch) spread over more links than its table holds:
// most inserts probe kLinksLdsProbes slots in LDS and then go to HBM anyway, and the flush adds a second insert for those that stayed.
// Measured on an MI355X (tools/links_rate.py, profiles/links_rate.txt: 262 144 reads per launch, k = 31, 150 bp reads, 100 bp on the last graph;
// kernel milliseconds per launch, and the whole launch in Mreads/s with the counting off -> on):
//     graph                          bound       links met   form A                 form B                 automatic
//     six unitigs, every read there         10           5   2.284 ms (3 841 ->  112)  0.028 ms (-> 2 785)    B
//     genome 300 k, 6 388 unitigs       17 032       8 516   0.056 ms (2 206 -> 1 533)  0.058 ms (-> 1 515)    A
//     bench.py's default, 98 866       263 640     126 638   0.032 ms (1 951 -> 1 611)  0.039 ms (-> 1 532)    A
//     chr1 scale, 3 966 085         10 576 224     328 356   0.034 ms (1 301 -> 1 120)  0.035 ms (-> 1 107)    A
// On five links form A serialises as the abundance kernel's did (2.3 ms; that one 6.8 ms with three adds per occurrence) and form B is eighty times
// faster: the automatic choice there is B, the faster one.  From 8 516 links on, B buys nothing: A is level with it or ahead (by a fifth on the default
// graph), and B's table already turns traversals away in most workgroups (438 of 512 on the 300 k graph, with 800 traversals per workgroup in 2 048
// slots: a run of sixteen taken slots is met now and then even at that fill; they cost an insert into HBM, not correctness).  So the cutoff lies
// somewhere between a bound of 10 and one of 17 032, nothing measured separates the values in between, and it stays where B provably never falls
// through.  B's table size, its sixteen probes and its two workgroups per CU were not varied: on the one shape where B runs by default its kernel is
// 0.028 ms of a 0.10 ms launch, next to the abundance kernel's 0.026 ms there.  Against the abundance kernel on the same graphs
// (profiles/abundance_rate.txt: 0.070 / 0.038 / 0.060 ms on default / 300 k / chr1) the links kernel takes 0.032 / 0.056 / 0.034 ms.
const uint64_t kLinksLdsAutoBound = kLinksLdsSlots / 2;

struct LinksPlan {
    uint32_t form = kLinksFormGlobal, blocks = 0, threads = 256, lds_bytes = 0;
};

// A pure function of the numbers (no device): want = 0 automatic, 1 form A, 2 form B.  B's 32-bit counts cannot wrap: a launch's rows lie in an arena
// of fewer than 2^32 ints, and every traversal is a pair of neighbouring ints of it.
inline LinksPlan plan_links(uint64_t links_bound, uint64_t n_reads, uint32_t num_cus, uint32_t want) {
    LinksPlan p;
    if (!num_cus) num_cus = 256;
    const bool lds = want == kLinksFormLds || (want == 0 && links_bound <= kLinksLdsAutoBound);
    p.form = lds ? kLinksFormLds : kLinksFormGlobal;
    p.threads = lds ? 1024 : 256;
    p.lds_bytes = lds ? kLinksLdsBytes : 0;
    const uint64_t groups = p.threads / kLinksLanes, most = lds ? (uint64_t)num_cus * 2 : (uint64_t)num_cus * 64;   // (a grid-stride loop over the reads)
    uint64_t blocks = (n_reads + groups - 1) / groups;
    if (blocks > most) blocks = most;
    p.blocks = (uint32_t)blocks;
    return p;
}

// table: u64[2 * capacity] = {key, count} per slot, then u64[kLinksTailWords]: [0] = traversals that found no place (the table is full: the
// counts are incomplete), [1] = workgroups of form B whose LDS table sent at least one traversal straight to HBM, [2] = used slots (= distinct links).  arena_ints: ints the arena
// buffer holds (a row that would end beyond it is skipped).  Launches nothing for zero reads.
const uint32_t kLinksTailWords = 3;
inline uint64_t links_table_bytes(uint64_t capacity) { return (2 * capacity + kLinksTailWords) * 8; }
hipError_t launch_links(uint64_t n_unitigs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n_reads, unsigned long long* table, uint64_t capacity,
                        const LinksPlan& plan, hipStream_t stream);

}  // namespace bgr

#endif
