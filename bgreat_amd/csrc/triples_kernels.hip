// triples_kernels.hip -- the unitig triples a greedy / anchors launch threads (bgr_triple, include/bgreat_gpu.h): behind the mapping passes one
// kernel reads every mapped read's row [off, id_1 .. id_n] from (results, arena) and adds 1 per three consecutive ids (id_j, id_j+1, id_j+2) to
// the count of the triple's canonical form -- the smaller of key(a, b, c) and key(-c, -b, -a), triples_kernels.h -- in an open-addressed table
// of {u64 k0, u64 k1, u64 count} in HBM.  No read characters, no strand, no offset, no graph: the kernel needs the path ints and the number of
// unitigs, so one kernel serves every k.
//
// Geometry as the links kernel's: sixteen lanes share a read, lane i takes the triple (id_i, id_i+1, id_i+2) of a pass of sixteen; the two
// triples that straddle two passes are lanes 14's and 15's, which read their last ids from the next pass's first places.
//
// The table: linear probing from triples_hash(k0, k1) & (capacity - 1); a word that is 0 is empty (ids are 1-based: no word of a key is 0).  The
// key does not fit one compare-and-swap, so a slot is claimed word by word.  An insert of (k0, k1), at each slot of its probe sequence:
//   1  load the slot's k0; if it is 0, atomicCAS(k0, 0, mine);
//   2  if the slot's k0 is not mine: next slot;
//   3  load the slot's k1; if it is 0, atomicCAS(k1, 0, mine);
//   4  if the slot's k1 is mine: no-return 64-bit atomicAdd on the count, done;
//   5  else: next slot.
// No lock, no spin: no step waits for another thread.  Why no key ends up in two slots:
//   - each word is written once, by a CAS from 0, and never changes afterwards: a word read as non-zero is final;
//   - a thread passes a slot only when a word of it is finally different from its key's (step 2 or step 5);
//   - so a slot that ends up holding the key K was never passed by a thread that carried K: every such thread that reached it stopped there, and
//     a thread reaches a slot only by passing all slots before it on K's one probe sequence -- K sits in the first slot of the sequence that
//     holds it and in no later one;
//   - a slot whose k0 was claimed by one thread and whose k1 was set by another, with the same (a, b) and another c, is a consistent slot of that
//     other key; the first thread sees a k1 that is not its own and moves on (step 5);
//   - every thread that claims a k0 goes on to the CAS on k1 in the same loop iteration, so when the kernel has ended no slot has its k0 set and
//     its k1 empty: the host takes a slot as used exactly when its k1 is not 0.
// The thread whose CAS on k1 succeeded from 0 adds 1 to the used-slots word.  Every probe loop ends after `capacity` slots: an insert that found
// no place adds to the overflow word behind the table and the host refuses the counts (BGR_E_CAPACITY).  All atomics are relaxed and of agent
// scope: the table is read only after the stream has been waited for.  Integer adds commute: the counts do not depend on the geometry or on the
// order of the launches.
#include <hip/hip_runtime.h>

#include <vector>

#include "triples_kernels.h"

namespace {

typedef unsigned long long ull;

// count[(k0, k1)] += 1 in the table in HBM; false = no place in `capacity` slots
__device__ __forceinline__ bool triples_insert(ull* table, ull* used, uint64_t mask, uint64_t k0, uint64_t k1) {
    uint64_t slot = bgr::triples_hash(k0, k1) & mask;
    for (uint64_t probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
        ull* sp = table + bgr::kTriplesSlotWords * slot;
        ull c0 = __hip_atomic_load(sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c0 == 0) {
            c0 = atomicCAS(sp, 0ull, (ull)k0);
            if (c0 == 0) c0 = k0;
        }
        if (c0 != k0) continue;
        ull c1 = __hip_atomic_load(sp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c1 == 0) {
            c1 = atomicCAS(sp + 1, 0ull, (ull)k1);
            if (c1 == 0) { c1 = k1; atomicAdd(used, 1ull); }   // (claimed: once per distinct triple of the table's lifetime)
        }
        if (c1 == k1) {
            atomicAdd(sp + 2, 1ull);
            return true;
        }
    }
    return false;
}

}  // namespace

__global__ void __launch_bounds__(256) bgr_triples_kernel(uint32_t n_unitigs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n_reads, ull* table,
                                                          uint64_t capacity) {
    const uint64_t mask = capacity - 1;
    ull* tail = table + bgr::kTriplesSlotWords * capacity;   // [0] overflow, [1] used slots
    const uint32_t sub = threadIdx.x & 15, per_block = blockDim.x >> 4, stride = gridDim.x * per_block;
    for (uint32_t r = blockIdx.x * per_block + (threadIdx.x >> 4); r < n_reads; r += stride) {   // (one read per 16-lane group)
        const uint2 res = results[r];
        const uint32_t np = res.y & 0xFFFFFFu;
        if (np < 4 || (uint64_t)res.x + np > arena_ints) continue;   // not mapped, a path of one or two unitigs -- or a row that is not in the arena
        const int32_t* ids = arena + res.x + 1;   // id_1 .. id_n, n = np - 1
        const uint32_t n_triples = np - 3;        // n - 2
        for (uint32_t j = sub; j < n_triples; j += 16) {
            const int32_t a = ids[j], b = ids[j + 1], c = ids[j + 2];   // (j <= n - 3, so j + 2 <= n - 1: inside the row)
            const uint32_t ua = (uint32_t)(a < 0 ? -(int64_t)a : (int64_t)a), ub = (uint32_t)(b < 0 ? -(int64_t)b : (int64_t)b), uc = (uint32_t)(c < 0 ? -(int64_t)c : (int64_t)c);
            if (ua == 0 || ub == 0 || uc == 0 || ua > n_unitigs || ub > n_unitigs || uc > n_unitigs) continue;   // (INT32_MIN is 2^31 here: beyond; nothing is negated before this)
            const bgr::TripleKey key = bgr::triples_canonical(a, b, c);
            if (!triples_insert(table, tail + 1, mask, key.k0, key.k1)) atomicAdd(tail, 1ull);
        }
    }
}

namespace bgr {

uint64_t triples_bound_of_blob(const BgrBlobHeader* h, const uint8_t* base) {
    if (!h || !base) return 0;
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(base + h->off_meta);
    // begins[2 r + 0]: oriented unitigs that begin with the canonical spelling of key r's (k-1)-mer, [2 r + 1]: with the other spelling
    std::vector<uint32_t> begins(2 * h->n_keys, 0);
    const bool twice = h->has_exc != 0;   // (the strands need not agree on a spelling there: triples_kernels.h)
    auto add = [&](uint32_t rec, bool canonical, bool other) {
        if (rec >= h->n_keys) return;
        if (canonical || twice) ++begins[2 * (uint64_t)rec];
        if (other || twice) ++begins[2 * (uint64_t)rec + 1];
    };
    for (uint64_t i = 1; i <= h->n_unitigs; ++i) {
        const BgrUnitigMeta& m = meta[i];
        add(m.rec_beg, (m.flags & BGR_META_CANON_BEG) != 0, (m.flags & BGR_META_CANON_RCBEG) != 0);   // +i begins with beg
        add(m.rec_end, (m.flags & BGR_META_CANON_RCEND) != 0, (m.flags & BGR_META_CANON_END) != 0);   // -i begins with the reverse complement of end
    }
    uint64_t bound = 0;
    for (uint64_t i = 1; i <= h->n_unitigs; ++i) {
        const BgrUnitigMeta& m = meta[i];
        if (m.rec_beg >= h->n_keys || m.rec_end >= h->n_keys) continue;
        // E(beg) = B(reverse complement of beg): the other spelling's count when beg is the canonical one; B(end): end's own spelling
        const uint64_t in = begins[2 * (uint64_t)m.rec_beg + ((m.flags & BGR_META_CANON_BEG) ? 1 : 0)];
        const uint64_t out = begins[2 * (uint64_t)m.rec_end + ((m.flags & BGR_META_CANON_END) ? 0 : 1)];
        bound += in * out;
    }
    return bound;
}

hipError_t launch_triples(uint64_t n_unitigs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n_reads, unsigned long long* table, uint64_t capacity,
                          uint32_t num_cus, hipStream_t stream) {
    if (n_reads == 0) return hipSuccess;
    if (n_unitigs >= 0x40000000ull) return hipErrorInvalidValue;   // (a graph has fewer than 2^30 unitigs: an id and its sign fit 31 bits of the key)
    if (!table || capacity < 2 || (capacity & (capacity - 1))) return hipErrorInvalidValue;
    if (!num_cus) num_cus = 256;
    const uint64_t groups = 256 / kTriplesLanes, most = (uint64_t)num_cus * 64;   // (a grid-stride loop over the reads)
    uint64_t blocks = ((uint64_t)n_reads + groups - 1) / groups;
    if (blocks > most) blocks = most;
    hipLaunchKernelGGL(bgr_triples_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, (uint32_t)n_unitigs, results, arena, arena_ints, n_reads, table, capacity);
    return hipGetLastError();
}

}  // namespace bgr
