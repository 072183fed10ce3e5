// links_kernels.hip -- the links a greedy / anchors launch crosses (bgr_link, include/bgreat_gpu.h): behind the mapping passes one kernel reads
// every mapped read's row [off, id_1 .. id_n] from (results, arena) and adds 1 per consecutive pair (id_j, id_j+1) to the count of the pair's
// canonical form -- the smaller of key(a, b) and key(-b, -a), links_kernels.h -- in an open-addressed table of {u64 key, u64 count} in HBM.
// No read characters, no strand, no offset, no graph: the kernel needs the path ints and the number of unitigs, so one kernel serves every k.
//
// Geometry as the abundance kernel's: sixteen lanes share a read, lane i takes the pair (id_i, id_i+1) of a pass of sixteen; the pair that
// straddles two passes (unitig 16 of one, unitig 1 of the next) is lane 15's, which reads its second id from the next pass's first place.
//
// The table: linear probing from links_hash(key) & (capacity - 1); key 0 = an empty slot (ids are 1-based).  An insert reads the slot's key,
// claims an empty slot with a 64-bit atomicCAS, and adds to the count of the slot that holds its key with a no-return 64-bit atomicAdd.  A key
// is written once and never changes, so a key read without the CAS is final unless it is 0.  Every probe loop ends after `capacity` slots:
// an insert that found no place adds to the overflow word behind the table and the host refuses the counts (BGR_E_CAPACITY).
//
// Two forms (plan_links in links_kernels.h chooses):
//   A  every traversal is an insert into the table in HBM;
//   B  the same insert into a table of kLinksLdsSlots {u64 key, u32 count} in the workgroup's LDS, over at most kLinksLdsProbes slots; a
//      traversal that finds no place there goes to HBM as in form A.  The workgroup flushes its table once, one insert per used slot.
// Integer adds commute: the counts do not depend on the form, the geometry or the order of the launches.
#include <hip/hip_runtime.h>

#include "links_kernels.h"

namespace {

typedef unsigned long long ull;

// count[key] += v in the table in HBM; false = no place in `capacity` slots
__device__ __forceinline__ bool links_insert(ull* table, ull* used, uint64_t mask, uint64_t key, ull v) {
    uint64_t slot = bgr::links_hash(key) & mask;
    for (uint64_t probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
        ull* kp = table + 2 * slot;
        ull cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(kp, 0ull, (ull)key);
            if (cur == 0) { cur = key; atomicAdd(used, 1ull); }   // (claimed: once per distinct link of the table's lifetime)
        }
        if (cur == key) {
            atomicAdd(kp + 1, v);
            return true;
        }
    }
    return false;
}

}  // namespace

template <bool LDS>
__global__ void __launch_bounds__(LDS ? 1024 : 256) bgr_links_kernel(uint32_t n_unitigs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n_reads, ull* table,
                                                         uint64_t capacity) {
    __shared__ ull lds_keys[LDS ? bgr::kLinksLdsSlots : 1];
    __shared__ uint32_t lds_cnt[LDS ? bgr::kLinksLdsSlots : 1];
    __shared__ uint32_t lds_fell[2];   // [0]: the table turned a traversal away ([1] keeps the block at kLinksLdsBytes)
    const uint64_t mask = capacity - 1;
    ull* tail = table + 2 * capacity;   // [0] overflow, [1] workgroups of form B that fell through, [2] used slots
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < bgr::kLinksLdsSlots; i += blockDim.x) { lds_keys[i] = 0; lds_cnt[i] = 0; }
        if (threadIdx.x == 0) lds_fell[0] = 0;
        __syncthreads();
    }
    const uint32_t sub = threadIdx.x & 15, per_block = blockDim.x >> 4, stride = gridDim.x * per_block;
    for (uint32_t r = blockIdx.x * per_block + (threadIdx.x >> 4); r < n_reads; r += stride) {   // (one read per 16-lane group)
        const uint2 res = results[r];
        const uint32_t np = res.y & 0xFFFFFFu;
        if (np < 3 || (uint64_t)res.x + np > arena_ints) continue;   // not mapped, a path of one unitig -- or a row that is not in the arena
        const int32_t* ids = arena + res.x + 1;   // id_1 .. id_n, n = np - 1
        const uint32_t n_pairs = np - 2;
        for (uint32_t j = sub; j < n_pairs; j += 16) {
            const int32_t a = ids[j], b = ids[j + 1];   // (j + 1 <= n - 1: inside the row)
            const uint32_t ua = (uint32_t)(a < 0 ? -(int64_t)a : (int64_t)a), ub = (uint32_t)(b < 0 ? -(int64_t)b : (int64_t)b);
            if (ua == 0 || ub == 0 || ua > n_unitigs || ub > n_unitigs) continue;   // (as the abundance kernel skips such ids)
            const uint64_t key = bgr::links_canonical(a, b);
            bool done = false;
            if (LDS) {
                uint32_t s = (uint32_t)bgr::links_hash(key) & (bgr::kLinksLdsSlots - 1);
                for (uint32_t probe = 0; probe < bgr::kLinksLdsProbes && !done; ++probe, s = (s + 1) & (bgr::kLinksLdsSlots - 1)) {
                    ull cur = __hip_atomic_load(&lds_keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (cur == 0) {
                        cur = atomicCAS(&lds_keys[s], 0ull, (ull)key);
                        if (cur == 0) cur = key;
                    }
                    if (cur == key) { atomicAdd(&lds_cnt[s], 1u); done = true; }
                }
                if (!done) atomicOr(&lds_fell[0], 1u);
            }
            if (!done && !links_insert(table, tail + 2, mask, key, 1ull)) atomicAdd(tail, 1ull);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < bgr::kLinksLdsSlots; i += blockDim.x) {
            const ull key = lds_keys[i];
            if (key && !links_insert(table, tail + 2, mask, key, (ull)lds_cnt[i])) atomicAdd(tail, (ull)lds_cnt[i]);
        }
        if (threadIdx.x == 0 && lds_fell[0]) atomicAdd(tail + 1, 1ull);
    }
}

namespace bgr {

uint64_t links_bound_of_blob(const BgrBlobHeader* h, const uint8_t* base) {
    if (!h || !base) return 0;
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(base + h->off_meta);
    const BgrKeyEntry* keys = reinterpret_cast<const BgrKeyEntry*>(base + h->off_keys);   // (a wide entry s is read as entry 2 s: graph_layout.h)
    const BgrSlot* slots = reinterpret_cast<const BgrSlot*>(base + h->off_recs);
    const uint64_t step = h->wide_keys ? 2 : 1;
    // (a graph with exception planes: the reverse complement of a non-ACGT character is 'A', utils.cpp:66-73, so the two strands of a junction need
    // not agree on what a slot's unitig looks like; every slot counts in both orientations there)
    const bool twice = h->has_exc != 0;
    auto weight = [&](uint32_t rec, bool right) -> uint64_t {   // w(half): its slots, those with both orientation bits twice
        if (rec >= h->n_keys) return 0;
        const uint32_t hd = right ? keys[step * rec].hR : keys[step * rec].hL;
        if (hd == BGR_HNONE) return 0;
        uint64_t w = 0;
        for (uint64_t q = hd; q < h->n_slots; ++q) {
            const BgrSlot& sl = slots[q];
            w += 1 + (twice || ((sl.idf & BGR_SLOT_F0) && (sl.idf & BGR_SLOT_F1)) ? 1 : 0);
            if (sl.Fo_x & BGR_SLOT_LAST) break;
        }
        return w;
    };
    uint64_t bound = 0;
    for (uint64_t i = 1; i <= h->n_unitigs; ++i) {
        const BgrUnitigMeta& m = meta[i];
        // out of the end: the walk to the right asks getBegin(end), which reads the left half of a canonical key, else the right one; out of the
        // beginning: the walk to the left asks getEnd(beg), the other way round.  The walks of the other strand read the same halves -- but for
        // a (k-1)-mer that is its own reverse complement, where they read the other one.
        const bool ce = (m.flags & BGR_META_CANON_END) != 0, cre = (m.flags & BGR_META_CANON_RCEND) != 0;
        const bool cb = (m.flags & BGR_META_CANON_BEG) != 0, crb = (m.flags & BGR_META_CANON_RCBEG) != 0;
        if (ce && cre) bound += weight(m.rec_end, false) + weight(m.rec_end, true);
        else bound += weight(m.rec_end, !ce);
        if (cb && crb) bound += weight(m.rec_beg, false) + weight(m.rec_beg, true);
        else bound += weight(m.rec_beg, cb);
    }
    return bound;
}

hipError_t launch_links(uint64_t n_unitigs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n_reads, unsigned long long* table, uint64_t capacity,
                        const LinksPlan& plan, hipStream_t stream) {
    if (n_reads == 0 || plan.blocks == 0) return hipSuccess;
    if (n_unitigs >= 0x40000000ull) return hipErrorInvalidValue;   // (a graph has fewer than 2^30 unitigs: an id and its sign fit 31 bits of the key)
    if (!table || capacity < 2 || (capacity & (capacity - 1))) return hipErrorInvalidValue;
    if (plan.form == kLinksFormLds)
        hipLaunchKernelGGL(bgr_links_kernel<true>, dim3(plan.blocks), dim3(plan.threads), 0, stream, (uint32_t)n_unitigs, results, arena, arena_ints, n_reads, table, capacity);
    else
        hipLaunchKernelGGL(bgr_links_kernel<false>, dim3(plan.blocks), dim3(plan.threads), 0, stream, (uint32_t)n_unitigs, results, arena, arena_ints, n_reads, table, capacity);
    return hipGetLastError();
}

}  // namespace bgr
