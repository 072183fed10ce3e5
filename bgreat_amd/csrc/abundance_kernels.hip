// abundance_kernels.hip -- per-unitig abundance of a greedy / anchors launch (bgr_run_options.abundance, include/bgreat_gpu.h): behind the
// mapping passes one kernel reads every mapped read's row [off, id_1 .. id_n] from (results, arena) and adds, for every occurrence j of a
// unitig, 1 to reads[|id_j|], o_j to bases[|id_j|] and max(0, o_j - (k-1)) to kmers[|id_j|], where o_j is the stretch of the walk positions
// [off, off + cl) that lies on unitig j.  No read characters, no strand, no key compare: the kernel needs the path ints, the read's length
// and the unitig lengths of BgrUnitigMeta, so one kernel serves every k.
//
// Geometry as gaf_stat's (text_gaf.hip): sixteen lanes share a read, lane i takes unitig i of a pass of sixteen, a prefix sum by shuffles
// places every unitig in the walk (e_j = e_{j-1} - (k-1) + len_j); a path of any length takes ceil(n / 16) passes with the walk's size so far
// carried from one to the next.  With e_j <= plen the covered stretch needs no second pass for plen:
//     o_j = max(0, min(off + cl, e_j) - max(off, s_j)) = max(0, min(off + L, e_j) - max(off, s_j))      (cl = max(0, min(L, plen - off)))
//
// Two forms of the adds (plan_abundance in abundance_kernels.h chooses):
//   A  no-return device-scope 64-bit atomicAdd on the table in HBM (global_atomic_add_x2), three per occurrence at most;
//   B  the same adds on a table of 32-bit counters in the workgroup's LDS, flushed once per workgroup with 64-bit atomics on the entries
//      that are not zero.  Only for launches whose size keeps every counter below 2^32 (plan_abundance: k x total_bases < 2^32).
// Integer adds commute: the table does not depend on the form, the geometry or the order of the launches.
#include <hip/hip_runtime.h>

#include "abundance_kernels.h"

namespace {

typedef unsigned long long ull;

__device__ __forceinline__ int64_t grp16_up64(int64_t x, uint32_t d) {   // shuffles inside a 16-lane group, 64-bit by halves
    const uint64_t u = (uint64_t)x;
    return (int64_t)(((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(u >> 32), d, 16) << 32) | (uint32_t)__shfl_up((int)(uint32_t)u, d, 16));
}
__device__ __forceinline__ int64_t grp16_get64(int64_t x, uint32_t l) {
    const uint64_t u = (uint64_t)x;
    return (int64_t)(((uint64_t)(uint32_t)__shfl((int)(uint32_t)(u >> 32), (int)l, 16) << 32) | (uint32_t)__shfl((int)(uint32_t)u, (int)l, 16));
}

template <bool LDS>
__device__ __forceinline__ void add_to(uint32_t* lds_tab, ull* table, uint32_t idx, uint32_t v) {
    if (LDS) atomicAdd(&lds_tab[idx], v);   // (no counter of a launch that plan_abundance gives form B reaches 2^32)
    else atomicAdd(&table[idx], (ull)v);
}

}  // namespace

template <bool LDS>
__global__ void __launch_bounds__(1024) bgr_abundance_kernel(const BgrUnitigMeta* meta, uint32_t K1, uint32_t n_unitigs, const uint2* results, const int32_t* arena,
                                                             uint64_t arena_ints, const uint64_t* read_offs, uint32_t n_reads, ull* table) {
    extern __shared__ uint32_t lds_tab[];
    const uint32_t entries = 3 * (n_unitigs + 1);
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < entries; i += blockDim.x) lds_tab[i] = 0;
        __syncthreads();
    }
    const uint32_t sub = threadIdx.x & 15, per_block = blockDim.x >> 4, stride = gridDim.x * per_block;
    for (uint32_t r = blockIdx.x * per_block + (threadIdx.x >> 4); r < n_reads; r += stride) {   // (one read per 16-lane group: the flow below is uniform in a group)
        const uint2 res = results[r];
        const uint32_t np = res.y & 0xFFFFFFu;
        if (np < 2 || (uint64_t)res.x + np > arena_ints) continue;   // not mapped (an empty row) -- or a row that is not in the arena
        const int32_t* path = arena + res.x;
        const int64_t off = path[0];
        const int64_t hi = off + (int64_t)(read_offs[r + 1] - read_offs[r]);   // the read covers the walk positions [off, min(hi, plen))
        const uint32_t nu = np - 1;
        int64_t total = 0;   // e of the last unitig of the pass before
        for (uint32_t u0 = 0; u0 < nu; u0 += 16) {
            const uint32_t u = u0 + sub;
            const bool on = u < nu;
            const int32_t sid = on ? path[1 + u] : 0;
            const uint32_t id = (uint32_t)(sid < 0 ? -(int64_t)sid : (int64_t)sid);
            const bool ok = on && id != 0 && id <= n_unitigs;
            const int64_t len = ok ? (int64_t)meta[id].len : 0;
            const int64_t grow = on ? len - (u == 0 ? 0 : (int64_t)K1) : 0;   // e_j - e_{j-1}
            int64_t inc = grow;
#pragma unroll
            for (uint32_t d = 1; d < 16; d <<= 1) { const int64_t up = grp16_up64(inc, d); if (sub >= d) inc += up; }
            const int64_t e = total + inc, s = e - len;
            total = grp16_get64(e, 15);   // (lanes behind the path's end add nothing: lane 15 holds the pass's last e)
            if (ok) {
                const int64_t a = off > s ? off : s, b = hi < e ? hi : e;
                const int64_t o = b > a ? b - a : 0;
                add_to<LDS>(lds_tab, table, 3 * id, 1u);
                if (o > 0) add_to<LDS>(lds_tab, table, 3 * id + 1, (uint32_t)o);
                if (o > (int64_t)K1) add_to<LDS>(lds_tab, table, 3 * id + 2, (uint32_t)(o - (int64_t)K1));
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < entries; i += blockDim.x) {
            const uint32_t v = lds_tab[i];
            if (v) atomicAdd(&table[i], (ull)v);
        }
    }
}

namespace bgr {

hipError_t prepare_abundance(uint64_t lds_per_cu) {
    const uint64_t most = lds_per_cu && lds_per_cu < kAbundanceLdsMax ? lds_per_cu : kAbundanceLdsMax;   // (what plan_abundance lets a table have)
    if (most <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&bgr_abundance_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
}

hipError_t launch_abundance(const BgrDeviceGraph& g, uint64_t n_unitigs, const uint2* results, const int32_t* arena, uint64_t arena_ints, const uint64_t* read_offs,
                            uint32_t n_reads, unsigned long long* table, const AbundancePlan& plan, hipStream_t stream) {
    if (n_reads == 0 || plan.blocks == 0) return hipSuccess;
    if (n_unitigs >= 0x40000000ull) return hipErrorInvalidValue;   // (a graph has fewer than 2^30 unitigs: 3 * id fits 32 bits)
    const uint32_t K1 = g.k - 1, nu = (uint32_t)n_unitigs;
    if (plan.form == kAbundanceFormLds) {
        if (plan.lds_bytes < 12ull * (n_unitigs + 1)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(bgr_abundance_kernel<true>, dim3(plan.blocks), dim3(plan.threads), plan.lds_bytes, stream, g.meta, K1, nu, results, arena, arena_ints, read_offs,
                           n_reads, table);
    } else {
        hipLaunchKernelGGL(bgr_abundance_kernel<false>, dim3(plan.blocks), dim3(plan.threads), 0, stream, g.meta, K1, nu, results, arena, arena_ints, read_offs, n_reads, table);
    }
    return hipGetLastError();
}

}  // namespace bgr
