// bubbles_kernels.hip -- bubbles of the graph that a set of counted links spans (bgr_bubble, include/bgreat_gpu.h): adjacency from the {key, count}
// pairs with one atomic per oriented edge, then count / scan / emit over tiles of oriented ids (bubbles_kernels.h has the passes).  Pass 1 is bound
// by the bytes of the pairs it reads (an aligner's table is mostly empty slots), passes 2 and 4 by the four bytes of deg per oriented id: only an id
// of out-degree 2 goes on to the handful of dependent loads of the rule.
#include <hip/hip_runtime.h>

#include "bubbles_kernels.h"
#include "links_kernels.h"
#include "variants_kernels.h"

namespace {

typedef unsigned long long u64;
constexpr uint32_t kTile = bgr::kBubblesTile, kThreads = bgr::kBubblesThreads, kPer = kTile / kThreads;
static_assert(kPer == 4 && kThreads == 256, "a thread owns one uint4 of deg words; four waves per workgroup");

// exclusive scan of v over the workgroup's 256 threads; *total = the sum.  sw: four LDS words.  Every thread calls it.
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* sw, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= (uint32_t)off) incl += t;
    }
    if (lane == 63u) sw[wave] = incl;
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < kThreads / 64; ++i) { const uint32_t s = sw[i]; all += s; if (i < wave) pre += s; }
    *total = all;
    return pre + incl - v;
}

// one oriented edge from -> dest joins the adjacency
__device__ __forceinline__ void add_edge(uint32_t* deg, int32_t* to, uint64_t* cnt, int32_t from, int32_t dest, uint64_t count) {
    const u64 o = bgr::bubbles_o(from);
    const uint32_t r = atomicAdd(deg + o, 1u);
    if (r < 2u) { to[2 * o + r] = dest; cnt[2 * o + r] = count; }
}

}  // namespace

// pass 1: one thread per pair
__global__ void __launch_bounds__(256) bgr_bubbles_adjacency_kernel(const ulonglong2* pairs, u64 n_pairs, u64 n_unitigs, u64 min_link, uint32_t* deg, int32_t* to, uint64_t* cnt) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    const ulonglong2 kv = pairs[i];
    if (kv.x == 0 || kv.y < min_link) return;
    const int32_t a = bgr::links_key_from(kv.x), b = bgr::links_key_to(kv.x);
    const u64 ua = bgr::bubbles_abs(a), ub = bgr::bubbles_abs(b);
    if (ua == 0 || ub == 0 || ua > n_unitigs || ub > n_unitigs) return;   // (nothing is ever written beyond the 2 n oriented ids)
    add_edge(deg, to, cnt, a, b, kv.y);
    if (b != -a) add_edge(deg, to, cnt, -b, -a, kv.y);
}

// passes 2 and 4
template <bool EMIT>
__global__ void __launch_bounds__(256) bgr_bubbles_classify_kernel(u64 n_unitigs, const uint32_t* deg, const int32_t* to, const uint64_t* cnt, uint32_t* counts, const uint64_t* offs, bgr_bubble* out) {
    __shared__ uint32_t sw[kThreads / 64];
    const u64 o0 = (u64)blockIdx.x * kTile + threadIdx.x * kPer, ids = 2 * n_unitigs;
    const uint4 d4 = *reinterpret_cast<const uint4*>(deg + o0);   // (deg holds whole tiles)
    const uint32_t d[kPer] = {d4.x, d4.y, d4.z, d4.w};
    bgr_bubble rec[kPer];
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i)
        if (d[i] == 2u && o0 + i < ids && bgr::bubble_at(deg, to, cnt, n_unitigs, bgr::bubbles_id_of(o0 + i), &rec[i])) mask |= 1u << i;
    uint32_t tile_sites;
    const uint32_t rank = block_scan_excl((uint32_t)__popc(mask), sw, &tile_sites);
    if (EMIT) {
        if (tile_sites != counts[blockIdx.x]) return;   // (cannot be: both passes read the same adjacency; never write beyond what was counted)
        bgr_bubble* o = out + offs[blockIdx.x] + rank;
        uint32_t slot = 0;
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i)
            if ((mask >> i) & 1u) o[slot++] = rec[i];
    } else if (threadIdx.x == 0) {
        counts[blockIdx.x] = tile_sites;
    }
}

namespace bgr {

hipError_t launch_bubbles_count(const unsigned long long* pairs, uint64_t n_pairs, uint64_t n_unitigs, uint64_t min_link, void* scratch, hipStream_t stream, hipEvent_t* after) {
    if (n_unitigs == 0) return hipSuccess;
    const uint64_t tiles = bubbles_tiles(n_unitigs), blocks1 = (n_pairs + 255) / 256;
    if (!scratch || (n_pairs && !pairs) || min_link == 0 || n_unitigs >= 0x40000000ull || blocks1 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const BubblesScratch s(scratch, n_unitigs);
    auto mark = [&](int i) -> hipError_t { return after ? hipEventRecord(after[i], stream) : hipSuccess; };
    hipError_t e = hipMemsetAsync(s.deg, 0, tiles * kBubblesTile * 4, stream);
    if (e != hipSuccess) return e;
    if (n_pairs)
        hipLaunchKernelGGL(bgr_bubbles_adjacency_kernel, dim3((uint32_t)blocks1), dim3(256), 0, stream, reinterpret_cast<const ulonglong2*>(pairs), (u64)n_pairs, (u64)n_unitigs, (u64)min_link, s.deg,
                           s.to, s.cnt);
    if ((e = mark(0)) != hipSuccess) return e;
    hipLaunchKernelGGL(bgr_bubbles_classify_kernel<false>, dim3((uint32_t)tiles), dim3(kThreads), 0, stream, (u64)n_unitigs, (const uint32_t*)s.deg, (const int32_t*)s.to,
                       (const uint64_t*)s.cnt, s.counts, (const uint64_t*)s.offs, (bgr_bubble*)nullptr);
    if ((e = mark(1)) != hipSuccess) return e;
    if ((e = launch_variants_scan(s.counts, tiles, s.offs, stream)) != hipSuccess) return e;
    if ((e = mark(2)) != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t launch_bubbles_emit(uint64_t n_unitigs, const void* scratch, bgr_bubble* out, hipStream_t stream) {
    if (n_unitigs == 0) return hipSuccess;
    if (!scratch || !out || n_unitigs >= 0x40000000ull) return hipErrorInvalidValue;
    const BubblesScratch s(const_cast<void*>(scratch), n_unitigs);
    hipLaunchKernelGGL(bgr_bubbles_classify_kernel<true>, dim3((uint32_t)bubbles_tiles(n_unitigs)), dim3(kThreads), 0, stream, (u64)n_unitigs, (const uint32_t*)s.deg, (const int32_t*)s.to,
                       (const uint64_t*)s.cnt, s.counts, (const uint64_t*)s.offs, out);
    return hipGetLastError();
}

}  // namespace bgr
