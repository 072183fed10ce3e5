// blocks_kernels.hip -- phased bubble pairs chained into haplotype blocks (bgr_block_entry, include/bgreat_gpu.h): an index of the nodes by source,
// one thread per phase record for the links, pointer jumping towards the heads with the parity carried along, rings opened and ranked again, then
// count / scan / place over tiles of nodes (blocks_kernels.h has the passes).  Every pass is a gather: a round of the jumping reads one 16-byte
// state per node and one more wherever its pointer leads, so the passes are bound by dependent loads, not by arithmetic.
#include <hip/hip_runtime.h>

#include "blocks_kernels.h"
#include "variants_kernels.h"

namespace {

typedef unsigned long long u64;
constexpr uint32_t kTile = bgr::kBlocksTile, kThreads = bgr::kBlocksThreads, kPer = kTile / kThreads, kNone = bgr::kBlocksNone;
constexpr uint32_t kDone = 2u;   // bit 1 of a state's parity word: the node has met its head
static_assert(kPer == 4 && kThreads == 256, "a thread owns four consecutive nodes; four waves per workgroup");

// exclusive scan of v over the workgroup's 256 threads; *total = the sum.  sw: four LDS words of this call's own.  Every thread calls it.
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

__device__ __forceinline__ bool id_in(int32_t x, u64 n_unitigs) { const u64 a = bgr::bubbles_abs(x); return a != 0 && a <= n_unitigs; }

}  // namespace

// pass 1: one thread per node
__global__ void __launch_bounds__(256) bgr_blocks_index_kernel(const bgr_bubble* bubbles, uint32_t n_nodes, u64 n_unitigs, uint32_t* nos, uint32_t* err) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes) return;
    const int32_t s = bgr::blocks_source(bubbles[x >> 1], (uint32_t)x & 1u);
    if (!id_in(s, n_unitigs)) { atomicOr(err, (uint32_t)bgr::kBlocksErrId); return; }   // (nothing is ever written beyond the 2 n oriented ids)
    if (atomicCAS(nos + bgr::bubbles_o(s), kNone, (uint32_t)x) != kNone) atomicOr(err, (uint32_t)bgr::kBlocksErrSource);
}

// pass 2: one thread per phase record
__global__ void __launch_bounds__(256) bgr_blocks_link_kernel(const bgr_bubble* bubbles, uint32_t n_nodes, const bgr_phase* phase, u64 n_phase, u64 n_unitigs, u64 min_phase,
                                                              const uint32_t* nos, uint32_t* next, uint32_t* prev, uint32_t* err) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_phase) return;
    const bgr_phase p = phase[i];
    uint32_t par;
    if (!bgr::blocks_decided(p.count, min_phase, &par)) return;
    if (!id_in(p.source, n_unitigs) || !id_in(p.via, n_unitigs)) { atomicOr(err, (uint32_t)bgr::kBlocksErrId); return; }
    const uint32_t X = nos[bgr::bubbles_o(p.source)], Y = nos[bgr::bubbles_o(p.via)];
    if (X >= n_nodes || Y >= n_nodes) { atomicOr(err, (uint32_t)bgr::kBlocksErrMissing); return; }   // ("none" is beyond every node)
    const bgr_bubble bx = bubbles[X >> 1], by = bubbles[Y >> 1];
    const uint32_t rx = X & 1u, ry = Y & 1u;
    if (bgr::blocks_sink(bx, rx) != p.via || bgr::blocks_branch(bx, rx, 0) != p.in[0] || bgr::blocks_branch(bx, rx, 1) != p.in[1] || bgr::blocks_sink(by, ry) != p.sink ||
        bgr::blocks_branch(by, ry, 0) != p.out[0] || bgr::blocks_branch(by, ry, 1) != p.out[1] || (X >> 1) == (Y >> 1)) {
        atomicOr(err, (uint32_t)bgr::kBlocksErrDiffers);
        return;
    }
    const uint32_t bit = par << 31;   // (a node index is below 2^31: blocks_check)
    if (atomicCAS(next + X, kNone, Y) != kNone || atomicCAS(prev + Y, kNone, X | bit) != kNone || atomicCAS(next + (Y ^ 1u), kNone, X ^ 1u) != kNone ||
        atomicCAS(prev + (X ^ 1u), kNone, (Y ^ 1u) | bit) != kNone)
        atomicOr(err, (uint32_t)bgr::kBlocksErrTaken);
}

// pass 3, the start: a state is {x: pointer, y: links jumped, z: xor of their parities | kDone, w: smallest node of the span}
__global__ void __launch_bounds__(256) bgr_blocks_rank_init_kernel(uint32_t n_nodes, const uint32_t* prev, uint4* s) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes) return;
    const uint32_t w = prev[x];
    s[x] = w == kNone ? make_uint4((uint32_t)x, 0u, kDone, (uint32_t)x) : make_uint4(w & 0x7FFFFFFFu, 1u, w >> 31, (uint32_t)x);
}

// pass 3, a round: src is read, dst is written
__global__ void __launch_bounds__(256) bgr_blocks_rank_round_kernel(uint32_t n_nodes, const uint4* src, uint4* dst) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes) return;
    uint4 s = src[x];
    if (!(s.z & kDone) && s.x < n_nodes) {   // (a pointer is a node: next and prev hold nothing else)
        const uint4 q = src[s.x];
        s = make_uint4(q.x, s.y + q.y, ((s.z ^ q.z) & 1u) | (q.z & kDone), s.w < q.w ? s.w : q.w);
    }
    dst[x] = s;
}

// pass 4: a thread touches its own node's words only
__global__ void __launch_bounds__(256) bgr_blocks_open_kernel(uint32_t n_nodes, const uint4* s, uint32_t* next, uint32_t* prev, uint32_t* ring) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes) return;
    const uint4 st = s[x];
    uint32_t word = 0;
    if (!(st.z & kDone)) {   // on a ring, whose first node is st.w
        word = 1u;
        if (st.w == (uint32_t)x) { word |= (prev[x] >> 31) << 1; prev[x] = kNone; }   // (the removed link's parity stays with the node it entered)
        if (next[x] == st.w) next[x] = kNone;
    }
    ring[x] = word;
}

// pass 5: a chain has one tail, so a head's word has one writer.  meta = {x: size, y: tail, z: the ring's flags, w: 1 = written}
__global__ void __launch_bounds__(256) bgr_blocks_tail_kernel(uint32_t n_nodes, const uint4* s, const uint32_t* next, const uint32_t* ring, uint4* meta) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes || next[x] != kNone) return;
    const uint4 st = s[x];
    if (!(st.z & kDone) || st.x >= n_nodes) return;   // (cannot be: every ring has been opened)
    const uint32_t r = ring[st.x];
    uint32_t flags = 0;
    if (r & 1u) flags = BGR_BLOCK_CIRCULAR | (((r >> 1) & 1u) != (st.z & 1u) ? BGR_BLOCK_CONFLICT : 0u);
    meta[st.x] = make_uint4(st.y + 1u, (uint32_t)x, flags, 1u);
}

// passes 6 and 8
template <bool EMIT>
__global__ void __launch_bounds__(256) bgr_blocks_heads_kernel(uint32_t n_nodes, const uint32_t* prev, const uint4* meta, uint32_t* counts_s, uint32_t* counts_b, const uint64_t* offs_s,
                                                               const uint64_t* offs_b, uint32_t* hoff, uint32_t* hblk) {
    __shared__ uint32_t sw_s[kThreads / 64], sw_b[kThreads / 64];
    const u64 x0 = (u64)blockIdx.x * kTile + threadIdx.x * kPer;
    uint32_t size[kPer], sum = 0, heads = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        size[i] = 0;
        const u64 x = x0 + i;
        if (x < n_nodes && prev[x] == kNone) {
            const uint4 m = meta[x];
            const bool reported = m.w == 1u && (m.z & BGR_BLOCK_CIRCULAR ? !(x & 1u) : x < (u64)(m.y ^ 1u));
            if (reported) { size[i] = m.x; sum += m.x; ++heads; }   // (a size is at least 1)
        }
    }
    uint32_t tile_sum, tile_heads;
    const uint32_t rank_s = block_scan_excl(sum, sw_s, &tile_sum), rank_b = block_scan_excl(heads, sw_b, &tile_heads);
    if (EMIT) {
        if (tile_sum != counts_s[blockIdx.x] || tile_heads != counts_b[blockIdx.x]) return;   // (cannot be: both passes read the same words)
        uint32_t off = (uint32_t)offs_s[blockIdx.x] + rank_s, blk = (uint32_t)offs_b[blockIdx.x] + rank_b + 1u;
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {   // (hoff and hblk hold whole tiles)
            hoff[x0 + i] = size[i] ? off : kNone;
            hblk[x0 + i] = size[i] ? blk : 0u;
            if (size[i]) { off += size[i]; ++blk; }
        }
    } else if (threadIdx.x == 0) {
        counts_s[blockIdx.x] = tile_sum;
        counts_b[blockIdx.x] = tile_heads;
    }
}

// pass 8, the entries: one thread per node
__global__ void __launch_bounds__(256) bgr_blocks_write_kernel(uint32_t n_nodes, const uint4* s, const uint4* meta, const uint32_t* hoff, const uint32_t* hblk, bgr_block_entry* out,
                                                               uint32_t* err) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes) return;
    const uint4 st = s[x];
    if (!(st.z & kDone) || st.x >= n_nodes) return;
    const uint32_t off = hoff[st.x];
    if (off == kNone) return;   // (the mate reading is the one reported)
    const uint4 m = meta[st.x];
    const u64 at = (u64)off + st.y;
    if (at >= n_nodes / 2 || st.y >= m.x) { atomicOr(err, (uint32_t)bgr::kBlocksErrPlace); return; }   // (never write beyond the n entries)
    bgr_block_entry e;
    e.block = hblk[st.x]; e.index = st.y; e.size = m.x; e.bubble = (uint32_t)(x >> 1);
    e.flags = ((uint32_t)x & 1u ? BGR_BLOCK_REVERSED : 0u) | (st.z & 1u ? BGR_BLOCK_HAP : 0u) | m.z;
    e.reserved = 0;
    out[at] = e;
}

namespace bgr {

namespace {
bool blocks_args_ok(uint64_t n_bubbles, uint64_t n_unitigs, const void* scratch) { return scratch && n_bubbles && n_bubbles < 0x40000000ull && n_unitigs < 0x40000000ull; }
uint32_t grid_of(uint64_t n) { return (uint32_t)((n + 255) / 256); }
}  // namespace

hipError_t launch_blocks_link(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_phase* phase, uint64_t n_phase, uint64_t n_unitigs, uint64_t min_phase, void* scratch,
                              hipStream_t stream) {
    if (!blocks_args_ok(n_bubbles, n_unitigs, scratch) || !bubbles || (n_phase && !phase) || min_phase == 0 || (n_phase + 255) / 256 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const BlocksScratch s(scratch, n_bubbles, n_unitigs);
    const uint32_t N = (uint32_t)(2 * n_bubbles);
    hipError_t e = hipMemsetAsync(s.nos, 0xFF, s.none_bytes, stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.meta, 0, (uint64_t)N * 16, stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.err, 0, 16, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bgr_blocks_index_kernel, dim3(grid_of(N)), dim3(256), 0, stream, bubbles, N, (u64)n_unitigs, s.nos, s.err);
    if (n_phase)
        hipLaunchKernelGGL(bgr_blocks_link_kernel, dim3(grid_of(n_phase)), dim3(256), 0, stream, bubbles, N, phase, (u64)n_phase, (u64)n_unitigs, (u64)min_phase, (const uint32_t*)s.nos, s.next,
                           s.prev, s.err);
    return hipGetLastError();
}

// the states of all nodes, ranked from prev as it stands: -> the buffer that holds them
static uint4* rank_all(const BlocksScratch& s, uint32_t N, uint32_t rounds, hipStream_t stream) {
    uint4 *src = s.sa, *dst = s.sb;
    hipLaunchKernelGGL(bgr_blocks_rank_init_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, (const uint32_t*)s.prev, src);
    for (uint32_t r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(bgr_blocks_rank_round_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, (const uint4*)src, dst);
        uint4* t = src; src = dst; dst = t;
    }
    return src;
}
static const uint4* ranked(const BlocksScratch& s, uint64_t n_bubbles) { return blocks_rounds(n_bubbles) & 1u ? s.sb : s.sa; }

hipError_t launch_blocks_rank(uint64_t n_bubbles, uint64_t n_unitigs, void* scratch, hipStream_t stream) {
    if (!blocks_args_ok(n_bubbles, n_unitigs, scratch)) return hipErrorInvalidValue;
    const BlocksScratch s(scratch, n_bubbles, n_unitigs);
    const uint32_t N = (uint32_t)(2 * n_bubbles), rounds = blocks_rounds(n_bubbles);
    const uint4* first = rank_all(s, N, rounds, stream);
    hipLaunchKernelGGL(bgr_blocks_open_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, first, s.next, s.prev, s.ring);
    (void)rank_all(s, N, rounds, stream);   // (ends in the buffer `ranked` names)
    return hipGetLastError();
}

hipError_t launch_blocks_count(uint64_t n_bubbles, uint64_t n_unitigs, void* scratch, hipStream_t stream) {
    if (!blocks_args_ok(n_bubbles, n_unitigs, scratch)) return hipErrorInvalidValue;
    const BlocksScratch s(scratch, n_bubbles, n_unitigs);
    const uint32_t N = (uint32_t)(2 * n_bubbles);
    const uint64_t tiles = blocks_tiles(n_bubbles);
    hipLaunchKernelGGL(bgr_blocks_tail_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, ranked(s, n_bubbles), (const uint32_t*)s.next, (const uint32_t*)s.ring, s.meta);
    hipLaunchKernelGGL(bgr_blocks_heads_kernel<false>, dim3((uint32_t)tiles), dim3(kBlocksThreads), 0, stream, N, (const uint32_t*)s.prev, (const uint4*)s.meta, s.counts_s, s.counts_b,
                       (const uint64_t*)s.offs_s, (const uint64_t*)s.offs_b, s.hoff, s.hblk);
    hipError_t e = launch_variants_scan(s.counts_s, tiles, s.offs_s, stream);
    if (e == hipSuccess) e = launch_variants_scan(s.counts_b, tiles, s.offs_b, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_blocks_place(uint64_t n_bubbles, uint64_t n_unitigs, void* scratch, bgr_block_entry* out, hipStream_t stream) {
    if (!blocks_args_ok(n_bubbles, n_unitigs, scratch) || !out) return hipErrorInvalidValue;
    const BlocksScratch s(scratch, n_bubbles, n_unitigs);
    const uint32_t N = (uint32_t)(2 * n_bubbles);
    hipLaunchKernelGGL(bgr_blocks_heads_kernel<true>, dim3((uint32_t)blocks_tiles(n_bubbles)), dim3(kBlocksThreads), 0, stream, N, (const uint32_t*)s.prev, (const uint4*)s.meta, s.counts_s,
                       s.counts_b, (const uint64_t*)s.offs_s, (const uint64_t*)s.offs_b, s.hoff, s.hblk);
    hipLaunchKernelGGL(bgr_blocks_write_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, ranked(s, n_bubbles), (const uint4*)s.meta, (const uint32_t*)s.hoff, (const uint32_t*)s.hblk, out,
                       s.err);
    return hipGetLastError();
}

}  // namespace bgr
