// recompact_kernels.hip -- a kept subset of the graph's unitigs compacted into maximal non-branching chains (bgr_chain, include/bgreat_gpu.h): the
// ends counted in a table indexed by meta's key indices, unique successors, pointer jumping towards the heads with rings cut and ranked again,
// count / scan / place over the node index, the chains' characters spelled by output in aligned 16-byte stores, the records
// (recompact_kernels.h has the passes).  Passes 1 - 4 are gathers of a few words per node, bound by dependent loads; the spell pass is a gather of
// 2-bit codes that ends in a streaming write.
#include <hip/hip_runtime.h>

#include "recompact_kernels.h"

namespace {

typedef unsigned long long u64;
constexpr uint32_t kTile = bgr::kRecompactTile, kThreads = bgr::kRecompactThreads, kPer = kTile / kThreads, kNone = bgr::kRecompactNone;
constexpr uint32_t kDone = 1u;   // a state's z word: the node has met its head
static_assert(kPer == 4 && kThreads == 256, "a thread owns four consecutive items; four waves per workgroup");
static_assert(bgr::kRecompactSpellTile == kThreads * 16 * 4, "a thread writes four 16-byte stores of its workgroup's tile");

__device__ __forceinline__ u64 shfl_up64(u64 v, int off) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), off, 64);
    return ((u64)hi << 32) | lo;
}

// exclusive scan of v over the workgroup's 256 threads; *total = the sum.  sw: four LDS words of this call's own.  Every thread calls it.
__device__ __forceinline__ u64 block_scan_excl64(u64 v, u64* sw, u64* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 t = shfl_up64(incl, off);
        if (lane >= (uint32_t)off) incl += t;
    }
    if (lane == 63u) sw[wave] = incl;
    __syncthreads();
    u64 pre = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < kThreads / 64; ++i) { const u64 s = sw[i]; all += s; if (i < wave) pre += s; }
    *total = all;
    return pre + incl - v;
}

// the table entry of node o's begin key (end = false) or end key (end = true): 2 * key index + orientation bit, kNone when the key index lies
// beyond the table.  The bit is 0 where the (k-1)-mer is its own canonical form: a palindrome has the flag set in both readings
__device__ __forceinline__ uint32_t end_key(const BgrUnitigMeta* meta, uint32_t o, bool end, u64 n_keys) {
    const BgrUnitigMeta m = meta[(o >> 1) + 1];
    const bool neg = o & 1u;
    const uint32_t rec = (end != neg) ? m.rec_end : m.rec_beg;
    const uint32_t flag = end ? (neg ? BGR_META_CANON_RCBEG : BGR_META_CANON_END) : (neg ? BGR_META_CANON_RCEND : BGR_META_CANON_BEG);
    if (rec >= n_keys) return kNone;
    return 2u * rec + (m.flags & flag ? 0u : 1u);
}

__device__ __forceinline__ int32_t id_of(uint32_t o) { const int32_t u = (int32_t)(o >> 1) + 1; return o & 1u ? -u : u; }

}  // namespace

// pass 1: one thread per node
__global__ void __launch_bounds__(256) bgr_recompact_ends_kernel(const BgrUnitigMeta* meta, uint32_t n_nodes, u64 n_keys, const uint8_t* keep, uint2* tab, uint32_t* err) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes || !keep[x >> 1]) return;
    const uint32_t key = end_key(meta, (uint32_t)x, false, n_keys);
    if (key == kNone) { atomicOr(err, (uint32_t)bgr::kRecompactErrKey); return; }   // (nothing is written beyond the 2 n_keys entries)
    atomicAdd(&tab[key].x, 1u);
    tab[key].y = (uint32_t)id_of((uint32_t)x);   // (read only where the count ends at 1: then this was the one writer)
}

// pass 2: one thread per node
__global__ void __launch_bounds__(256) bgr_recompact_succ_kernel(const BgrUnitigMeta* meta, uint32_t n_nodes, u64 n_keys, const uint8_t* keep, const uint2* tab, uint32_t* succ,
                                                                 uint32_t* err) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes || !keep[x >> 1]) return;
    const uint32_t key = end_key(meta, (uint32_t)x, true, n_keys);
    if (key == kNone) { atomicOr(err, (uint32_t)bgr::kRecompactErrKey); return; }
    const uint2 e = tab[key];
    if (e.x != 1u) return;
    const int32_t y = (int32_t)e.y;
    const uint32_t a = y < 0 ? (uint32_t)(-(int64_t)y) : (uint32_t)y;
    if (a == 0 || 2ull * a > n_nodes) { atomicOr(err, (uint32_t)bgr::kRecompactErrId); return; }   // (meta has n + 1 entries)
    const uint32_t oy = 2u * (a - 1u) + (y < 0 ? 1u : 0u);
    if (a == (uint32_t)(x >> 1) + 1u) return;   // a self-loop or a hairpin
    const uint32_t back = end_key(meta, oy ^ 1u, true, n_keys);   // out(-y) = in(y)
    if (back == kNone) { atomicOr(err, (uint32_t)bgr::kRecompactErrKey); return; }
    if (tab[back].x == 1u) succ[x] = oy;
}

// pass 3, the start: a state is {x: pointer, y: links jumped, z: kDone, w: smallest node of the span}
__global__ void __launch_bounds__(256) bgr_recompact_rank_init_kernel(uint32_t n_nodes, const uint32_t* succ, uint4* s) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes) return;
    const uint32_t w = succ[x ^ 1u];   // pred(x) = succ[mate] ^ 1
    s[x] = w == kNone ? make_uint4((uint32_t)x, 0u, kDone, (uint32_t)x) : make_uint4(w ^ 1u, 1u, 0u, (uint32_t)x);
}

// pass 3, a round: src is read, dst is written
__global__ void __launch_bounds__(256) bgr_recompact_rank_round_kernel(uint32_t n_nodes, const uint4* src, uint4* dst) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes) return;
    uint4 s = src[x];
    if (!(s.z & kDone) && s.x < n_nodes) {   // (a pointer is a node: succ holds nothing else)
        const uint4 q = src[s.x];
        s = make_uint4(q.x, s.y + q.y, q.z & kDone, s.w < q.w ? s.w : q.w);
    }
    dst[x] = s;
}

// pass 3, the rings: a thread touches its own node's words only
__global__ void __launch_bounds__(256) bgr_recompact_open_kernel(uint32_t n_nodes, const uint4* s, uint32_t* succ, uint32_t* ring) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes) return;
    const uint4 st = s[x];
    const bool on_ring = !(st.z & kDone);
    if (on_ring) {   // whose smallest node is st.w: forward in the reported reading (cut where it is entered), reversed in the mate (cut where it is left)
        if (!(st.w & 1u)) { if (succ[x] == st.w) succ[x] = kNone; }
        else if (st.w == (uint32_t)x) succ[x] = kNone;
    }
    ring[x] = on_ring ? 1u : 0u;
}

// pass 4: a chain has one tail, so a head's word has one writer.  meta = {x: size, y: tail}
__global__ void __launch_bounds__(256) bgr_recompact_tail_kernel(uint32_t n_nodes, const uint8_t* keep, const uint4* s, const uint32_t* succ, uint2* cmeta) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes || !keep[x >> 1] || succ[x] != kNone) return;
    const uint4 st = s[x];
    if (!(st.z & kDone) || st.x >= n_nodes) return;   // (cannot be: every ring has been opened)
    cmeta[st.x] = make_uint2(st.y + 1u, (uint32_t)x);
}

// pass 4: per node the size of the chain it heads in the reported reading and a 1, else two zeroes
__global__ void __launch_bounds__(256) bgr_recompact_heads_kernel(uint32_t n_nodes, const uint8_t* keep, const uint32_t* succ, const uint2* cmeta, uint32_t* hsize, uint32_t* hflag) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes) return;
    uint32_t size = 0;
    if (keep[x >> 1] && succ[x ^ 1u] == kNone) {
        const uint2 m = cmeta[x];
        if (m.x != 0u && (uint32_t)x < (m.y ^ 1u)) size = m.x;   // head < -tail (never equal: no chain is its own mate)
    }
    hsize[x] = size;
    hflag[x] = size ? 1u : 0u;
}

// the scan, per tile: the tiles' sums, or (EMIT) the items' exclusive offsets and, behind the last, the total
template <bool EMIT>
__global__ void __launch_bounds__(256) bgr_recompact_tiles_kernel(u64 n_items, const uint32_t* v, uint64_t* tsum, const uint64_t* toff, u64 n_tiles, uint64_t* off) {
    __shared__ u64 sw[kThreads / 64];
    const u64 x0 = (u64)blockIdx.x * kTile + threadIdx.x * kPer;
    u64 val[kPer], sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        val[i] = x0 + i < n_items ? v[x0 + i] : 0;
        sum += val[i];
    }
    u64 tile_sum;
    const u64 rank = block_scan_excl64(sum, sw, &tile_sum);
    if (EMIT) {
        u64 o = toff[blockIdx.x] + rank;
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            if (x0 + i < n_items) off[x0 + i] = o;
            o += val[i];
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) off[n_items] = toff[n_tiles];
    } else if (threadIdx.x == 0) tsum[blockIdx.x] = tile_sum;
}

// the scan, over the tiles: one workgroup; toff[0 .. T] = exclusive sums and the total
__global__ void __launch_bounds__(256) bgr_recompact_tile_scan_kernel(const uint64_t* tsum, u64 n_tiles, uint64_t* toff) {
    __shared__ u64 sw[kThreads / 64];
    u64 carry = 0;
    for (u64 base = 0; base < n_tiles; base += kThreads) {
        const u64 i = base + threadIdx.x;
        const u64 v = i < n_tiles ? tsum[i] : 0;
        u64 all;
        const u64 ex = block_scan_excl64(v, sw, &all);
        if (i < n_tiles) toff[i] = carry + ex;
        carry += all;
        __syncthreads();   // (sw is written again)
    }
    if (threadIdx.x == 0) toff[n_tiles] = carry;
}

// pass 4, the walk: one thread per node
__global__ void __launch_bounds__(256) bgr_recompact_place_kernel(const BgrUnitigMeta* meta, uint32_t k1, uint32_t n_nodes, u64 total_bases, const uint8_t* keep, const uint4* s,
                                                                  const uint2* cmeta, const uint32_t* hflag, const uint64_t* hoff, int32_t* walk, uint64_t* pbase, uint32_t* plen,
                                                                  uint32_t* err) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes || !keep[x >> 1]) return;
    const uint4 st = s[x];
    if (!(st.z & kDone) || st.x >= n_nodes) return;
    if (!hflag[st.x]) return;   // (the mate reading is the one reported)
    const u64 at = hoff[st.x] + st.y;
    if (at >= n_nodes / 2 || st.y >= cmeta[st.x].x) { atomicOr(err, (uint32_t)bgr::kRecompactErrPlace); return; }   // (never write beyond the n places)
    const BgrUnitigMeta m = meta[(x >> 1) + 1];
    if (m.F > total_bases || 2 * (u64)m.len > total_bases - m.F) { atomicOr(err, (uint32_t)bgr::kRecompactErrSeq); return; }   // (both strands lie inside the store)
    if (m.len <= k1) { atomicOr(err, (uint32_t)bgr::kRecompactErrLen); return; }   // (a unitig has at least k characters)
    const uint32_t skip = st.y ? k1 : 0u;
    walk[at] = id_of((uint32_t)x);
    pbase[at] = m.F + (x & 1u ? m.len : 0u) + skip;
    plen[at] = m.len - skip;
}

// pass 5: a workgroup spells kRecompactSpellTile output bytes from the flat list of pieces
__global__ void __launch_bounds__(256) bgr_recompact_spell_kernel(const uint64_t* seq, u64 n_items, u64 total, const uint64_t* ioff, const uint64_t* pbase, const uint32_t* plen, char* out) {
    __shared__ u64 s_item[2];
    const u64 tile0 = (u64)blockIdx.x * bgr::kRecompactSpellTile;
    if (threadIdx.x < 2) {   // the pieces that hold the tile's first and last byte: the last i with ioff[i] <= pos
        const u64 last = tile0 + bgr::kRecompactSpellTile - 1 < total - 1 ? tile0 + bgr::kRecompactSpellTile - 1 : total - 1;
        const u64 pos = threadIdx.x ? last : tile0;
        u64 lo = 0, hi = n_items - 1;
        while (lo < hi) {
            const u64 mid = (lo + hi + 1) >> 1;
            if (ioff[mid] <= pos) lo = mid; else hi = mid - 1;
        }
        s_item[threadIdx.x] = lo;
    }
    __syncthreads();
    const u64 first = s_item[0], last = s_item[1];
#pragma unroll 1
    for (uint32_t r = 0; r < 4; ++r) {
        const u64 pos = tile0 + ((u64)r * kThreads + threadIdx.x) * 16;
        if (pos >= total) return;
        u64 lo = first, hi = last;
        while (lo < hi) {
            const u64 mid = (lo + hi + 1) >> 1;
            if (ioff[mid] <= pos) lo = mid; else hi = mid - 1;
        }
        u64 item = lo, local = pos - ioff[lo];
        uint32_t left = plen[item];   // characters of the current piece from its beginning
        u64 base = pbase[item];
        const uint32_t n = total - pos < 16 ? (uint32_t)(total - pos) : 16u;
        uint32_t word[4] = {0, 0, 0, 0};
        if (local < left && n == 16 && left - local >= 16) {   // all 16 inside one piece, as nearly all are: 32 bits of the store, four codes to four characters by one byte permute
            // (the word behind the last base's is read whatever the shift: it exists, seq ends in two pad words -- graph_layout.h)
            const u64 b = base + local, w0 = seq[b >> 5], w1 = seq[(b >> 5) + 1];
            const uint32_t sh = 2u * ((uint32_t)b & 31u);
            const uint32_t v = (uint32_t)((sh ? (w0 << sh) | (w1 >> (64u - sh)) : w0) >> 32);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t c = (v >> (24u - 8u * j)) & 0xFFu;   // bases 4 j .. 4 j + 3, the first in bits 7..6
                const uint32_t sel = ((c << 24) | (c << 14) | (c << 4) | (c >> 6)) & 0x03030303u;   // byte i = the code of base 4 j + i
                word[j] = __builtin_amdgcn_perm(0x54474341u, 0x54474341u, sel);   // "ACGT"
            }
            *reinterpret_cast<uint4*>(out + pos) = make_uint4(word[0], word[1], word[2], word[3]);
            continue;
        }
        u64 cw = ~0ull, w = 0;
        bool ok = true;
        for (uint32_t c = 0; ok && c < n; ++c) {
            while (local >= left) {   // over the piece's border (a piece that was refused is empty)
                local -= left;
                if (++item >= n_items) { ok = false; break; }   // (cannot be: pos lies below the total)
                left = plen[item];
                base = pbase[item];
            }
            if (!ok) break;
            const u64 b = base + local;
            if ((b >> 5) != cw) { cw = b >> 5; w = seq[cw]; }
            const uint32_t code = (uint32_t)(w >> (62u - 2u * ((uint32_t)b & 31u))) & 3u;
            word[c >> 2] |= ((0x54474341u >> (8u * code)) & 0xFFu) << (8u * (c & 3u));   // "ACGT"
            ++local;
        }
        if (n == 16) *reinterpret_cast<uint4*>(out + pos) = make_uint4(word[0], word[1], word[2], word[3]);
        else for (uint32_t c = 0; c < n; ++c) out[pos + c] = (char)((word[c >> 2] >> (8u * (c & 3u))) & 0xFFu);   // (the last bytes of all: nothing beyond the total)
    }
}

// pass 6: one thread per node; an emitting head writes its record
__global__ void __launch_bounds__(256) bgr_recompact_records_kernel(uint32_t n_nodes, const uint2* cmeta, const uint32_t* hflag, const uint64_t* hoff, const uint64_t* hord,
                                                                    const uint64_t* ioff, const uint32_t* ring, bgr_chain* out, u64 n_records, uint32_t* err) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_nodes || !hflag[x]) return;
    const u64 at = hord[x], a = hoff[x], size = cmeta[x].x;
    if (at >= n_records || a + size > n_nodes / 2) { atomicOr(err, (uint32_t)bgr::kRecompactErrPlace); return; }   // (never write beyond the records, never read beyond ioff[n])
    bgr_chain c;
    c.seq_off = ioff[a]; c.seq_len = ioff[a + size] - ioff[a]; c.walk_off = a; c.n_unitigs = (uint32_t)size; c.flags = ring[x] ? BGR_CHAIN_CIRCULAR : 0u;
    out[at] = c;
}

namespace bgr {

namespace {
bool recompact_args_ok(uint64_t n_unitigs, const void* scratch) { return scratch && n_unitigs && n_unitigs < 0x40000000ull && !(reinterpret_cast<uintptr_t>(scratch) & 15u); }
uint32_t grid_of(uint64_t n) { return (uint32_t)((n + 255) / 256); }
uint32_t* err_of(const RecompactScratch& s) { return reinterpret_cast<uint32_t*>(s.words + 1); }

// off[0 .. n_items] = the exclusive sums of v and their total
void scan_items(const RecompactScratch& s, const uint32_t* v, uint64_t n_items, uint64_t* off, hipStream_t stream) {
    const u64 T = recompact_tiles(n_items);
    hipLaunchKernelGGL(bgr_recompact_tiles_kernel<false>, dim3((uint32_t)T), dim3(kRecompactThreads), 0, stream, (u64)n_items, v, s.tsum, (const uint64_t*)s.toff, T, off);
    hipLaunchKernelGGL(bgr_recompact_tile_scan_kernel, dim3(1), dim3(kRecompactThreads), 0, stream, (const uint64_t*)s.tsum, T, s.toff);
    hipLaunchKernelGGL(bgr_recompact_tiles_kernel<true>, dim3((uint32_t)T), dim3(kRecompactThreads), 0, stream, (u64)n_items, v, s.tsum, (const uint64_t*)s.toff, T, off);
}

// the states of all nodes, ranked from succ as it stands: -> the buffer that holds them
uint4* rank_all(const RecompactScratch& s, uint32_t N, uint32_t rounds, hipStream_t stream) {
    uint4 *src = s.sa, *dst = s.sb;
    hipLaunchKernelGGL(bgr_recompact_rank_init_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, (const uint32_t*)s.succ, src);
    for (uint32_t r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(bgr_recompact_rank_round_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, (const uint4*)src, dst);
        uint4* t = src; src = dst; dst = t;
    }
    return src;
}
const uint4* ranked(const RecompactScratch& s, uint64_t n_unitigs) { return recompact_rounds(n_unitigs) & 1u ? s.sb : s.sa; }
}  // namespace

hipError_t launch_recompact_links(const BgrDeviceGraph& dg, uint64_t n_unitigs, uint64_t n_keys, void* scratch, hipStream_t stream) {
    if (!recompact_args_ok(n_unitigs, scratch) || !dg.meta || n_keys >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    const RecompactScratch s(scratch, n_unitigs, n_keys);
    const uint32_t N = (uint32_t)(2 * n_unitigs);
    hipError_t e = hipMemsetAsync(s.words, 0, 16, stream);
    if (e == hipSuccess && n_keys) e = hipMemsetAsync(s.tab, 0, 2 * n_keys * sizeof(uint2), stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.succ, 0xFF, (uint64_t)N * 4, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bgr_recompact_ends_kernel, dim3(grid_of(N)), dim3(256), 0, stream, dg.meta, N, (u64)n_keys, (const uint8_t*)s.keep, s.tab, err_of(s));
    hipLaunchKernelGGL(bgr_recompact_succ_kernel, dim3(grid_of(N)), dim3(256), 0, stream, dg.meta, N, (u64)n_keys, (const uint8_t*)s.keep, (const uint2*)s.tab, s.succ, err_of(s));
    return hipGetLastError();
}

hipError_t launch_recompact_rank(uint64_t n_unitigs, uint64_t n_keys, void* scratch, hipStream_t stream) {
    if (!recompact_args_ok(n_unitigs, scratch)) return hipErrorInvalidValue;
    const RecompactScratch s(scratch, n_unitigs, n_keys);
    const uint32_t N = (uint32_t)(2 * n_unitigs), rounds = recompact_rounds(n_unitigs);
    const uint4* first = rank_all(s, N, rounds, stream);
    hipLaunchKernelGGL(bgr_recompact_open_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, first, s.succ, s.ring);
    (void)rank_all(s, N, rounds, stream);   // (ends in the buffer `ranked` names)
    return hipGetLastError();
}

hipError_t launch_recompact_place(const BgrDeviceGraph& dg, uint64_t n_unitigs, uint64_t n_keys, uint64_t total_bases, void* scratch, hipStream_t stream) {
    if (!recompact_args_ok(n_unitigs, scratch) || !dg.meta || dg.k < 2 || dg.k > BGR_MAX_K) return hipErrorInvalidValue;
    const RecompactScratch s(scratch, n_unitigs, n_keys);
    const uint32_t N = (uint32_t)(2 * n_unitigs);
    hipError_t e = hipMemsetAsync(s.meta, 0, (uint64_t)N * sizeof(uint2), stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.plen, 0, n_unitigs * 4, stream);   // (a place that no node takes, or whose node is refused, is an empty piece)
    if (e == hipSuccess) e = hipMemsetAsync(s.pbase, 0, n_unitigs * 8, stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.walk, 0, n_unitigs * 4, stream);
    if (e != hipSuccess) return e;
    const uint4* st = ranked(s, n_unitigs);
    hipLaunchKernelGGL(bgr_recompact_tail_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, (const uint8_t*)s.keep, st, (const uint32_t*)s.succ, s.meta);
    hipLaunchKernelGGL(bgr_recompact_heads_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, (const uint8_t*)s.keep, (const uint32_t*)s.succ, (const uint2*)s.meta, s.hsize, s.hflag);
    scan_items(s, s.hsize, N, s.hoff, stream);
    scan_items(s, s.hflag, N, s.hord, stream);
    hipLaunchKernelGGL(bgr_recompact_place_kernel, dim3(grid_of(N)), dim3(256), 0, stream, dg.meta, dg.k - 1, N, (u64)total_bases, (const uint8_t*)s.keep, st, (const uint2*)s.meta,
                       (const uint32_t*)s.hflag, (const uint64_t*)s.hoff, s.walk, s.pbase, s.plen, err_of(s));
    scan_items(s, s.plen, n_unitigs, s.ioff, stream);
    return hipGetLastError();
}

hipError_t launch_recompact_spell(const BgrDeviceGraph& dg, uint64_t n_unitigs, uint64_t n_keys, uint64_t walk_n, uint64_t total, void* scratch, char* out, hipStream_t stream) {
    if (!recompact_args_ok(n_unitigs, scratch) || !dg.seq || !out || (reinterpret_cast<uintptr_t>(out) & 15u) || total == 0 || walk_n == 0 || walk_n > n_unitigs) return hipErrorInvalidValue;
    const uint64_t tiles = (total + kRecompactSpellTile - 1) / kRecompactSpellTile;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const RecompactScratch s(scratch, n_unitigs, n_keys);
    hipLaunchKernelGGL(bgr_recompact_spell_kernel, dim3((uint32_t)tiles), dim3(kRecompactThreads), 0, stream, dg.seq, (u64)walk_n, (u64)total, (const uint64_t*)s.ioff, (const uint64_t*)s.pbase,
                       (const uint32_t*)s.plen, out);
    return hipGetLastError();
}

hipError_t launch_recompact_records(uint64_t n_unitigs, uint64_t n_keys, void* scratch, bgr_chain* out, uint64_t n_records, hipStream_t stream) {
    if (!recompact_args_ok(n_unitigs, scratch) || !out || n_records == 0) return hipErrorInvalidValue;
    const RecompactScratch s(scratch, n_unitigs, n_keys);
    const uint32_t N = (uint32_t)(2 * n_unitigs);
    hipLaunchKernelGGL(bgr_recompact_records_kernel, dim3(grid_of(N)), dim3(256), 0, stream, N, (const uint2*)s.meta, (const uint32_t*)s.hflag, (const uint64_t*)s.hoff, (const uint64_t*)s.hord,
                       (const uint64_t*)s.ioff, (const uint32_t*)s.ring, out, (u64)n_records, err_of(s));
    return hipGetLastError();
}

}  // namespace bgr
