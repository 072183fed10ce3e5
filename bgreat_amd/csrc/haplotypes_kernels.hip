// haplotypes_kernels.hip -- the sequences of the haplotype blocks spelled from the graph's 2-bit store (bgr_haplotype, include/bgreat_gpu.h): one
// thread per (entry, hap) for the pieces, lengths and junctions, a 64-bit scan over tiles of items, the spelling assigned by output in aligned
// 16-byte stores, the records (haplotypes_kernels.h has the passes).  The spell pass is a gather of 2-bit codes that ends in a streaming write: one
// output byte per two input bits, so the stores and the dependent loads in front of them decide its rate, not the bytes read.
#include <hip/hip_runtime.h>

#include "haplotypes_kernels.h"

namespace {

typedef unsigned long long u64;
constexpr uint32_t kTile = bgr::kHapTile, kThreads = bgr::kHapThreads, kPer = kTile / kThreads;
static_assert(kPer == 4 && kThreads == 256, "a thread owns four consecutive items; four waves per workgroup");
static_assert(bgr::kHapSpellTile == kThreads * 16 * 4, "a thread writes four 16-byte stores of its workgroup's tile");

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

struct Ori { u64 base; uint32_t len; uint32_t err; };   // an oriented unitig in seq; err: the error word's bits

__device__ __forceinline__ Ori oriented(const BgrUnitigMeta* meta, int32_t id, u64 n_unitigs, u64 total_bases) {
    Ori o = {0, 0, 0};
    const u64 a = bgr::bubbles_abs(id);
    if (a == 0 || a > n_unitigs) { o.err = bgr::kHapErrId; return o; }   // (nothing beyond meta's n_unitigs + 1 entries is read)
    const u64 F = meta[a].F;
    const uint32_t len = meta[a].len;
    if (F > total_bases || 2 * (u64)len > total_bases - F) { o.err = bgr::kHapErrSeq; return o; }   // (both strands lie inside the store)
    o.base = F + (id < 0 ? len : 0u);
    o.len = len;
    return o;
}

// the n <= 32 bases at base offset o of seq, right aligned (first base most significant); the word behind the last base's exists: seq ends in two pad words
__device__ __forceinline__ u64 window(const uint64_t* seq, u64 o, uint32_t n) {
    const u64 w0 = seq[o >> 5], w1 = seq[(o >> 5) + 1];
    const uint32_t sh = 2u * ((uint32_t)o & 31u);
    const u64 v = sh ? (w0 << sh) | (w1 >> (64u - sh)) : w0;
    return v >> (64u - 2u * n);
}

// -> 1 when the last k1 bases of p differ from the first k1 of c (1 <= k1 <= 63: one or two windows), or either is shorter than that
__device__ __forceinline__ uint32_t junction_bad(const uint64_t* seq, const Ori& p, const Ori& c, uint32_t k1) {
    if (p.len < k1 || c.len < k1) return 1u;
    const u64 a = p.base + p.len - k1, b = c.base;
    const uint32_t n0 = k1 < 32u ? k1 : 32u;
    if (window(seq, a, n0) != window(seq, b, n0)) return 1u;
    if (k1 > 32u && window(seq, a + 32, k1 - 32u) != window(seq, b + 32, k1 - 32u)) return 1u;
    return 0u;
}

}  // namespace

// pass 1: one thread per (entry, hap)
__global__ void __launch_bounds__(256) bgr_hap_items_kernel(const BgrUnitigMeta* meta, const uint64_t* seq, uint32_t k1, u64 n_unitigs, u64 total_bases, const bgr_bubble* bubbles, u64 n_bubbles,
                                                            const bgr_block_entry* entries, u64 n_entries, u64 min_block, uint64_t* pbase, uint32_t* plen, uint64_t* ilen, uint32_t* head,
                                                            uint64_t* words) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * n_entries) return;
    const u64 e = t >> 1;
    const uint32_t which = (uint32_t)t & 1u;
    const bgr_block_entry en = entries[e];
    uint32_t* err = reinterpret_cast<uint32_t*>(words + 1);
    if (en.index >= en.size || en.index > e || e - en.index + en.size > n_entries || en.bubble >= n_bubbles) { atomicOr(err, (uint32_t)bgr::kHapErrEntry); return; }
    const u64 p = 2 * (e - en.index) + (u64)which * en.size + en.index;   // (below 2 n_entries: the block lies inside the list)
    const bgr_bubble b = bubbles[en.bubble];
    const Ori src = oriented(meta, bgr::hap_src(en, b), n_unitigs, total_bases), br = oriented(meta, bgr::hap_branch(en, b, which), n_unitigs, total_bases),
              snk = oriented(meta, bgr::hap_snk(en, b), n_unitigs, total_bases);
    const bool kept = en.size >= min_block;
    uint32_t l0 = 0, l1 = 0, l2 = 0;
    if (const uint32_t bits = src.err | br.err | snk.err) atomicOr(err, bits);   // (the item stays empty)
    else if (kept) {
        l0 = en.index == 0 ? src.len : 0u;
        l1 = br.len > k1 ? br.len - k1 : 0u;
        l2 = snk.len > k1 ? snk.len - k1 : 0u;
        const uint32_t bad = junction_bad(seq, src, br, k1) + junction_bad(seq, br, snk, k1);
        if (bad) atomicAdd(reinterpret_cast<u64*>(words), (u64)bad);
    }
    pbase[3 * p] = src.base; pbase[3 * p + 1] = br.base + k1; pbase[3 * p + 2] = snk.base + k1;
    plen[3 * p] = l0; plen[3 * p + 1] = l1; plen[3 * p + 2] = l2;
    ilen[p] = (u64)l0 + l1 + l2;
    head[p] = kept && en.index == 0 && which == 0 ? 1u : 0u;
}

// pass 2, the tiles' sums and (EMIT) the items' offsets and ordinals
template <bool EMIT>
__global__ void __launch_bounds__(256) bgr_hap_tiles_kernel(u64 n_items, const uint64_t* ilen, const uint32_t* head, uint64_t* tsum, const uint64_t* toff, u64 n_tiles, uint64_t* ioff,
                                                            uint64_t* iord) {
    __shared__ u64 sw_l[kThreads / 64], sw_h[kThreads / 64];
    const u64 x0 = (u64)blockIdx.x * kTile + threadIdx.x * kPer;
    u64 len[kPer], hd[kPer], sum = 0, heads = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        const bool in = x0 + i < n_items;
        len[i] = in ? ilen[x0 + i] : 0;
        hd[i] = in ? head[x0 + i] : 0;
        sum += len[i];
        heads += hd[i];
    }
    u64 tile_sum, tile_heads;
    const u64 rank_l = block_scan_excl64(sum, sw_l, &tile_sum), rank_h = block_scan_excl64(heads, sw_h, &tile_heads);
    if (EMIT) {
        u64 off = toff[blockIdx.x] + rank_l, ord = toff[n_tiles + 1 + blockIdx.x] + rank_h;
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            if (x0 + i < n_items) { ioff[x0 + i] = off; iord[x0 + i] = ord; }
            off += len[i];
            ord += hd[i];
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) { ioff[n_items] = toff[n_tiles]; iord[n_items] = toff[2 * n_tiles + 1]; }
    } else if (threadIdx.x == 0) {
        tsum[blockIdx.x] = tile_sum;
        tsum[n_tiles + blockIdx.x] = tile_heads;
    }
}

// pass 2, over the tiles: one workgroup; toff[0 .. T] = exclusive sums of the lengths and their total, toff[T + 1 .. 2 T + 1] likewise of the heads
__global__ void __launch_bounds__(256) bgr_hap_tile_scan_kernel(const uint64_t* tsum, u64 n_tiles, uint64_t* toff) {
    __shared__ u64 sw[kThreads / 64];
    for (uint32_t part = 0; part < 2; ++part) {
        const uint64_t* in = tsum + part * n_tiles;
        uint64_t* out = toff + part * (n_tiles + 1);
        u64 carry = 0;
        for (u64 base = 0; base < n_tiles; base += kThreads) {
            const u64 i = base + threadIdx.x;
            const u64 v = i < n_tiles ? in[i] : 0;
            u64 all;
            const u64 ex = block_scan_excl64(v, sw, &all);
            if (i < n_tiles) out[i] = carry + ex;
            carry += all;
            __syncthreads();   // (sw is written again)
        }
        if (threadIdx.x == 0) out[n_tiles] = carry;
    }
}

// pass 3: a workgroup spells kHapSpellTile output bytes
__global__ void __launch_bounds__(256) bgr_hap_spell_kernel(const uint64_t* seq, u64 n_items, u64 total, const uint64_t* ioff, const uint64_t* pbase, const uint32_t* plen, char* out) {
    __shared__ u64 s_item[2];
    const u64 tile0 = (u64)blockIdx.x * bgr::kHapSpellTile;
    if (threadIdx.x < 2) {   // the items that hold the tile's first and last byte: the last i with ioff[i] <= pos (an empty item before it shares its offset)
        const u64 last = tile0 + bgr::kHapSpellTile - 1 < total - 1 ? tile0 + bgr::kHapSpellTile - 1 : total - 1;
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
        uint32_t piece = 0;
        uint32_t left = plen[3 * item];   // characters of the current piece from its beginning
        u64 base = pbase[3 * item];
        const uint32_t n = total - pos < 16 ? (uint32_t)(total - pos) : 16u;
        uint32_t word[4] = {0, 0, 0, 0};
        bool ok = true;
        while (local >= left) {   // (an item's first piece is empty unless it heads its block)
            local -= left;
            if (++piece == 3) { piece = 0; ++item; }
            if (item >= n_items) { ok = false; break; }
            left = plen[3 * item + piece];
            base = pbase[3 * item + piece];
        }
        if (ok && n == 16 && left - local >= 16) {   // all 16 inside one piece, as nearly all are: 32 bits of the store, four codes to four characters by one byte permute
            const u64 b = base + local, w0 = seq[b >> 5], w1 = seq[(b >> 5) + 1];
            const uint32_t sh = 2u * ((uint32_t)b & 31u);
            const uint32_t v = (uint32_t)((sh ? (w0 << sh) | (w1 >> (64u - sh)) : w0) >> 32);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t x = (v >> (24u - 8u * j)) & 0xFFu;   // bases 4 j .. 4 j + 3, the first in bits 7..6
                const uint32_t sel = ((x << 24) | (x << 14) | (x << 4) | (x >> 6)) & 0x03030303u;   // byte i = the code of base 4 j + i
                word[j] = __builtin_amdgcn_perm(0x54474341u, 0x54474341u, sel);   // "ACGT" (a selector below 4 picks from the second operand; both hold the table)
            }
            *reinterpret_cast<uint4*>(out + pos) = make_uint4(word[0], word[1], word[2], word[3]);
            continue;
        }
        u64 cw = ~0ull, w = 0;
        for (uint32_t c = 0; ok && c < n; ++c) {
            while (local >= left) {   // over the piece's border (empty pieces and empty items too)
                local -= left;
                if (++piece == 3) { piece = 0; ++item; }
                if (item >= n_items) { ok = false; break; }   // (cannot be: pos lies below the total)
                left = plen[3 * item + piece];
                base = pbase[3 * item + piece];
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

// pass 4: one thread per entry; the head of a kept block writes its two records
__global__ void __launch_bounds__(256) bgr_hap_records_kernel(const bgr_block_entry* entries, u64 n_entries, u64 min_block, const uint64_t* ioff, const uint64_t* iord, bgr_haplotype* out,
                                                              u64 n_records, uint64_t* words) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    const bgr_block_entry en = entries[e];
    if (en.index != 0 || en.size < min_block) return;
    const u64 p = 2 * e, at = 2 * iord[p];
    if (e + en.size > n_entries || at + 1 >= n_records) { atomicOr(reinterpret_cast<uint32_t*>(words + 1), (uint32_t)bgr::kHapErrPlace); return; }   // (never write beyond the records)
    const u64 o0 = ioff[p], o1 = ioff[p + en.size], o2 = ioff[p + 2 * (u64)en.size];
    bgr_haplotype h;
    h.block = en.block; h.hap = 0; h.size = en.size; h.flags = bgr::hap_ring(en); h.offset = o0; h.length = o1 - o0;
    out[at] = h;
    h.hap = 1; h.offset = o1; h.length = o2 - o1;
    out[at + 1] = h;
}

namespace bgr {

namespace {
bool hap_args_ok(uint64_t n_entries, const void* scratch) { return scratch && n_entries && n_entries < 0x40000000ull; }
uint32_t grid_of(uint64_t n) { return (uint32_t)((n + 255) / 256); }
}  // namespace

hipError_t launch_hap_items(const BgrDeviceGraph& dg, uint64_t n_unitigs, uint64_t total_bases, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries,
                            uint64_t n_entries, uint64_t min_block, void* scratch, hipStream_t stream) {
    if (!hap_args_ok(n_entries, scratch) || !bubbles || !entries || !dg.meta || !dg.seq || dg.k < 2 || dg.k > BGR_MAX_K || min_block == 0) return hipErrorInvalidValue;
    const HapScratch s(scratch, n_entries);
    const u64 I = 2 * n_entries, T = hap_tiles(n_entries);
    hipError_t e = hipMemsetAsync(s.words, 0, 16, stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.ilen, 0, I * 8, stream);   // (an item that pass 1 refuses writes nothing: the scan still sums words that were written)
    if (e == hipSuccess) e = hipMemsetAsync(s.head, 0, I * 4, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bgr_hap_items_kernel, dim3(grid_of(I)), dim3(256), 0, stream, dg.meta, dg.seq, dg.k - 1, (u64)n_unitigs, (u64)total_bases, bubbles, (u64)n_bubbles, entries, (u64)n_entries,
                       (u64)min_block, s.pbase, s.plen, s.ilen, s.head, s.words);
    hipLaunchKernelGGL(bgr_hap_tiles_kernel<false>, dim3((uint32_t)T), dim3(kHapThreads), 0, stream, I, (const uint64_t*)s.ilen, (const uint32_t*)s.head, s.tsum, (const uint64_t*)s.toff, T, s.ioff,
                       s.iord);
    hipLaunchKernelGGL(bgr_hap_tile_scan_kernel, dim3(1), dim3(kHapThreads), 0, stream, (const uint64_t*)s.tsum, T, s.toff);
    hipLaunchKernelGGL(bgr_hap_tiles_kernel<true>, dim3((uint32_t)T), dim3(kHapThreads), 0, stream, I, (const uint64_t*)s.ilen, (const uint32_t*)s.head, s.tsum, (const uint64_t*)s.toff, T, s.ioff,
                       s.iord);
    return hipGetLastError();
}

hipError_t launch_hap_spell(const BgrDeviceGraph& dg, uint64_t n_entries, uint64_t total, void* scratch, char* out, hipStream_t stream) {
    if (!hap_args_ok(n_entries, scratch) || !dg.seq || !out || (reinterpret_cast<uintptr_t>(out) & 15u) || total == 0) return hipErrorInvalidValue;
    const uint64_t tiles = (total + kHapSpellTile - 1) / kHapSpellTile;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const HapScratch s(scratch, n_entries);
    hipLaunchKernelGGL(bgr_hap_spell_kernel, dim3((uint32_t)tiles), dim3(kHapThreads), 0, stream, dg.seq, (u64)(2 * n_entries), (u64)total, (const uint64_t*)s.ioff, (const uint64_t*)s.pbase,
                       (const uint32_t*)s.plen, out);
    return hipGetLastError();
}

hipError_t launch_hap_records(const bgr_block_entry* entries, uint64_t n_entries, uint64_t min_block, void* scratch, bgr_haplotype* out, uint64_t n_records, hipStream_t stream) {
    if (!hap_args_ok(n_entries, scratch) || !entries || !out || n_records == 0 || min_block == 0) return hipErrorInvalidValue;
    const HapScratch s(scratch, n_entries);
    hipLaunchKernelGGL(bgr_hap_records_kernel, dim3(grid_of(n_entries)), dim3(256), 0, stream, entries, (u64)n_entries, (u64)min_block, (const uint64_t*)s.ioff, (const uint64_t*)s.iord, out,
                       (u64)n_records, s.words);
    return hipGetLastError();
}

}  // namespace bgr
