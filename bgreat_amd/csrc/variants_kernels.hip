// variants_kernels.hip -- SNV sites on the unitigs from one pileup table in HBM (bgr_variant_site, include/bgreat_gpu.h): a device-wide
// reduce / scan / classify / compact in five launches (variants_kernels.h has the passes and why the scan runs flat over all unitigs), and the
// kernel that adds one pileup table into another.  All of it is bound by the bytes it reads: the loads are dwordx4 where the tile is whole, a
// thread owns eight consecutive delta words (one 32-byte stretch, a wave 2 KiB), the scans inside a workgroup run on __shfl_up within a wave
// and through four LDS words between the waves.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "variants_kernels.h"

using bgr::u64;

namespace {

constexpr uint32_t kTile = bgr::kVariantsTile, kThreads = bgr::kVariantsThreads, kPer = kTile / kThreads;
static_assert(kPer == 8 && kThreads == 256, "a thread owns two uint4 of delta words; four waves per workgroup");
// starts of the unitigs that lie in a tile, kept in LDS: a unitig owns len + 1 >= 2 words, so at most kTile / 2 begin inside a tile; with the one
// the tile begins in, the first one behind the tile and the rounding to whole turns of the workgroup that is below kStarts
constexpr uint32_t kStarts = kTile / 2 + kThreads;

// exclusive scan of v over the workgroup's 256 threads (mod 2^32); *total = the sum.  sw: four LDS words.  Every thread calls it.
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* sw, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= (uint32_t)off) incl += t;
    }
    __syncthreads();   // (the words may still be read from the call before)
    if (lane == 63u) sw[wave] = incl;
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < kThreads / 64; ++i) { const uint32_t s = sw[i]; all += s; if (i < wave) pre += s; }
    *total = all;
    return pre + incl - v;
}

// the tile's eight words of this thread: delta[w .. w + 8), zero beyond the table's end
__device__ __forceinline__ void load8(const uint32_t* delta, u64 w, u64 words, uint32_t d[kPer]) {
    if (w + kPer <= words) {
        const uint4 a = *reinterpret_cast<const uint4*>(delta + w), b = *reinterpret_cast<const uint4*>(delta + w + 4);
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) d[i] = w + i < words ? delta[w + i] : 0u;
    }
}

}  // namespace

// pass 1: sums[t] = the tile's delta words added up
__device__ __forceinline__ void tile_sums_body(const uint32_t* delta, u64 words, uint32_t* sums) {
    __shared__ uint32_t sw[kThreads / 64];
    const u64 w0 = (u64)blockIdx.x * kTile;
    uint32_t s = 0;
#pragma unroll
    for (uint32_t it = 0; it < kPer / 4; ++it) {   // (lane i at 16 i bytes of a 4 KiB stretch)
        const u64 w = w0 + (u64)it * (kThreads * 4) + threadIdx.x * 4u;
        if (w + 4 <= words) { const uint4 a = *reinterpret_cast<const uint4*>(delta + w); s += a.x + a.y + a.z + a.w; }
        else for (uint32_t i = 0; i < 4; ++i) if (w + i < words) s += delta[w + i];
    }
    uint32_t total;
    (void)block_scan_excl(s, sw, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ void __launch_bounds__(256) bgr_variants_tile_sums_kernel(const uint32_t* delta, u64 words, uint32_t* sums) { tile_sums_body(delta, words, sums); }
// with strands: the total table's words (blockIdx.y == 0) and the forward table's (1) in one launch
__global__ void __launch_bounds__(256) bgr_variants_tile_sums2_kernel(const uint32_t* delta, const uint32_t* delta_f, u64 words, uint32_t* sums, uint32_t* sums_f) {
    if (blockIdx.y == 0) tile_sums_body(delta, words, sums); else tile_sums_body(delta_f, words, sums_f);
}

// passes 2 and 4: out[t] = in[0] + .. + in[t - 1] for t = 0 .. n (64-bit; its low word is the sum mod 2^32).  One workgroup; a thread takes
// sixteen consecutive values of a turn (the arrays are a few bytes per tile: nothing here is bound by bandwidth).
__device__ __forceinline__ void scan_body(const uint32_t* in, u64 n, u64* out) {
    __shared__ u64 sw64[kThreads / 64];
    constexpr uint32_t kEach = 16;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 run = 0;
    for (u64 base = 0; base < n; base += (u64)kThreads * kEach) {
        const u64 i0 = base + (u64)threadIdx.x * kEach;
        u64 mine = 0;
        for (uint32_t i = 0; i < kEach; ++i) if (i0 + i < n) mine += in[i0 + i];
        u64 incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u64 t = __shfl_up((unsigned long long)incl, (unsigned)off, 64);
            if (lane >= (uint32_t)off) incl += t;
        }
        __syncthreads();
        if (lane == 63u) sw64[wave] = incl;
        __syncthreads();
        u64 pre = 0, all = 0;
#pragma unroll
        for (uint32_t i = 0; i < kThreads / 64; ++i) { const u64 s = sw64[i]; all += s; if (i < wave) pre += s; }
        u64 at = run + pre + incl - mine;
        for (uint32_t i = 0; i < kEach; ++i) if (i0 + i < n) { out[i0 + i] = at; at += in[i0 + i]; }
        run += all;
    }
    if (threadIdx.x == 0) out[n] = run;
}
__global__ void __launch_bounds__(256) bgr_variants_scan_kernel(const uint32_t* in, u64 n, u64* out) { scan_body(in, n, out); }
// with strands, pass 2: two workgroups, one per table's tile sums (neither waits for the other)
__global__ void __launch_bounds__(256) bgr_variants_scan2_kernel(const uint32_t* in, const uint32_t* in_f, u64 n, u64* out, u64* out_f) {
    if (blockIdx.x == 0) scan_body(in, n, out); else scan_body(in_f, n, out_f);
}

// passes 3 and 5.  STRANDS: the forward table (alt_f, delta_f, carry_f) is scanned along; a base with a candidate allele also reads its four forward
// alt words, an allele must pass variants_strand_passing as well, and a record is a 64-byte bgr_variant_strand_site (out_s).  A compile-time
// constant: the instances without it are the kernel as it was.
template <bool EMIT, bool STRANDS>
__global__ void __launch_bounds__(256) bgr_variants_classify_kernel(BgrDeviceGraph g, u64 n_unitigs, u64 total_bases, const uint32_t* alt, const uint32_t* delta,
                                                                   const u64* base_offs, bgr_variant_params prm, const u64* carry, uint32_t* counts, const u64* offs,
                                                                   bgr_variant_site* out, const uint32_t* alt_f, const uint32_t* delta_f, const u64* carry_f,
                                                                   uint32_t min_alt_strand, bgr_variant_strand_site* out_s) {
    __shared__ uint32_t sw[kThreads / 64];
    __shared__ u64 s_start[kStarts], s_F[kStarts];
    __shared__ u64 s_id0;
    const u64 words = total_bases + n_unitigs, w0 = (u64)blockIdx.x * kTile, w_end = w0 + kTile;
    // unitig id begins at word base_offs[id] + id - 1; id n + 1 "begins" at the table's end
    auto start_of = [&](u64 id) -> u64 { return id <= n_unitigs + 1 ? base_offs[id] + id - 1 : ~0ull; };
    if (threadIdx.x == 0) {   // the unitig word w0 lies in: the last id whose start is <= w0
        u64 lo = 1, hi = n_unitigs;
        while (lo < hi) { const u64 mid = (lo + hi + 1) >> 1; if (start_of(mid) <= w0) lo = mid; else hi = mid - 1; }
        s_id0 = lo;
    }
    __syncthreads();
    const u64 id0 = s_id0;
    uint32_t filled = 0;   // entries of the two LDS arrays that are written
    for (uint32_t base = 0; base < kStarts; base += kThreads) {   // the starts of id0, id0 + 1, .. up to the first one behind the tile
        const u64 id = id0 + base + threadIdx.x, st = start_of(id);
        s_start[base + threadIdx.x] = st;
        s_F[base + threadIdx.x] = id <= n_unitigs ? g.meta[id].F : 0;
        filled = base + kThreads;
        if (__syncthreads_or(st >= w_end)) break;
    }
    auto start_at = [&](u64 j) -> u64 { return j < filled ? s_start[j] : start_of(id0 + j); };   // (beyond the LDS copy only if unitigs of no base exist)
    auto F_at = [&](u64 j) -> u64 { return j < filled ? s_F[j] : (id0 + j <= n_unitigs ? g.meta[id0 + j].F : 0); };

    const u64 wf = w0 + threadIdx.x * kPer;
    uint32_t d[kPer];
    load8(delta, wf, words, d);
#pragma unroll
    for (uint32_t i = 1; i < kPer; ++i) d[i] += d[i - 1];
    uint32_t tile_sum;
    const uint32_t before = (uint32_t)carry[blockIdx.x] + block_scan_excl(d[kPer - 1], sw, &tile_sum);   // the running sum in front of this thread's words
    uint32_t df[kPer], before_f = 0;   // the same of the forward table
    if (STRANDS) {
        load8(delta_f, wf, words, df);
#pragma unroll
        for (uint32_t i = 1; i < kPer; ++i) df[i] += df[i - 1];
        before_f = (uint32_t)carry_f[blockIdx.x] + block_scan_excl(df[kPer - 1], sw, &tile_sum);
    }

    // this thread's first word: the last j with start_at(j) <= wf, among the starts in LDS (they ascend; those of ids beyond n + 1 are ~0)
    u64 j = 0;
    if (wf < words) {
        u64 lo = 0, hi = filled - 1;
        while (lo < hi) { const u64 mid = (lo + hi + 1) >> 1; if (s_start[mid] <= wf) lo = mid; else hi = mid - 1; }
        j = lo;
    }
    u64 cur = start_at(j), next = start_at(j + 1), F = F_at(j);
    // what the emit pass keeps of a site until its rank is known, in registers (the loops are unrolled: every index is a constant)
    uint32_t site_mask = 0, refs = 0, s_id[kPer], s_pos[kPer];
    uint4 s_alt[kPer], s_falt[kPer];
    u64 seq_word = 0, seq_at = ~0ull;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        const u64 w = wf + i;
        if (w < words) {
            while (w >= next) { ++j; cur = next; next = start_at(j + 1); F = F_at(j); }
            const u64 pos = w - cur, len = next - cur - 1, id = id0 + j, b = w - (id - 1), p = F + pos;
            const uint32_t depth = before + d[i];
            if (pos != len && depth >= prm.min_depth && b < total_bases) {   // not the unitig's extra word, and a base an allele can pass at
                const uint4 a4 = *reinterpret_cast<const uint4*>(alt + 4 * b);
                if ((p >> 5) != seq_at) { seq_at = p >> 5; seq_word = g.seq[seq_at]; }
                const uint32_t ref = (uint32_t)(seq_word >> (62 - 2 * (p & 31))) & 3u;
                const uint32_t c[4] = {a4.x, a4.y, a4.z, a4.w};
                uint32_t m = bgr::variants_passing(depth, c, ref, prm.min_depth, prm.min_alt, prm.min_af_ppm);
                if (STRANDS && m) {
                    const uint4 f4 = *reinterpret_cast<const uint4*>(alt_f + 4 * b);
                    const uint32_t cf[4] = {f4.x, f4.y, f4.z, f4.w};
                    m = bgr::variants_strand_passing(m, c, cf, min_alt_strand);
                    if (EMIT) s_falt[i] = f4;
                }
                if (m) {
                    site_mask |= 1u << i;
                    if (EMIT) { refs |= ref << (2 * i); s_id[i] = (uint32_t)id; s_pos[i] = (uint32_t)pos; s_alt[i] = a4; }
                }
            }
        }
    }
    uint32_t tile_sites;
    const uint32_t rank = block_scan_excl((uint32_t)__popc(site_mask), sw, &tile_sites);
    if (EMIT) {
        if (tile_sites != counts[blockIdx.x]) return;   // (cannot be: both passes read the same table; never write beyond what was counted)
        uint4* o = STRANDS ? reinterpret_cast<uint4*>(out_s + offs[blockIdx.x] + rank) : reinterpret_cast<uint4*>(out + offs[blockIdx.x] + rank);
        uint32_t slot = 0;
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i)
            if ((site_mask >> i) & 1u) {
                const uint32_t ref = (refs >> (2 * i)) & 3u;
                const uint4 a4 = s_alt[i];
                const uint32_t nn = ref == 0 ? a4.x : ref == 1 ? a4.y : ref == 2 ? a4.z : a4.w;
                if (STRANDS) {
                    const uint4 f4 = s_falt[i];
                    const uint32_t fn = ref == 0 ? f4.x : ref == 1 ? f4.y : ref == 2 ? f4.z : f4.w;
                    o[4 * slot] = make_uint4(s_id[i], s_pos[i], before + d[i], ref == 0 ? 0u : a4.x);
                    o[4 * slot + 1] = make_uint4(ref == 1 ? 0u : a4.y, ref == 2 ? 0u : a4.z, ref == 3 ? 0u : a4.w, nn);
                    o[4 * slot + 2] = make_uint4(before_f + df[i], ref == 0 ? 0u : f4.x, ref == 1 ? 0u : f4.y, ref == 2 ? 0u : f4.z);
                    o[4 * slot + 3] = make_uint4(ref == 3 ? 0u : f4.w, fn, 0u, 0u);
                } else {
                    o[2 * slot] = make_uint4(s_id[i], s_pos[i], before + d[i], ref == 0 ? 0u : a4.x);
                    o[2 * slot + 1] = make_uint4(ref == 1 ? 0u : a4.y, ref == 2 ? 0u : a4.z, ref == 3 ? 0u : a4.w, nn);
                }
                ++slot;
            }
    } else if (threadIdx.x == 0) {
        counts[blockIdx.x] = tile_sites;
    }
}

// dst[i] += src[i]
__global__ void __launch_bounds__(256) bgr_pileup_add_kernel(uint32_t* dst, const uint32_t* src, u64 n_words, u64 n_u32, uint32_t tail_u64) {
    const u64 stride = (u64)gridDim.x * blockDim.x, quads = n_u32 / 4;
    for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
        uint4 a = reinterpret_cast<uint4*>(dst)[q];
        const uint4 b = reinterpret_cast<const uint4*>(src)[q];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        reinterpret_cast<uint4*>(dst)[q] = a;
    }
    if (blockIdx.x == 0) {
        for (u64 i = 4 * quads + threadIdx.x; i < n_u32; i += blockDim.x) dst[i] += src[i];
        if (tail_u64 && threadIdx.x == 0) {   // (n_words - 2 is even: a table's tail is 8-byte aligned)
            u64* dt = reinterpret_cast<u64*>(dst + n_words - 2);
            *dt += *reinterpret_cast<const u64*>(src + n_words - 2);
        }
    }
}

namespace bgr {

namespace {
struct Scratch {   // (carry_f, sums_f: the forward table's carries and tile sums, there only with strands)
    u64* carry; u64* offs; uint32_t* sums; uint32_t* counts; u64* carry_f; uint32_t* sums_f;
    Scratch(void* p, uint64_t tiles) {
        carry = static_cast<u64*>(p); offs = carry + tiles + 1;
        sums = reinterpret_cast<uint32_t*>(offs + tiles + 1); counts = sums + tiles;
        carry_f = reinterpret_cast<u64*>(static_cast<char*>(p) + variants_scratch_bytes(tiles, false));
        sums_f = reinterpret_cast<uint32_t*>(carry_f + tiles + 1);
    }
};
// what both launchers refuse
bool variants_args_ok(uint64_t n_unitigs, uint64_t tiles, const uint32_t* table, const uint64_t* base_offs, const bgr_variant_strand_params& sp, const void* scratch) {
    return table && base_offs && scratch && n_unitigs < 0x40000000ull && tiles <= 0x7FFFFFFFull && variants_params_ok(bgr_variant_params{sp.min_depth, sp.min_alt, sp.min_af_ppm});
}
// the classify kernel's instances, [strands][emit]
const decltype(&bgr_variants_classify_kernel<false, false>) kClassify[2][2] = {{bgr_variants_classify_kernel<false, false>, bgr_variants_classify_kernel<true, false>},
                                                                               {bgr_variants_classify_kernel<false, true>, bgr_variants_classify_kernel<true, true>}};
}  // namespace

hipError_t launch_variants_count(const BgrDeviceGraph& g, uint64_t n_unitigs, uint64_t total_bases, const uint32_t* table, const uint32_t* table_fwd,
                                 const uint64_t* base_offs, const bgr_variant_strand_params& sp, void* scratch, hipStream_t stream, hipEvent_t* after) {
    const uint64_t tiles = variants_tiles(total_bases, n_unitigs);
    if (n_unitigs == 0 || tiles == 0) return hipSuccess;
    if (!variants_args_ok(n_unitigs, tiles, table, base_offs, sp, scratch)) return hipErrorInvalidValue;
    const bgr_variant_params prm = {sp.min_depth, sp.min_alt, sp.min_af_ppm};
    const Scratch s(scratch, tiles);
    const uint32_t* alt = table;
    const uint32_t* delta = table + pileup_alt_words(total_bases);
    const uint32_t* delta_f = table_fwd ? table_fwd + pileup_alt_words(total_bases) : nullptr;
    const u64 words = pileup_delta_words(total_bases, n_unitigs);
    auto mark = [&](int i) -> hipError_t { return after ? hipEventRecord(after[i], stream) : hipSuccess; };
    hipError_t e;
    if (table_fwd) hipLaunchKernelGGL(bgr_variants_tile_sums2_kernel, dim3((uint32_t)tiles, 2), dim3(kThreads), 0, stream, delta, delta_f, words, s.sums, s.sums_f);
    else hipLaunchKernelGGL(bgr_variants_tile_sums_kernel, dim3((uint32_t)tiles), dim3(kThreads), 0, stream, delta, words, s.sums);
    if ((e = mark(0)) != hipSuccess) return e;
    if (table_fwd) hipLaunchKernelGGL(bgr_variants_scan2_kernel, dim3(2), dim3(kThreads), 0, stream, (const uint32_t*)s.sums, (const uint32_t*)s.sums_f, (u64)tiles, s.carry, s.carry_f);
    else hipLaunchKernelGGL(bgr_variants_scan_kernel, dim3(1), dim3(kThreads), 0, stream, (const uint32_t*)s.sums, (u64)tiles, s.carry);
    if ((e = mark(1)) != hipSuccess) return e;
    hipLaunchKernelGGL(kClassify[table_fwd != nullptr][0], dim3((uint32_t)tiles), dim3(kThreads), 0, stream, g, (u64)n_unitigs, (u64)total_bases, alt, delta,
                       reinterpret_cast<const u64*>(base_offs), prm, (const u64*)s.carry, s.counts, (const u64*)s.offs, (bgr_variant_site*)nullptr, table_fwd, delta_f,
                       table_fwd ? (const u64*)s.carry_f : nullptr, table_fwd ? sp.min_alt_strand : 0u, (bgr_variant_strand_site*)nullptr);
    if ((e = mark(2)) != hipSuccess) return e;
    hipLaunchKernelGGL(bgr_variants_scan_kernel, dim3(1), dim3(kThreads), 0, stream, (const uint32_t*)s.counts, (u64)tiles, s.offs);
    if ((e = mark(3)) != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t launch_variants_emit(const BgrDeviceGraph& g, uint64_t n_unitigs, uint64_t total_bases, const uint32_t* table, const uint32_t* table_fwd,
                                const uint64_t* base_offs, const bgr_variant_strand_params& sp, const void* scratch, void* out, hipStream_t stream) {
    const uint64_t tiles = variants_tiles(total_bases, n_unitigs);
    if (n_unitigs == 0 || tiles == 0) return hipSuccess;
    if (!variants_args_ok(n_unitigs, tiles, table, base_offs, sp, scratch) || !out) return hipErrorInvalidValue;
    const bgr_variant_params prm = {sp.min_depth, sp.min_alt, sp.min_af_ppm};
    const Scratch s(const_cast<void*>(scratch), tiles);
    hipLaunchKernelGGL(kClassify[table_fwd != nullptr][1], dim3((uint32_t)tiles), dim3(kThreads), 0, stream, g, (u64)n_unitigs, (u64)total_bases, table,
                       table + pileup_alt_words(total_bases), reinterpret_cast<const u64*>(base_offs), prm, (const u64*)s.carry, s.counts, (const u64*)s.offs,
                       table_fwd ? nullptr : static_cast<bgr_variant_site*>(out), table_fwd, table_fwd ? table_fwd + pileup_alt_words(total_bases) : nullptr,
                       table_fwd ? (const u64*)s.carry_f : nullptr, table_fwd ? sp.min_alt_strand : 0u, table_fwd ? static_cast<bgr_variant_strand_site*>(out) : nullptr);
    return hipGetLastError();
}

hipError_t launch_variants_scan(const uint32_t* in, uint64_t n, uint64_t* out, hipStream_t stream) {
    if (!in || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bgr_variants_scan_kernel, dim3(1), dim3(kThreads), 0, stream, in, (u64)n, out);
    return hipGetLastError();
}

hipError_t launch_pileup_add(uint32_t* dst, const uint32_t* src, uint64_t n_words, bool tail_u64, uint32_t num_cus, hipStream_t stream) {
    if (n_words == 0) return hipSuccess;
    if (!dst || !src || (tail_u64 && (n_words < 2 || (n_words & 1)))) return hipErrorInvalidValue;
    if (!num_cus) num_cus = 256;
    const uint64_t n_u32 = tail_u64 ? n_words - 2 : n_words;
    uint64_t blocks = (n_u32 / 4 + 255) / 256;
    if (blocks > (uint64_t)num_cus * 8) blocks = (uint64_t)num_cus * 8;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(bgr_pileup_add_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, dst, src, (u64)n_words, (u64)n_u32, tail_u64 ? 1u : 0u);
    return hipGetLastError();
}

}  // namespace bgr
