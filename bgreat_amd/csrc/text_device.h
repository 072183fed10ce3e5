// text_device.h -- the device helpers that more than one unit of the text route needs (text_kernels.hip: the streaming kernels; text_correct.hip:
// correction mode; text_gaf.hip: GAF lines and path stats): the wave and workgroup scans, 16 bytes of text as words and masks, decimal numbers,
// copies by the 16 lanes of a group, and WalkIter, the serial walk of a path that -c spells and a GAF line of a long path walks again.
// Included behind device_common.h by .hip files only.
#ifndef BGREAT_AMD_TEXT_DEVICE_H
#define BGREAT_AMD_TEXT_DEVICE_H

#include "device_common.h"

namespace bgr {
namespace {

// inclusive scan over the 64 lanes of a wave without LDS: four row_shr steps scan each row of 16, row_bcast:15 carries row 0 into row 1 and row 2 into row 3,
// row_bcast:31 carries rows 0..1 into rows 2..3 (a lane whose source lies outside its row, or whose row is masked out, adds the 0 given as `old`)
#define BGR_DPP0(x, ctrl, rows) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(x), ctrl, rows, 0xF, false))
__device__ __forceinline__ uint32_t wave_inclusive_scan32(uint32_t x) {
    x += BGR_DPP0(x, 0x111, 0xF); x += BGR_DPP0(x, 0x112, 0xF); x += BGR_DPP0(x, 0x114, 0xF); x += BGR_DPP0(x, 0x118, 0xF);
    x += BGR_DPP0(x, 0x142, 0xA);
    x += BGR_DPP0(x, 0x143, 0xC);
    return x;
}
#define BGR_DPP0_64(x, ctrl, rows) (((u64)BGR_DPP0((uint32_t)((x) >> 32), ctrl, rows) << 32) | BGR_DPP0((uint32_t)(x), ctrl, rows))
__device__ __forceinline__ u64 wave_inclusive_scan64(u64 x) {
    x += BGR_DPP0_64(x, 0x111, 0xF); x += BGR_DPP0_64(x, 0x112, 0xF); x += BGR_DPP0_64(x, 0x114, 0xF); x += BGR_DPP0_64(x, 0x118, 0xF);
    x += BGR_DPP0_64(x, 0x142, 0xA);
    x += BGR_DPP0_64(x, 0x143, 0xC);
    return x;
}

__device__ __forceinline__ uint32_t block_exclusive_scan32(uint32_t v, uint32_t* lds_waves, uint32_t* block_total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;   // (up to 16 waves)
    const uint32_t inc = wave_inclusive_scan32(v);
    if (lane == 63) lds_waves[wave] = inc;
    __syncthreads();
    // every wave scans the (at most 16) wave totals itself: one LDS read, four shuffles (a loop over them waits for LDS sixteen times)
    const uint32_t t = lane < nw ? lds_waves[lane] : 0u;
    uint32_t ti = t;
    ti += BGR_DPP0(ti, 0x111, 0xF); ti += BGR_DPP0(ti, 0x112, 0xF); ti += BGR_DPP0(ti, 0x114, 0xF); ti += BGR_DPP0(ti, 0x118, 0xF);   // (row 0 holds them)
    const uint32_t before = (uint32_t)__shfl((int)(ti - t), wave, 64);
    *block_total = (uint32_t)__shfl((int)ti, 15, 64);
    __syncthreads();
    return before + inc - v;
}

// bit 7 of every byte of x that equals the byte replicated in `pat`
__device__ __forceinline__ uint32_t eq_bytes(uint32_t x, uint32_t pat) { return bgr_zero_bytes(x ^ pat); }

// 16 bytes from `p` (any alignment; bytes at or beyond `end` read as zero)
__device__ __forceinline__ void load16(const uint8_t* text, uint32_t p, uint32_t end, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (p >= end) return;
    const u32x4_unaligned v = *reinterpret_cast<const u32x4_unaligned*>(text + p);  // (the buffer is padded by 32 bytes)
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    const uint32_t valid = end - p;
    if (valid < 16) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t lo = 4u * d;
            if (valid <= lo) w[d] = 0;
            else if (valid < lo + 4) w[d] &= 0xFFFFFFFFu >> (8 * (lo + 4 - valid));
        }
    }
}
// bit i (0..15) = byte i of the 16 loaded equals c
__device__ __forceinline__ uint32_t mask16(const uint32_t w[4], uint32_t pat) {
    uint32_t m = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) m |= nibble_of(eq_bytes(w[d], pat)) << (4 * d);
    return m;
}

__device__ __forceinline__ u64 shfl64(u64 x, int l) { return ((u64)(uint32_t)__shfl((int)(uint32_t)(x >> 32), l, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)x, l, 64); }
// exclusive scans of N 64-bit values per thread over the workgroup, array after array (value n of thread t comes behind value n - 1 of every thread): one pair
// of barriers for all of them.  ex[n] = what lies in front of v[n]; *total = everything.  (fields packed in a value must not carry into each other)
template <int N>
__device__ __forceinline__ void block_exclusive_scan64xN(const u64 (&v)[N], u64* lds_waves /* N * 16 */, u64 (&ex)[N], u64* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    u64 inc[N];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        inc[n] = wave_inclusive_scan64(v[n]);
        if (lane == 63) lds_waves[n * 16 + wave] = inc[n];
    }
    __syncthreads();
    u64 run = 0;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const u64 t = lane < nw ? lds_waves[n * 16 + lane] : 0ull;
        u64 ti = t;
        ti += BGR_DPP0_64(ti, 0x111, 0xF); ti += BGR_DPP0_64(ti, 0x112, 0xF); ti += BGR_DPP0_64(ti, 0x114, 0xF); ti += BGR_DPP0_64(ti, 0x118, 0xF);
        ex[n] = run + shfl64(ti - t, wave) + inc[n] - v[n];
        run += shfl64(ti, 15);
    }
    *total = run;
    __syncthreads();
}

constexpr uint32_t kNone = 0xFFFFFFFFu;   // "no such position" of the searches in a text

__device__ __forceinline__ uint32_t dec_len(int32_t v) {  // characters of to_string(v) + '.'
    uint32_t u = (uint32_t)v, len = 1;
    if (v < 0) { u = 0u - u; len = 2; }
    len += u < 10 ? 1 : u < 100 ? 2 : u < 1000 ? 3 : u < 10000 ? 4 : u < 100000 ? 5 : u < 1000000 ? 6 : u < 10000000 ? 7 : u < 100000000 ? 8 : u < 1000000000 ? 9 : 10;
    return len;
}
// the first min(m, 16) bytes of v to dst (any alignment)
__device__ __forceinline__ void store_upto16(uint8_t* dst, const u32x4_unaligned v, uint32_t m) {
    if (m >= 16) { *reinterpret_cast<u32x4_unaligned*>(dst) = v; return; }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};   // (the last bytes: byte stores out of registers -- a loop of byte loads and stores waits for memory once per byte)
#pragma unroll
    for (uint32_t i = 0; i < 15; ++i) if (i < m) dst[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}
// n bytes from src to dst by the 16 lanes of a group (any alignment on both sides; the SOURCE may be read up to 15 bytes past its end: the text is padded)
__device__ __forceinline__ void group_copy(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t sub) {
    for (uint32_t b = 16 * sub; b < n; b += 256) {
        store_upto16(dst + b, *reinterpret_cast<const u32x4_unaligned*>(src + b), n - b);
    }
}

// the walk recoverPath spells (text_correct.hip has the reference's lines), unitig by unitig; WIDE: k > 33, see there
template <bool WIDE>
struct WalkIter {   // the oriented unitigs of a path, one after the other
    const BgrDeviceGraph& g;
    const int32_t* path;
    uint32_t np, K1;
    uint32_t i = 1;          // path int of the current unitig
    u64 base = 0;            // where its oriented bases start in seq
    uint32_t len = 0, skip = 0;  // its length; bases of it that belong to the overlap with its predecessor (0 for the first, else k-1)
    bool bad = false;
    __device__ WalkIter(const BgrDeviceGraph& g_, const int32_t* p, uint32_t n) : g(g_), path(p), np(n), K1(g_.k - 1) {}
    __device__ u64 kmer_at(u64 b) const { return win32(g.seq, b) >> (64 - 2 * (WIDE ? 32 : K1)); }
    __device__ bool kmer_eq(u64 b, u64 t, u64 t2) const { return kmer_at(b) == t && (!WIDE || win32(g.seq, b + 32) >> (128 - 2 * K1) == t2); }
    __device__ bool load() {  // unitig i as its sign orients it; false when the id is out of range (getUnitig of a bad int)
        const int32_t s = path[i];
        const uint32_t id = (uint32_t)(s < 0 ? -(int64_t)s : (int64_t)s);
        if (id == 0 || id > (uint32_t)g.hdr->n_unitigs) return false;
        const BgrUnitigMeta m = g.meta[id];
        len = m.len;
        base = m.F + (s < 0 ? m.len : 0);
        return true;
    }
    __device__ bool first() { skip = 0; i = 1; if (np < 2 || !load()) { bad = true; return false; } return true; }
    __device__ bool next() {   // false: no further unitig (or bad set: bug compaction)
        if (i + 1 >= np) return false;
        const u64 tail = kmer_at(base + len - K1), tail2 = WIDE ? win32(g.seq, base + len - K1 + 32) >> (128 - 2 * K1) : 0;
        ++i;
        if (!load()) { bad = true; return false; }
        if (!kmer_eq(base, tail, tail2)) {  // compactionEnd's second try: the reverse complement (the other strand of the store)
            const int32_t s = path[i];
            const uint32_t id = (uint32_t)(s < 0 ? -(int64_t)s : (int64_t)s);
            const BgrUnitigMeta m = g.meta[id];
            const u64 other = m.F + (s < 0 ? 0 : m.len);
            if (!kmer_eq(other, tail, tail2)) { bad = true; return false; }
            base = other;
        }
        skip = K1;
        return true;
    }
};

__device__ __forceinline__ uint8_t base_char(uint32_t code) { return (uint8_t)((0x54474341u >> (8 * code)) & 0xFF); }  // "ACGT"

__device__ __forceinline__ uint32_t dec_digits(u64 u) {   // characters of to_string(u)
    uint32_t n = 1;
    for (u64 p = 10; n < 20 && u >= p; p *= 10) ++n;
    return n;
}
// to_string(u) ending in front of e
__device__ __forceinline__ void put_dec(uint8_t* e, u64 u) {
    if (u <= 0xFFFFFFFFull) { uint32_t v = (uint32_t)u; do { const uint32_t q = v / 10; *--e = (uint8_t)('0' + (v - q * 10)); v = q; } while (v); }
    else do { const u64 q = u / 10; *--e = (uint8_t)('0' + (uint32_t)(u - q * 10)); u = q; } while (u);
}

}  // namespace
}  // namespace bgr

#undef BGR_DPP0_64
#undef BGR_DPP0

#endif
