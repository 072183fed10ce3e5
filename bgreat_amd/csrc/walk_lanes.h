// walk_lanes.h -- the walk of a mapped read's path by the sixteen lanes of a group, shared by the kernels that need to know where every unitig of
// a path lies in the walk and on which strand it was glued on: gaf_stat (text_gaf.hip: GAF lines, path stats) and the pileup kernel
// (pileup_kernels.hip).  Included behind device_common.h by .hip files only.
//
// A serial walk costs three dependent loads per unitig (path int -> meta -> bases) in every lane; here lane i takes unitig i of a pass of sixteen:
// all path ints, metas and the (k-1)-mers at both ends of both strands are in flight together, and what compactionEnd (utils.cpp:171-179) decides
// -- which strand of each unitig continues the walk, given the strand its predecessor was glued on in -- runs down the lanes by shuffles
// (state 0: forward strand at F, 1: reverse complement at F + len, 2: no walk).  A prefix sum of the new bases places every unitig in the walk.
// A path of any length takes ceil(n / 16) passes; the walk's size so far and the (k-1)-mer at its end are carried from one to the next.
// WIDE (k > 33: a (k-1)-mer is longer than one word): the overlap compare takes a second window for the bases behind the first 32.
#ifndef BGREAT_AMD_WALK_LANES_H
#define BGREAT_AMD_WALK_LANES_H

#include "device_common.h"

namespace bgr {
namespace {

// 16 bytes at p of which `valid` (>= 1) belong to the buffer; PADDED: the buffer may be read 15 bytes past its end (the text is)
template <bool PADDED>
__device__ __forceinline__ void load16p(const uint8_t* p, uint32_t valid, uint32_t w[4]) {
    if (PADDED || valid >= 16) {
        const u32x4_unaligned v = *reinterpret_cast<const u32x4_unaligned*>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        w[0] = w[1] = w[2] = w[3] = 0;
        for (uint32_t i = 0; i < valid; ++i) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    }
}
// shuffles inside a 16-lane group (64-bit by halves)
__device__ __forceinline__ u64 grp_get64(u64 x, uint32_t l) {
    return ((u64)(uint32_t)__shfl((int)(uint32_t)(x >> 32), (int)l, 16) << 32) | (uint32_t)__shfl((int)(uint32_t)x, (int)l, 16);
}
__device__ __forceinline__ u64 grp_up64(u64 x, uint32_t d) {
    return ((u64)(uint32_t)__shfl_up((int)(uint32_t)(x >> 32), d, 16) << 32) | (uint32_t)__shfl_up((int)(uint32_t)x, d, 16);
}

// bit i (0..15) = character i of the sixteen in ch[] is the one of "ACGT" that the 2-bit code of base i names (codes: base i at bits 31 - 2 i,
// 30 - 2 i); a character outside ACGT equals none
__device__ __forceinline__ uint32_t eq16_acgt(const uint32_t ch[4], uint32_t codes) {
    uint32_t eq = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t x = codes >> (24 - 8 * d);
        const uint32_t sel = ((x >> 6) & 3u) | (((x >> 4) & 3u) << 8) | (((x >> 2) & 3u) << 16) | ((x & 3u) << 24);
        eq |= nibble_of(bgr_zero_bytes(ch[d] ^ __builtin_amdgcn_perm(0u, 0x54474341u, sel))) << (4 * d);   // "ACGT" by code
    }
    return eq;
}

// what a pass hands the next one: the walk's size, the (k-1)-mer at its end
struct WalkCarry {
    u64 total = 0, cT = 0, cT2 = 0;
};
// one lane's unitig of a pass (lane `sub` holds unitig u0 + sub of the path)
struct WalkLane {
    int32_t sid = 0;      // the path int (0 behind the path's end)
    uint32_t id = 0, len = 0;
    uint32_t st = 2;      // the strand it was glued on in: 0 forward (at F), 1 reverse complement (at F + len)
    uint32_t last = 0;    // lane of the pass's last unitig
    bool on = false;      // a unitig of the path
    u64 F = 0;
    u64 start = 0, end = 0;      // its NEW bases lie at the walk positions [start, end) (its whole extent: [end - len, end))
    u64 pass_start = 0, pass_end = 0;   // the walk's size in front of and behind this pass, in every lane
};

// One pass of sixteen unitigs (u0, u0 + 16, ... in turn, starting with a fresh WalkCarry); false, in every lane: the path spells no walk (an id
// that is 0 or beyond the graph's, a unitig that glues on in neither strand).  Called by all sixteen lanes.
template <bool WIDE>
__device__ __forceinline__ bool walk_pass(const BgrDeviceGraph& g, const int32_t* path, uint32_t nu, uint32_t u0, uint32_t sub, WalkCarry& c, WalkLane& w) {
    const uint32_t K1 = g.k - 1, n_unitigs = (uint32_t)g.hdr->n_unitigs;
    const uint32_t sh1 = 64 - 2 * (WIDE ? 32 : K1), sh2 = WIDE ? 128 - 2 * K1 : 0;
    const uint32_t u = u0 + sub;
    const bool on = u < nu;
    const int32_t sid = on ? path[1 + u] : 0;
    const uint32_t id = (uint32_t)(sid < 0 ? -(int64_t)sid : (int64_t)sid);
    const bool ok = on && id != 0 && id <= n_unitigs;
    uint32_t len = 0;
    u64 F = 0, hA = 0, hB = 0, tA = 0, tB = 0, hA2 = 0, hB2 = 0, tA2 = 0, tB2 = 0;
    if (ok) {
        const BgrUnitigMeta m = g.meta[id];
        len = m.len; F = m.F;
        hA = win32(g.seq, F) >> sh1; hB = win32(g.seq, F + len) >> sh1;
        tA = win32(g.seq, F + len - K1) >> sh1; tB = win32(g.seq, F + 2ull * len - K1) >> sh1;
        if (WIDE) {
            hA2 = win32(g.seq, F + 32) >> sh2; hB2 = win32(g.seq, F + len + 32) >> sh2;
            tA2 = win32(g.seq, F + len - K1 + 32) >> sh2; tB2 = win32(g.seq, F + 2ull * len - K1 + 32) >> sh2;
        }
    }
    // the strand this unitig is glued on in when its predecessor lies on its strand A (rA) / B (rB)
    u64 pA = grp_up64(tA, 1), pB = grp_up64(tB, 1), pA2 = WIDE ? grp_up64(tA2, 1) : 0, pB2 = WIDE ? grp_up64(tB2, 1) : 0;
    if (sub == 0) { pA = pB = c.cT; pA2 = pB2 = c.cT2; }
    const uint32_t sS = sid > 0 ? 0u : 1u;   // the strand its sign names: compactionEnd's first try
    const u64 hS = sS ? hB : hA, hR = sS ? hA : hB, hS2 = sS ? hB2 : hA2, hR2 = sS ? hA2 : hB2;
    uint32_t rA = 2, rB = 2;
    if (ok) {
        rA = (hS == pA && hS2 == pA2) ? sS : (hR == pA && hR2 == pA2) ? sS ^ 1u : 2u;
        rB = (hS == pB && hS2 == pB2) ? sS : (hR == pB && hR2 == pB2) ? sS ^ 1u : 2u;
    }
    uint32_t st = sub == 0 ? (u0 == 0 ? (ok ? sS : 2u) : rA) : 2u;
#pragma unroll
    for (uint32_t j = 1; j < 16; ++j) {
        const uint32_t p = (uint32_t)__shfl_up((int)st, 1, 16);
        if (sub == j) st = p == 0 ? rA : p == 1 ? rB : 2u;
    }
    if (row16_sum(on && st == 2 ? 1u : 0u)) return false;
    // where it lies in the walk
    const u64 new_len = on ? (u64)len - (u == 0 ? 0u : K1) : 0ull;
    u64 inc = new_len;
#pragma unroll
    for (uint32_t d = 1; d < 16; d <<= 1) { const u64 up = grp_up64(inc, d); if (sub >= d) inc += up; }
    w.sid = sid; w.id = id; w.len = len; w.st = st; w.on = on; w.F = F;
    w.start = c.total + inc - new_len; w.end = c.total + inc;
    w.pass_start = c.total;
    w.pass_end = grp_get64(w.end, 15);
    w.last = nu - u0 < 16 ? nu - u0 - 1 : 15u;
    c.cT = grp_get64(st ? tB : tA, w.last);
    if (WIDE) c.cT2 = grp_get64(st ? tB2 : tA2, w.last);
    c.total = w.pass_end;
    return true;
}

}  // namespace
}  // namespace bgr

#endif
