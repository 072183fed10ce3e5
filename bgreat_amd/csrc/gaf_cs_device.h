// gaf_cs_device.h -- the differences of a mapped read from what its path spells, in the read's order, by the sixteen lanes of a group: what is
// underneath the cs:Z: field of a GAF line (--gaf --cs: the instances of the GAF kernels that carry it, text_gaf.hip) and bgr_aligner_path_diffs.
// Included by text_gaf.hip behind walk_lanes.h and text_device.h.
//
// The field is minimap2's short form with substitutions only: ":<n>" per maximal run of n equal characters, "*<path base><read base>" (lower case,
// "n" for a read character outside ACGT) per difference.  Its bytes must be known exactly before the line is written (lines are packed by a scan),
// and a run may span lanes (16 characters each), turns (256) and passes of the walk (16 unitigs).  So:
//   * cs_pieces hands out the read PIECE by piece in ascending read order, whatever the strand: per turn lane j holds the piece of characters
//     [16 (c0 + j), + 16) that lies under the pass, with its mask of differences and the path's bases.  The compare is gaf_stat's.  A read mapped on
//     its reverse complement meets the passes of its walk last first: each of them walks from the path's start again (paths of more than sixteen
//     unitigs only; one pass costs nothing more).
//   * a piece is summed up as a CsSpan -- the open run at its start, the open run at its end, the bytes of everything closed between --, spans join
//     associatively, a scan over the lanes by shuffles gives every lane what lies in front of its piece, and one span carries from turn to turn
//     and from pass to pass.  The run in front of a difference is written by the lane that holds the difference.
// No atomics, no LDS, nothing sized by the read's length.
#ifndef BGREAT_AMD_GAF_CS_DEVICE_H
#define BGREAT_AMD_GAF_CS_DEVICE_H

#include "device_common.h"
#include "text_device.h"
#include "walk_lanes.h"

namespace bgr {
namespace {

// bytes of ":<n>"; an empty run is not written
__device__ __forceinline__ uint32_t cs_run_bytes(uint32_t n) {
    return n == 0 ? 0u : n < 10 ? 2u : n < 100 ? 3u : n < 1000 ? 4u : n < 10000 ? 5u : n < 100000 ? 6u : n < 1000000 ? 7u : n < 10000000 ? 8u : n < 100000000 ? 9u : n < 1000000000 ? 10u : 11u;
}
// ":<n>" at d[pos ...] -> the position behind it (n >= 1)
__device__ __forceinline__ uint32_t cs_put_run(uint8_t* d, uint32_t pos, uint32_t n) {
    const uint32_t end = pos + cs_run_bytes(n);
    d[pos] = ':';
    put_dec(d + end, n);
    return end;
}

// A stretch of the read: any = it holds a difference; lead / trail = the equal characters at its start / end (both its whole length when it holds
// none); bytes = the differences and the runs that lie between two of them
struct CsSpan {
    uint32_t lead, trail, bytes, any;
};
__device__ __forceinline__ CsSpan cs_join(const CsSpan& a, const CsSpan& b) {   // a in front of b
    CsSpan r;
    r.any = a.any | b.any;
    r.lead = a.any ? a.lead : a.lead + b.lead;
    r.trail = b.any ? b.trail : a.trail + b.trail;
    r.bytes = a.bytes + b.bytes + (a.any && b.any ? cs_run_bytes(a.trail + b.lead) : 0u);
    return r;
}
__device__ __forceinline__ CsSpan cs_up(const CsSpan& s, uint32_t d) {
    CsSpan r;
    r.lead = (uint32_t)__shfl_up((int)s.lead, d, 16); r.trail = (uint32_t)__shfl_up((int)s.trail, d, 16);
    r.bytes = (uint32_t)__shfl_up((int)s.bytes, d, 16); r.any = (uint32_t)__shfl_up((int)s.any, d, 16);
    return r;
}
// where the tokens of what follows a span begin (the run at its end stays open), and the bytes of a whole line's span
__device__ __forceinline__ uint32_t cs_closed_bytes(const CsSpan& s) { return s.bytes + (s.any ? cs_run_bytes(s.lead) : 0u); }
__device__ __forceinline__ uint32_t cs_all_bytes(const CsSpan& s) { return cs_closed_bytes(s) + cs_run_bytes(s.trail); }

// codes of the bases of the characters i .. 15 of sixteen (base i at bits 31 - 2 i, 30 - 2 i)
__device__ __forceinline__ uint32_t cs_from(uint32_t i) { return i >= 16 ? 0u : 0xFFFFFFFFu >> (2 * i); }
__device__ __forceinline__ uint32_t cs_char(const uint4& ch, uint32_t i) {
    const uint32_t w = i < 4 ? ch.x : i < 8 ? ch.y : i < 12 ? ch.z : ch.w;
    return (w >> (8 * (i & 3))) & 0xFFu;
}
__device__ __forceinline__ uint32_t cs_read_code(uint32_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }   // 4: outside ACGT
__device__ __forceinline__ uint8_t cs_lower(uint32_t code) { return (uint8_t)((0x6E74676361ull >> (8 * code)) & 0xFF); }   // "acgtn"

// The read of a mapped row whose path spells a walk (the caller has gaf_stat's word for it), piece by piece in ascending read order:
// f(t0, a, b, mm, pc, ch) is called by all sixteen lanes once per turn; the lane's piece are the read positions [t0 + a, t0 + b) (a == b: none
// this turn), bit i of mm: position t0 + i differs from the path, pc: the path's bases there in the read's direction (cs_from's layout), ch: the
// sixteen characters from t0 on.
template <bool WIDE, bool PADDED, class F>
__device__ __forceinline__ void cs_pieces(const BgrDeviceGraph& g, const int32_t* path, uint32_t np, const uint8_t* read, uint32_t L, bool rc, uint32_t sub, F&& f) {
    const u64 off = (u64)path[0];
    const uint32_t nu = np - 1, K1 = g.k - 1, npass = (nu + 15) / 16;
    WalkCarry carry;
    for (uint32_t q = 0; q < npass; ++q) {
        const uint32_t p = rc ? npass - 1 - q : q;
        WalkLane w;
        if (!rc) {
            if (!walk_pass<WIDE>(g, path, nu, 16 * p, sub, carry, w)) return;
        } else {
            carry = WalkCarry();
            for (uint32_t x = 0; x <= p; ++x) if (!walk_pass<WIDE>(g, path, nu, 16 * x, sub, carry, w)) return;
        }
        const uint32_t u = 16 * p + sub, len = w.len, st = w.st, cnt = w.last + 1;
        const u64 F0 = w.F, start = w.start, end = w.end, total = w.pass_start, pass_end = w.pass_end;
        const u64 skip = u == 0 ? 0u : K1;   // (gaf_stat has the derivation)
        const int64_t cst = !rc ? (int64_t)(F0 + (st ? len : 0u) + skip) + (int64_t)off - (int64_t)start
                                : (int64_t)(F0 + (st ? 0u : len) + len - skip) + (int64_t)start - (int64_t)off - (int64_t)L;
        const u64 lo = total > off ? total : off, hi = pass_end < off + L ? pass_end : off + L;
        if (lo >= hi) continue;
        const uint32_t tlo = !rc ? (uint32_t)(lo - off) : L - (uint32_t)(hi - off), thi = !rc ? (uint32_t)(hi - off) : L - (uint32_t)(lo - off);
        for (uint32_t c0 = tlo >> 4; 16 * (u64)c0 < thi; c0 += 16) {
            const uint32_t t0 = 16 * (c0 + sub);
            const bool mine = t0 < thi;
            const uint32_t ca = tlo > t0 ? tlo : t0, cb = thi < t0 + 16 ? thi : t0 + 16;
            uint32_t ch[4] = {0, 0, 0, 0};
            if (mine) load16p<PADDED>(read + t0, L - t0, ch);
            uint32_t mm = 0, pc = 0;
            for (uint32_t v = 0; v < cnt; ++v) {
                const u64 sv = grp_get64(start, v), ev = grp_get64(end, v);
                const int64_t cv = (int64_t)grp_get64((u64)cst, v);
                const int64_t va = !rc ? (int64_t)sv - (int64_t)off : (int64_t)L - ((int64_t)ev - (int64_t)off);
                const int64_t vb = !rc ? (int64_t)ev - (int64_t)off : (int64_t)L - ((int64_t)sv - (int64_t)off);
                const int64_t xa = va > (int64_t)ca ? va : (int64_t)ca, xb = vb < (int64_t)cb ? vb : (int64_t)cb;
                if (mine && xa < xb) {
                    const uint32_t a = (uint32_t)xa - t0, b = (uint32_t)xb - t0;
                    const uint32_t codes = (uint32_t)(win32(g.seq, (u64)(xa + cv)) >> 32) >> (2 * a);
                    const uint32_t eq = eq16_acgt(ch, codes);
                    mm |= ~eq & ((1u << b) - 1u) & ~((1u << a) - 1u);
                    pc |= codes & cs_from(a) & ~cs_from(b);
                }
            }
            f(t0, mine ? ca - t0 : 0u, mine ? cb - t0 : 0u, mm, pc, make_uint4(ch[0], ch[1], ch[2], ch[3]));
        }
    }
}

// The ops of the field: their bytes in every lane; WRITE: and the bytes themselves at d (the lane that holds a difference writes the run in front
// of it and the difference; lane 0 the run at the line's end)
template <bool WIDE, bool PADDED, bool WRITE>
__device__ __forceinline__ uint32_t cs_ops(const BgrDeviceGraph& g, const int32_t* path, uint32_t np, const uint8_t* read, uint32_t L, bool rc, uint32_t sub, uint8_t* d) {
    CsSpan run = {0, 0, 0, 0};
    cs_pieces<WIDE, PADDED>(g, path, np, read, L, rc, sub, [&](uint32_t, uint32_t a, uint32_t b, uint32_t mm, uint32_t pc, const uint4& ch) {
        CsSpan me = {b - a, b - a, 0, 0};
        if (mm) {
            const uint32_t first = (uint32_t)__ffs((int)mm) - 1;
            me.any = 1;
            me.lead = first - a;
            me.trail = b - (32u - (uint32_t)__clz((int)mm));
            me.bytes = 3u * (uint32_t)__popc(mm);
            uint32_t prev = first + 1;
            for (uint32_t m = mm & (mm - 1); m; m &= m - 1) {
                const uint32_t i = (uint32_t)__ffs((int)m) - 1;
                me.bytes += cs_run_bytes(i - prev);
                prev = i + 1;
            }
        }
        CsSpan inc = me;
#pragma unroll
        for (uint32_t s = 1; s < 16; s <<= 1) {
            const CsSpan up = cs_up(inc, s);
            if (sub >= s) inc = cs_join(up, inc);
        }
        if (WRITE) {
            CsSpan ex = cs_up(inc, 1);
            if (sub == 0) ex = CsSpan{0, 0, 0, 0};
            if (mm) {
                const CsSpan front = cs_join(run, ex);
                uint32_t pos = cs_closed_bytes(front), open = front.trail, prev = a;
                for (uint32_t m = mm; m; m &= m - 1) {
                    const uint32_t i = (uint32_t)__ffs((int)m) - 1;
                    open += i - prev;
                    if (open) pos = cs_put_run(d, pos, open);
                    d[pos] = '*';
                    d[pos + 1] = cs_lower((pc >> (30 - 2 * i)) & 3u);
                    d[pos + 2] = cs_lower(cs_read_code(cs_char(ch, i)));
                    pos += 3;
                    open = 0;
                    prev = i + 1;
                }
            }
        }
        CsSpan all;
        all.lead = (uint32_t)__shfl((int)inc.lead, 15, 16); all.trail = (uint32_t)__shfl((int)inc.trail, 15, 16);
        all.bytes = (uint32_t)__shfl((int)inc.bytes, 15, 16); all.any = (uint32_t)__shfl((int)inc.any, 15, 16);
        run = cs_join(run, all);
    });
    if (WRITE && sub == 0 && run.trail) cs_put_run(d, cs_closed_bytes(run), run.trail);
    return cs_all_bytes(run);
}

// The differences themselves, ascending read position, at out[0 ...] (two words each: bgr_path_diff): as many as gaf_stat counted
template <bool WIDE, bool PADDED>
__device__ __forceinline__ void cs_diffs(const BgrDeviceGraph& g, const int32_t* path, uint32_t np, const uint8_t* read, uint32_t L, bool rc, uint32_t sub, uint2* out) {
    uint32_t n = 0;
    cs_pieces<WIDE, PADDED>(g, path, np, read, L, rc, sub, [&](uint32_t t0, uint32_t, uint32_t, uint32_t mm, uint32_t pc, const uint4& ch) {
        const uint32_t c = (uint32_t)__popc(mm);
        uint32_t inc = c;
#pragma unroll
        for (uint32_t s = 1; s < 16; s <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)inc, s, 16);
            if (sub >= s) inc += up;
        }
        uint32_t at = n + inc - c;
        for (uint32_t m = mm; m; m &= m - 1) {
            const uint32_t i = (uint32_t)__ffs((int)m) - 1;
            out[at++] = make_uint2(t0 + i, ((pc >> (30 - 2 * i)) & 3u) | (cs_read_code(cs_char(ch, i)) << 8));
        }
        n += (uint32_t)__shfl((int)inc, 15, 16);
    });
}

}  // namespace
}  // namespace bgr

#endif
