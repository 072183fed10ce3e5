// text_gaf.hip -- GAF output (--gaf, want_output 3) of the text route on the device (gfx950): one line per mapped read -- strand, coordinates
// and mismatches; the tagged instances behind --haplotag; and bgr_aligner_path_stats, the same per-read function over a device-resident launch.
// The kernels and their launchers (text_kernels.h).
// The walk is the one -c spells (WalkIter), the line describes the read as it stands in the input: a read mapped on its reverse complement
// (BGR_ST_RC) has its path written reversed with every orientation flipped.  With walk offset off = path[0], read size L, plen = size of
// the walk, cl = min(L, plen - off):   forward: query [0, cl), path [off, off + cl);   on the rc: query [L - cl, L), path [plen - off - cl, plen - off).
// NM counts the positions where the read's characters differ from what the path spells there (an N always differs).  Graphs without
// exception planes only, as -c on the device.  A 16-lane group per read: the unitigs of the path are spread over the lanes (gaf_stat), then the compare,
// 16 characters per lane-step -- characters by one 16-byte load, bases by one 64-bit window of the 2-bit store.
#include "device_common.h"
#include "text_kernels.h"
#include "text_device.h"
#include "walk_lanes.h"
#include "haplotag_device.h"
#include "gaf_cs_device.h"

namespace bgr {
namespace {

struct GafStat {
    u64 plen = 0;
    uint32_t cl = 0, nm = 0, segbytes = 0;   // segbytes: characters of the segment column ('>' or '<' and the id, per unitig)
    uint32_t obits = 0;                      // bit i: unitig i of the path (the first 32) was glued on in its forward strand
    bool bad = false;                        // the path spells no walk (the -c kernels' bug-compaction condition)
    int32_t sid0 = 0;                        // this lane's path int of the first pass (0 behind the path's end): what the tagged instances vote with
};
// the header's name: its characters behind the first one ('>' or '@') up to the first space or tab -> their number (0: the line gets '*')
__device__ __forceinline__ uint32_t gaf_name_len(const uint8_t* text, uint32_t p, uint32_t hl, uint32_t sub) {
    if (hl < 2) return 0;
    const uint32_t s = p + 1, e = p + hl;
    for (uint32_t base = s; base < e; base += 256) {
        uint32_t w[4];
        const uint32_t at = base + 16 * sub;
        load16(text, at, e, w);
        const uint32_t m = mask16(w, 0x20202020u) | mask16(w, 0x09090909u);
        const uint32_t first = row16_min(m ? at + (uint32_t)__ffs((int)m) - 1 : kNone);
        if (first != kNone) return first - s;
    }
    return e - s;
}
// The walk of one mapped read's path (np >= 1 ints) and the compare of the read with it, by the 16 lanes of a group; the results in every lane.
// read: its L characters as they stand in the input.  The walk itself -- lane i takes unitig i of a pass of sixteen -- is walk_pass (walk_lanes.h);
// then lane c takes the read's characters [16 c, 16 c + 16) and compares them with the one or two unitigs that lie under them.
template <bool WIDE, bool PADDED>
__device__ __forceinline__ GafStat gaf_stat(const BgrDeviceGraph& g, const int32_t* path, uint32_t np, const uint8_t* read, uint32_t L, bool rc, uint32_t sub) {
    GafStat s;
    const int32_t off_s = path[0];
    if (np < 2 || off_s < 0) { s.bad = true; return s; }
    const u64 off = (u64)off_s;
    const uint32_t nu = np - 1, K1 = g.k - 1;
    WalkCarry carry;
    uint32_t nm = 0;
    for (uint32_t u0 = 0; u0 < nu; u0 += 16) {
        WalkLane w;
        if (!walk_pass<WIDE>(g, path, nu, u0, sub, carry, w)) { s.bad = true; return s; }
        const uint32_t u = u0 + sub, id = w.id, len = w.len, st = w.st, last = w.last;
        const bool on = w.on;
        if (u0 == 0) s.sid0 = w.sid;
        const u64 F = w.F, start = w.start, end = w.end, total = w.pass_start, pass_end = w.pass_end;
        s.segbytes += row16_sum(on ? 1u + dec_digits(id) : 0u);
        s.obits |= row16_sum(on && u < 32 && st == 0 ? 1u << u : 0u);
        // read position t faces base t + cst of the store: forward the strand it was glued on in; on the rc the read runs against the walk, i.e. along
        // the unitig's OTHER strand (the store holds both)
        const u64 skip = u == 0 ? 0u : K1;
        const int64_t cst = !rc ? (int64_t)(F + (st ? len : 0u) + skip) + (int64_t)off - (int64_t)start
                                : (int64_t)(F + (st ? 0u : len) + len - skip) + (int64_t)start - (int64_t)off - (int64_t)L;
        const u64 lo = total > off ? total : off, hi = pass_end < off + L ? pass_end : off + L;   // walk positions of this pass that lie under the read
        if (lo < hi) {
            const uint32_t tlo = !rc ? (uint32_t)(lo - off) : L - (uint32_t)(hi - off), thi = !rc ? (uint32_t)(hi - off) : L - (uint32_t)(lo - off);
            const uint32_t cnt = last + 1;
            for (uint32_t c0 = tlo >> 4; 16 * (u64)c0 < thi; c0 += 16) {   // (every lane takes every turn: the shuffles below need them all)
                const uint32_t t0 = 16 * (c0 + sub);
                const bool mine = t0 < thi;
                const uint32_t ca = tlo > t0 ? tlo : t0, cb = thi < t0 + 16 ? thi : t0 + 16;   // the read positions [ca, cb) of these 16
                uint32_t ch[4] = {0, 0, 0, 0};
                if (mine) load16p<PADDED>(read + t0, L - t0, ch);
                for (uint32_t v = 0; v < cnt; ++v) {
                    const u64 sv = grp_get64(start, v), ev = grp_get64(end, v);
                    const int64_t cv = (int64_t)grp_get64((u64)cst, v);
                    // unitig v's new bases [sv, ev) of the walk in read positions
                    const int64_t va = !rc ? (int64_t)sv - (int64_t)off : (int64_t)L - ((int64_t)ev - (int64_t)off);
                    const int64_t vb = !rc ? (int64_t)ev - (int64_t)off : (int64_t)L - ((int64_t)sv - (int64_t)off);
                    const int64_t xa = va > (int64_t)ca ? va : (int64_t)ca, xb = vb < (int64_t)cb ? vb : (int64_t)cb;
                    if (mine && xa < xb) {
                        const uint32_t a = (uint32_t)xa - t0, b = (uint32_t)xb - t0;
                        const uint32_t codes = (uint32_t)(win32(g.seq, (u64)(xa + cv)) >> 32) >> (2 * a);   // base of character i at bits 31 - 2 i, 30 - 2 i
                        const uint32_t eq = eq16_acgt(ch, codes);
                        nm += (uint32_t)__popc(~eq & ((1u << b) - 1u) & ~((1u << a) - 1u));
                    }
                }
            }
        }
    }
    const u64 total = carry.total;
    if (off > total) { s.bad = true; return s; }
    s.plen = total;
    s.cl = total - off < L ? (uint32_t)(total - off) : L;
    s.nm = row16_sum(nm);
    return s;
}
// where the line's intervals lie (see above)
__device__ __forceinline__ void gaf_intervals(bool rc, uint32_t L, u64 off, u64 plen, uint32_t cl, uint32_t& qs, uint32_t& qe, u64& pstart) {
    if (!rc) { qs = 0; qe = cl; pstart = off; }
    else { qs = L - cl; qe = L; pstart = plen - (off + cl); }
}
// the line without its name and its segment column: 9 numbers, 12 tabs, '+', "255", "NM:i:", '\n'
__device__ __forceinline__ uint32_t gaf_fixed_bytes(uint32_t L, uint32_t qs, uint32_t qe, u64 plen, u64 pstart, uint32_t cl, uint32_t nm) {
    return 22 + dec_digits(L) + dec_digits(qs) + dec_digits(qe) + dec_digits(plen) + dec_digits(pstart) + dec_digits(pstart + cl) + dec_digits(cl - nm) + dec_digits(cl) + dec_digits(nm);
}

// sizes: a mapped read's line in the paths stream, the others' header + '\n' + read + '\n' in the notAligned stream; what the write kernel needs
// again is kept per read: row = {plen, strand bits of the first 32 unitigs, cl, NM | bit 31: the row does not hold it all (a longer path, a walk of
// 2^32 bases): the write kernel walks the path itself}, nlen = characters of the name.  (Measured: with the write kernel walking every path for the
// orientations, as -c's does for the bases, it took 150 us per 262 144 reads, of which the walk's dependent loads were two thirds.)
// *bug as correct_sizes sets it.
// TAG (the aligner has a tag table, bgr_aligner_haplotag_enable): the read's tag is computed here, where the walk holds the path's first sixteen ids in
// its lanes, kept in tags[a] next to the row, and the bytes of its five fields are part of the line's size.
// CS (bgr_aligner_gaf_cs_enable): the line ends in "\tcs:Z:" + the ops of gaf_cs_device.h; their bytes are part of the line's size and kept in csb[a].
// A read without a difference -- most are -- has the one run ":<cl>" and is not compared again.
__device__ __forceinline__ uint32_t gaf_tag_bytes(const bgr_read_tag& t) {   // "\tPS:i:" and its four siblings, HP's one digit, four numbers
    return t.block ? 31 + dec_digits(t.block) + dec_digits(t.a) + dec_digits(t.b) + dec_digits(t.others) : 0u;
}
template <bool WIDE, bool TAG, bool CS = false>
__device__ __forceinline__ void gaf_sizes(const BgrDeviceGraph& g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec, const uint32_t* acc_rec,
                                          uint32_t n_acc, uint32_t* psz, uint32_t* nsz, uint32_t* nlen, uint4* rows, uint32_t* bug, const uint32_t* tag_table, uint4* tags,
                                          uint32_t* csb = nullptr) {
    const uint32_t a = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, sub = threadIdx.x & 15;
    if (a >= n_acc) return;
    const uint2 res = results[a];
    const uint4 r = rec[acc_rec[a]];
    const uint32_t np = res.y & 0xFFFFFFu, L = r.w & 0x7FFFFFFFu;
    uint32_t ps = 0, ns = 0, nl = 0, cs = 0;
    uint4 row = make_uint4(0, 0, 0, 0);
    bgr_read_tag tag = {0, 0, 0, 0};
    if (np) {
        const bool rc = ((res.y >> 24) & BGR_ST_RC) != 0;
        const GafStat s = gaf_stat<WIDE, true>(g, arena + res.x, np, text + r.z, L, rc, sub);
        if (s.bad) { if (sub == 0) atomicMin(bug, a); }
        else {
            if (TAG) {   // (np >= 2 here; every lane of the group is: s.bad is the same in all sixteen)
                const uint32_t n_unitigs = (uint32_t)g.hdr->n_unitigs;
                tag = haplotag_group(tag_table, n_unitigs, arena + res.x + 1, np - 1, haplotag_vote(tag_table, n_unitigs, s.sid0), sub);
            }
            nl = gaf_name_len(text, r.x, r.y, sub);
            uint32_t qs, qe;
            u64 pstart;
            gaf_intervals(rc, L, (u64)arena[res.x], s.plen, s.cl, qs, qe, pstart);
            ps = (nl ? nl : 1u) + s.segbytes + gaf_fixed_bytes(L, qs, qe, s.plen, pstart, s.cl, s.nm) + (TAG ? gaf_tag_bytes(tag) : 0u);
            if (CS) {   // (s.nm is the same in all sixteen)
                cs = s.nm == 0 ? cs_run_bytes(s.cl) : cs_ops<WIDE, true, false>(g, arena + res.x, np, text + r.z, L, rc, sub, nullptr);
                ps += 6 + cs;
            }
            const bool again = np - 1 > 32 || (s.plen >> 32) != 0;   // (more than the row holds: the write kernel walks the path itself)
            row = make_uint4((uint32_t)s.plen, s.obits, s.cl, s.nm | (again ? 0x80000000u : 0u));
        }
    } else {
        ns = r.y + L + 2;
    }
    if (sub == 0) { psz[a] = ps; nsz[a] = ns; nlen[a] = nl; rows[a] = row; }
    if (TAG && sub == 1) tags[a] = make_uint4(tag.block, tag.a, tag.b, tag.others);
    if (CS && sub == 2) csb[a] = cs;
}
__global__ void __launch_bounds__(256) bgr_text_gaf_sizes_kernel(BgrDeviceGraph g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec,
                                                                 const uint32_t* acc_rec, uint32_t n_acc, uint32_t* psz, uint32_t* nsz, uint32_t* nlen, uint4* rows, uint32_t* bug) {
    gaf_sizes<false, false>(g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug, nullptr, nullptr);
}
__global__ void __launch_bounds__(256) bgr_text_gaf_sizes_wide_kernel(BgrDeviceGraph g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec,
                                                                      const uint32_t* acc_rec, uint32_t n_acc, uint32_t* psz, uint32_t* nsz, uint32_t* nlen, uint4* rows, uint32_t* bug) {
    gaf_sizes<true, false>(g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug, nullptr, nullptr);
}
template <bool WIDE>
__global__ void __launch_bounds__(256) bgr_text_gaf_sizes_tag_kernel(BgrDeviceGraph g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec,
                                                                     const uint32_t* acc_rec, uint32_t n_acc, uint32_t* psz, uint32_t* nsz, uint32_t* nlen, uint4* rows, uint32_t* bug,
                                                                     const uint32_t* tag_table, uint4* tags) {
    gaf_sizes<WIDE, true>(g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug, tag_table, tags);
}
template <bool WIDE, bool TAG>
__global__ void __launch_bounds__(256) bgr_text_gaf_sizes_cs_kernel(BgrDeviceGraph g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec,
                                                                    const uint32_t* acc_rec, uint32_t n_acc, uint32_t* psz, uint32_t* nsz, uint32_t* nlen, uint4* rows, uint32_t* bug,
                                                                    const uint32_t* tag_table, uint4* tags, uint32_t* csb) {
    gaf_sizes<WIDE, TAG, true>(g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug, tag_table, tags, csb);
}

// lead + to_string(v) at d[pos ...] by the lane whose turn it is -> the position behind it (every lane keeps count)
__device__ __forceinline__ uint32_t gaf_put(uint8_t* d, uint32_t pos, u64 v, bool mine, uint8_t lead = '\t') {
    const uint32_t end = pos + 1 + dec_digits(v);
    if (mine) { d[pos] = lead; put_dec(d + end, v); }
    return end;
}
// "\t" c0 c1 ":i:" to_string(v) at d[pos ...] by the lane whose turn it is -> the position behind it
__device__ __forceinline__ uint32_t gaf_put_tag(uint8_t* d, uint32_t pos, uint8_t c0, uint8_t c1, uint32_t v, bool mine) {
    const uint32_t end = pos + 6 + dec_digits(v);
    if (mine) { d[pos] = '\t'; d[pos + 1] = c0; d[pos + 2] = c1; d[pos + 3] = ':'; d[pos + 4] = 'i'; d[pos + 5] = ':'; put_dec(d + end, v); }
    return end;
}
// one 16-lane group per accepted read: a mapped read's line at its offset (the numbers by one lane each, the segments by the lanes in turn),
// the others into the notAligned stream as correct_write sends them.  TAG: the five fields of tags[a] behind NM, by the lanes 12 .. 15 and 0.
// CS: "\tcs:Z:" and the csb[a] bytes of the ops behind everything else, the ops by the lanes that hold the differences (gaf_cs_device.h)
template <bool WIDE, bool TAG, bool CS = false>
__device__ __forceinline__ void gaf_write(const BgrDeviceGraph& g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec, const uint32_t* acc_rec,
                                          uint32_t n_acc, const uint32_t* poff, const uint32_t* noff, const uint32_t* psz, const uint32_t* nlen, const uint4* rows,
                                          uint8_t* pout, uint8_t* nout, const uint4* tags, const uint32_t* csb = nullptr) {
    const uint32_t a = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, sub = threadIdx.x & 15;
    if (a >= n_acc) return;
    const uint2 res = results[a];
    const uint4 r = rec[acc_rec[a]];
    const uint32_t np = res.y & 0xFFFFFFu, hl = r.y, L = r.w & 0x7FFFFFFFu;
    if (!np) {   // alignerGreedy.cpp:421-427: header + '\n' + read + '\n'
        uint8_t* d = nout + noff[a];
        group_copy(d, text + r.x, hl, sub);
        if (sub == 0) d[hl] = '\n';
        group_copy(d + hl + 1, text + r.z, L, sub);
        if (sub == 0) d[hl + 1 + L] = '\n';
        return;
    }
    uint8_t* d = pout + poff[a];
    const uint4 row = rows[a];
    const uint32_t nl = nlen[a], line = psz[a], cl = row.z, nm = row.w & 0x7FFFFFFFu;
    if (!line) return;   // (a path that spells no walk: the call ends without this stream)
    const bool again = (row.w >> 31) != 0;
    const u64 off = (u64)arena[res.x];
    u64 plen = row.x;
    if (again) {
        WalkIter<WIDE> w0(g, arena + res.x, np);
        plen = 0;
        if (w0.first()) { plen = w0.len; while (w0.next()) plen += w0.len - w0.skip; }
    }
    const bool rc = ((res.y >> 24) & BGR_ST_RC) != 0;
    uint32_t qs, qe;
    u64 pstart;
    gaf_intervals(rc, L, off, plen, cl, qs, qe, pstart);
    const uint32_t name = nl ? nl : 1u;
    bgr_read_tag tag = {0, 0, 0, 0};
    if (TAG) { const uint4 t = tags[a]; tag.block = t.x; tag.a = t.y; tag.b = t.z; tag.others = t.w; }
    const uint32_t csbytes = CS ? csb[a] : 0u;
    const uint32_t segbytes = line - name - gaf_fixed_bytes(L, qs, qe, plen, pstart, cl, nm) - (TAG ? gaf_tag_bytes(tag) : 0u) - (CS ? 6u + csbytes : 0u);
    if (nl) group_copy(d, text + r.x + 1, nl, sub);
    else if (sub == 0) d[0] = '*';
    uint32_t pos = name;
    pos = gaf_put(d, pos, L, sub == 1);
    pos = gaf_put(d, pos, qs, sub == 2);
    pos = gaf_put(d, pos, qe, sub == 3);
    if (sub == 4) { d[pos] = '\t'; d[pos + 1] = '+'; d[pos + 2] = '\t'; }
    const uint32_t seg0 = pos + 3;
    pos = seg0 + segbytes;
    pos = gaf_put(d, pos, plen, sub == 5);
    pos = gaf_put(d, pos, pstart, sub == 6);
    pos = gaf_put(d, pos, pstart + cl, sub == 7);
    pos = gaf_put(d, pos, cl - nm, sub == 8);
    pos = gaf_put(d, pos, cl, sub == 9);
    if (sub == 10) { d[pos] = '\t'; d[pos + 1] = '2'; d[pos + 2] = '5'; d[pos + 3] = '5'; d[pos + 4] = '\t'; d[pos + 5] = 'N'; d[pos + 6] = 'M'; d[pos + 7] = ':'; d[pos + 8] = 'i'; }
    pos = gaf_put(d, pos + 9, nm, sub == 11, ':');
    if (TAG && tag.block) {
        pos = gaf_put_tag(d, pos, 'P', 'S', tag.block, sub == 12);
        pos = gaf_put_tag(d, pos, 'H', 'P', tag.a > tag.b ? 1u : tag.b > tag.a ? 2u : 0u, sub == 13);
        pos = gaf_put_tag(d, pos, 'h', 'a', tag.a, sub == 14);
        pos = gaf_put_tag(d, pos, 'h', 'b', tag.b, sub == 15);
        pos = gaf_put_tag(d, pos, 'h', 'o', tag.others, sub == 0);
        if (!CS && sub == 0) d[pos] = '\n';
    } else if (!CS && sub == 12) d[pos] = '\n';
    if (CS) {
        uint8_t* o = d + pos + 6;
        if (sub == 1) { d[pos] = '\t'; d[pos + 1] = 'c'; d[pos + 2] = 's'; d[pos + 3] = ':'; d[pos + 4] = 'Z'; d[pos + 5] = ':'; }
        if (nm == 0) { if (sub == 2 && cl) cs_put_run(o, 0, cl); }
        else cs_ops<WIDE, true, true>(g, arena + res.x, np, text + r.z, L, rc, sub, o);
        if (sub == 3) o[csbytes] = '\n';
    }
    // the segments: lane (i - 1) mod 16 writes unitig i -- from the front, or on the rc from the back with its orientation flipped
    if (!again) {
        uint32_t acc = 0;
        for (uint32_t i = 1; i < np; ++i) {
            const int32_t sid = arena[res.x + i];
            const uint32_t id = (uint32_t)(sid < 0 ? -(int64_t)sid : (int64_t)sid);
            const uint32_t len = 1 + dec_digits(id);
            if (acc + len > segbytes) break;
            if (((i - 1) & 15u) == sub) {
                const bool fwd = ((row.y >> (i - 1)) & 1u) != 0;
                uint8_t* p = d + seg0 + (rc ? segbytes - acc - len : acc);
                *p = fwd != rc ? '>' : '<';
                put_dec(p + len, id);
            }
            acc += len;
        }
        return;
    }
    WalkIter<WIDE> w(g, arena + res.x, np);   // (every lane walks the path)
    if (!w.first()) return;
    uint32_t acc = 0;
    for (;;) {
        const int32_t sid = arena[res.x + w.i];
        const uint32_t id = (uint32_t)(sid < 0 ? -(int64_t)sid : (int64_t)sid);
        const uint32_t len = 1 + dec_digits(id);
        if (acc + len > segbytes) break;
        if (((w.i - 1) & 15u) == sub) {
            const bool fwd = w.base == g.meta[id].F;
            uint8_t* p = d + seg0 + (rc ? segbytes - acc - len : acc);
            *p = fwd != rc ? '>' : '<';
            put_dec(p + len, id);
        }
        acc += len;
        if (!w.next()) break;
    }
}
__global__ void __launch_bounds__(256) bgr_text_gaf_write_kernel(BgrDeviceGraph g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec,
                                                                 const uint32_t* acc_rec, uint32_t n_acc, const uint32_t* poff, const uint32_t* noff, const uint32_t* psz,
                                                                 const uint32_t* nlen, const uint4* rows, uint8_t* pout, uint8_t* nout) {
    gaf_write<false, false>(g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout, nullptr);
}
__global__ void __launch_bounds__(256) bgr_text_gaf_write_wide_kernel(BgrDeviceGraph g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec,
                                                                      const uint32_t* acc_rec, uint32_t n_acc, const uint32_t* poff, const uint32_t* noff, const uint32_t* psz,
                                                                      const uint32_t* nlen, const uint4* rows, uint8_t* pout, uint8_t* nout) {
    gaf_write<true, false>(g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout, nullptr);
}
template <bool WIDE>
__global__ void __launch_bounds__(256) bgr_text_gaf_write_tag_kernel(BgrDeviceGraph g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec,
                                                                     const uint32_t* acc_rec, uint32_t n_acc, const uint32_t* poff, const uint32_t* noff, const uint32_t* psz,
                                                                     const uint32_t* nlen, const uint4* rows, uint8_t* pout, uint8_t* nout, const uint4* tags) {
    gaf_write<WIDE, true>(g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout, tags);
}
template <bool WIDE, bool TAG>
__global__ void __launch_bounds__(256) bgr_text_gaf_write_cs_kernel(BgrDeviceGraph g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec,
                                                                    const uint32_t* acc_rec, uint32_t n_acc, const uint32_t* poff, const uint32_t* noff, const uint32_t* psz,
                                                                    const uint32_t* nlen, const uint4* rows, uint8_t* pout, uint8_t* nout, const uint4* tags, const uint32_t* csb) {
    gaf_write<WIDE, TAG, true>(g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout, tags, csb);
}

// bgr_aligner_path_stats: the same per-read function over the results of a bgr_align_device launch, the reads where the caller keeps them
// (their buffer is not padded).  out[i] = {plen low, plen high, path start low, path start high, cl, NM | no-walk flag}; zeros for an unmapped read
// and for a row that does not lie wholly inside the launch's arena_ints (an empty row, as the counting kernels take it).
template <bool WIDE>
__device__ __forceinline__ void path_stats(const BgrDeviceGraph& g, const uint8_t* reads, const u64* offs, const uint2* results, const int32_t* arena, u64 arena_ints, uint32_t n, uint32_t* out) {
    const uint32_t a = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, sub = threadIdx.x & 15;
    if (a >= n) return;
    const uint2 res = results[a];
    const uint32_t np = res.y & 0xFFFFFFu;
    u64 plen = 0, pstart = 0;
    uint32_t cl = 0, nm = 0;
    if (np && (u64)res.x + np <= arena_ints) {
        const u64 o0 = offs[a];
        const uint32_t L = (uint32_t)(offs[a + 1] - o0);
        const bool rc = ((res.y >> 24) & BGR_ST_RC) != 0;
        const GafStat s = gaf_stat<WIDE, false>(g, arena + res.x, np, reads + o0, L, rc, sub);
        if (s.bad) nm = 0x80000000u;
        else {
            uint32_t qs, qe;
            gaf_intervals(rc, L, (u64)arena[res.x], s.plen, s.cl, qs, qe, pstart);
            plen = s.plen; cl = s.cl; nm = s.nm;
        }
    }
    if (sub < 6) {
        const uint32_t v = sub == 0 ? (uint32_t)plen : sub == 1 ? (uint32_t)(plen >> 32) : sub == 2 ? (uint32_t)pstart : sub == 3 ? (uint32_t)(pstart >> 32) : sub == 4 ? cl : nm;
        out[6ull * a + sub] = v;
    }
}
__global__ void __launch_bounds__(256) bgr_path_stats_kernel(BgrDeviceGraph g, const uint8_t* reads, const u64* offs, const uint2* results, const int32_t* arena, u64 arena_ints, uint32_t n, uint32_t* out) {
    path_stats<false>(g, reads, offs, results, arena, arena_ints, n, out);
}
__global__ void __launch_bounds__(256) bgr_path_stats_wide_kernel(BgrDeviceGraph g, const uint8_t* reads, const u64* offs, const uint2* results, const int32_t* arena, u64 arena_ints, uint32_t n, uint32_t* out) {
    path_stats<true>(g, reads, offs, results, arena, arena_ints, n, out);
}


// bgr_aligner_path_diffs: the differences of every read of a bgr_align_device launch as structs.  Count (gaf_stat's NM per read; nothing for an
// unmapped read, a row not wholly inside the arena, a path that spells no walk), the scan of launch_scan2_u32, fill (cs_diffs, the function under
// the cs:Z: ops, at the read's offset; the caller has checked that all of them fit).
template <bool WIDE>
__global__ void __launch_bounds__(256) bgr_path_diffs_count_kernel(BgrDeviceGraph g, const uint8_t* reads, const u64* offs, const uint2* results, const int32_t* arena, u64 arena_ints,
                                                                   uint32_t n, uint32_t* cnt) {
    const uint32_t a = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, sub = threadIdx.x & 15;
    if (a >= n) return;
    const uint2 res = results[a];
    const uint32_t np = res.y & 0xFFFFFFu;
    uint32_t nm = 0;
    if (np && (u64)res.x + np <= arena_ints) {
        const u64 o0 = offs[a];
        const GafStat s = gaf_stat<WIDE, false>(g, arena + res.x, np, reads + o0, (uint32_t)(offs[a + 1] - o0), ((res.y >> 24) & BGR_ST_RC) != 0, sub);
        if (!s.bad) nm = s.nm;
    }
    if (sub == 0) cnt[a] = nm;
}
template <bool WIDE>
__global__ void __launch_bounds__(256) bgr_path_diffs_fill_kernel(BgrDeviceGraph g, const uint8_t* reads, const u64* offs, const uint2* results, const int32_t* arena, uint32_t n,
                                                                  const uint32_t* cnt, const uint32_t* doff, uint2* out) {
    const uint32_t a = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, sub = threadIdx.x & 15;
    if (a >= n || cnt[a] == 0) return;   // (a row that counted differences lies inside the arena and spells a walk)
    const uint2 res = results[a];
    const u64 o0 = offs[a];
    cs_diffs<WIDE, false>(g, arena + res.x, res.y & 0xFFFFFFu, reads + o0, (uint32_t)(offs[a + 1] - o0), ((res.y >> 24) & BGR_ST_RC) != 0, sub, out + doff[a]);
}

}  // namespace

hipError_t launch_text_gaf_sizes(const BgrDeviceGraph& g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec, const uint32_t* acc_rec, uint32_t n_acc,
                                 uint32_t* psz, uint32_t* nsz, uint32_t* nlen, uint4* rows, uint32_t* bug, const uint32_t* tag_table, uint4* tags, uint32_t* csb, hipStream_t stream) {
    if (n_acc == 0) return hipSuccess;
    if (csb) {   // the instances that carry the cs:Z: field: only an aligner with that switch on launches them
        const dim3 grid((n_acc + 15) / 16), block(256);
        if (tag_table) {
            if (g.k > 33) hipLaunchKernelGGL((bgr_text_gaf_sizes_cs_kernel<true, true>), grid, block, 0, stream, g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug, tag_table, tags, csb);
            else hipLaunchKernelGGL((bgr_text_gaf_sizes_cs_kernel<false, true>), grid, block, 0, stream, g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug, tag_table, tags, csb);
        } else {
            if (g.k > 33) hipLaunchKernelGGL((bgr_text_gaf_sizes_cs_kernel<true, false>), grid, block, 0, stream, g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug, tag_table, tags, csb);
            else hipLaunchKernelGGL((bgr_text_gaf_sizes_cs_kernel<false, false>), grid, block, 0, stream, g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug, tag_table, tags, csb);
        }
        return hipGetLastError();
    }
    if (tag_table) {   // the tagged instances: only an aligner with a tag table launches them
        if (g.k > 33) hipLaunchKernelGGL(bgr_text_gaf_sizes_tag_kernel<true>, dim3((n_acc + 15) / 16), dim3(256), 0, stream, g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug, tag_table, tags);
        else hipLaunchKernelGGL(bgr_text_gaf_sizes_tag_kernel<false>, dim3((n_acc + 15) / 16), dim3(256), 0, stream, g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug, tag_table, tags);
        return hipGetLastError();
    }
    if (g.k > 33) hipLaunchKernelGGL(bgr_text_gaf_sizes_wide_kernel, dim3((n_acc + 15) / 16), dim3(256), 0, stream, g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug);
    else hipLaunchKernelGGL(bgr_text_gaf_sizes_kernel, dim3((n_acc + 15) / 16), dim3(256), 0, stream, g, text, results, arena, rec, acc_rec, n_acc, psz, nsz, nlen, rows, bug);
    return hipGetLastError();
}

hipError_t launch_text_gaf_write(const BgrDeviceGraph& g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec, const uint32_t* acc_rec, uint32_t n_acc,
                                 const uint32_t* poff, const uint32_t* noff, const uint32_t* psz, const uint32_t* nlen, const uint4* rows, uint8_t* pout, uint8_t* nout,
                                 const uint4* tags, const uint32_t* csb, hipStream_t stream) {
    if (n_acc == 0) return hipSuccess;
    if (csb) {
        const dim3 grid((n_acc + 15) / 16), block(256);
        if (tags) {
            if (g.k > 33) hipLaunchKernelGGL((bgr_text_gaf_write_cs_kernel<true, true>), grid, block, 0, stream, g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout, tags, csb);
            else hipLaunchKernelGGL((bgr_text_gaf_write_cs_kernel<false, true>), grid, block, 0, stream, g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout, tags, csb);
        } else {
            if (g.k > 33) hipLaunchKernelGGL((bgr_text_gaf_write_cs_kernel<true, false>), grid, block, 0, stream, g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout, tags, csb);
            else hipLaunchKernelGGL((bgr_text_gaf_write_cs_kernel<false, false>), grid, block, 0, stream, g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout, tags, csb);
        }
        return hipGetLastError();
    }
    if (tags) {
        if (g.k > 33) hipLaunchKernelGGL(bgr_text_gaf_write_tag_kernel<true>, dim3((n_acc + 15) / 16), dim3(256), 0, stream, g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout, tags);
        else hipLaunchKernelGGL(bgr_text_gaf_write_tag_kernel<false>, dim3((n_acc + 15) / 16), dim3(256), 0, stream, g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout, tags);
        return hipGetLastError();
    }
    if (g.k > 33) hipLaunchKernelGGL(bgr_text_gaf_write_wide_kernel, dim3((n_acc + 15) / 16), dim3(256), 0, stream, g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout);
    else hipLaunchKernelGGL(bgr_text_gaf_write_kernel, dim3((n_acc + 15) / 16), dim3(256), 0, stream, g, text, results, arena, rec, acc_rec, n_acc, poff, noff, psz, nlen, rows, pout, nout);
    return hipGetLastError();
}

hipError_t launch_path_stats(const BgrDeviceGraph& g, const uint8_t* reads, const uint64_t* read_offs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n,
                             uint32_t* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const u64* offs = reinterpret_cast<const u64*>(read_offs);
    if (g.k > 33) hipLaunchKernelGGL(bgr_path_stats_wide_kernel, dim3((n + 15) / 16), dim3(256), 0, stream, g, reads, offs, results, arena, (u64)arena_ints, n, out);
    else hipLaunchKernelGGL(bgr_path_stats_kernel, dim3((n + 15) / 16), dim3(256), 0, stream, g, reads, offs, results, arena, (u64)arena_ints, n, out);
    return hipGetLastError();
}

hipError_t launch_path_diffs_count(const BgrDeviceGraph& g, const uint8_t* reads, const uint64_t* read_offs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n,
                                   uint32_t* cnt, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const u64* offs = reinterpret_cast<const u64*>(read_offs);
    if (g.k > 33) hipLaunchKernelGGL(bgr_path_diffs_count_kernel<true>, dim3((n + 15) / 16), dim3(256), 0, stream, g, reads, offs, results, arena, (u64)arena_ints, n, cnt);
    else hipLaunchKernelGGL(bgr_path_diffs_count_kernel<false>, dim3((n + 15) / 16), dim3(256), 0, stream, g, reads, offs, results, arena, (u64)arena_ints, n, cnt);
    return hipGetLastError();
}

hipError_t launch_path_diffs_fill(const BgrDeviceGraph& g, const uint8_t* reads, const uint64_t* read_offs, const uint2* results, const int32_t* arena, uint32_t n, const uint32_t* cnt,
                                  const uint32_t* doff, uint2* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const u64* offs = reinterpret_cast<const u64*>(read_offs);
    if (g.k > 33) hipLaunchKernelGGL(bgr_path_diffs_fill_kernel<true>, dim3((n + 15) / 16), dim3(256), 0, stream, g, reads, offs, results, arena, n, cnt, doff, out);
    else hipLaunchKernelGGL(bgr_path_diffs_fill_kernel<false>, dim3((n + 15) / 16), dim3(256), 0, stream, g, reads, offs, results, arena, n, cnt, doff, out);
    return hipGetLastError();
}

}  // namespace bgr
