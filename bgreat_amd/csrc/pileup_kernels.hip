// pileup_kernels.hip -- per-base depth and mismatches on the unitigs of a greedy / anchors launch (bgr_pileup_base, include/bgreat_gpu.h):
// behind the mapping passes one kernel reads every mapped read's row [off, id_1 .. id_n] from (results, arena), walks the path as gaf_stat does
// (walk_lanes.h: sixteen lanes share a read, lane i takes unitig i of a pass of sixteen) and then
//   depth       every occurrence j of a unitig, extent [s_j, e_j) of the walk, covers the walk positions [max(off, s_j), min(off + L, e_j)): that
//               stretch in the unitig's forward-strand positions, [a, b), costs two no-return atomics on a difference array, +1 at a and -1 at b
//               (a unitig owns len + 1 words); the depth is the running sum, taken when the table is read;
//   mismatches  lane c takes the read's characters [16 c, 16 c + 16) and compares them with the unitigs under them -- the WHOLE extent of each,
//               so the k - 1 characters two neighbours share are compared with, and counted on, both -- and every character that differs is one
//               atomic on alt[base][code] (pileup_kernels.h has the layout).
// Read position t faces base t + cst of the 2-bit store, which holds both strands of a unitig (forward at F, reverse complement at F + len):
//   read as mapped:       walk position off + t, offset x = off + t - s_j of the unitig as glued on  ->  cst = F + (st ? len : 0) + off - s_j
//   read on its rc (ST_RC): R[t] is the complement of Q[L - 1 - t]; it faces the unitig's OTHER strand at len - 1 - x, x = off + L - 1 - t - s_j
//                                                                                                   ->  cst = F + (st ? 0 : len) + len + s_j - off - L
// so a base in the forward half counts at pos = B - F with the character's own code, one in the other half at pos = F + 2 len - 1 - B with the
// complement's.  A path that spells no walk (gaf_stat's condition) adds nothing and counts in the tail word: a path of more than sixteen
// unitigs is therefore walked once before anything is added.
// Integer adds commute (mod 2^32): the table does not depend on the geometry or the order of the launches.
// Strands (bgr_aligner_pileup_strands_enable): sB, the half of the store the read runs along, is 0 exactly when the read as given in the input is
// collinear with the strand the unitig file spells (no ST_RC and glued on forward, or ST_RC and glued on reversed).  The STRANDS instances repeat
// the adds of such an occurrence into a second table of the same layout, at the same indices: the forward pileup.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "pileup_kernels.h"
#include "walk_lanes.h"

namespace bgr {
namespace {

constexpr int kSrcAscii = 0, kSrcText = 1, kSrcPlanes = 2;

}  // namespace
}  // namespace bgr

using bgr::u64;

// STRANDS: an occurrence the read runs along forward -- the read as given in the input is collinear with the strand the unitig file spells, sB == 0 --
// repeats its two delta atomics and each of its alt atomics into a second table of the same layout (alt_f, delta_f): the forward pileup of
// bgr_aligner_pileup_forward.  A compile-time constant: the instances without it are the kernel as it was.
template <bool WIDE, int SRC, bool STRANDS>
__global__ void __launch_bounds__(256) bgr_pileup_kernel(BgrDeviceGraph g, uint32_t n_unitigs, u64 total_bases, const uint2* results, const int32_t* arena, u64 arena_ints,
                                                         const u64* read_offs, uint32_t n_reads, bgr::PileupReads rd, const u64* base_offs, uint32_t* alt, uint32_t* delta,
                                                         unsigned long long* skipped, uint32_t* alt_f, uint32_t* delta_f) {
    using namespace bgr;
    const u64 alt_words = 4 * total_bases, delta_words = total_bases + n_unitigs;
    const uint32_t sub = threadIdx.x & 15, per_block = blockDim.x >> 4, stride = gridDim.x * per_block;
    for (uint32_t r = blockIdx.x * per_block + (threadIdx.x >> 4); r < n_reads; r += stride) {   // (one read per 16-lane group: the flow below is uniform in a group)
        const uint2 res = results[r];
        const uint32_t np = res.y & 0xFFFFFFu;
        if (np == 0 || (u64)res.x + np > arena_ints) continue;   // not mapped (an empty row) -- or a row that is not in the arena
        const int32_t* path = arena + res.x;
        const int32_t off_s = path[0];
        const uint32_t nu = np - 1;
        bool bad = nu == 0 || off_s < 0;
        const u64 off = (u64)(off_s < 0 ? 0 : off_s);
        if (!bad && nu > 16) {   // a long path: is it a walk, and does the read begin on it?
            WalkCarry c;
            for (uint32_t u0 = 0; u0 < nu && !bad; u0 += 16) { WalkLane w; bad = !walk_pass<WIDE>(g, path, nu, u0, sub, c, w); }
            bad = bad || off > c.total;
        }
        const u64 ro = read_offs[r];
        const uint32_t L = (uint32_t)(read_offs[r + 1] - ro);
        const bool rc = ((res.y >> 24) & BGR_ST_RC) != 0;
        const u64 hiw = off + L;
        // the read's characters
        const u64 src = SRC == kSrcText ? (u64)rd.src_off[r] : ro;
        const uint32_t wbase = (uint32_t)((ro >> 5) + r);
        const bool hasN = SRC == kSrcPlanes && ((rd.hasn[r >> 5] >> (r & 31)) & 1u);
        WalkCarry carry;
        for (uint32_t u0 = 0; u0 < nu && !bad; u0 += 16) {
            WalkLane w;
            if (!walk_pass<WIDE>(g, path, nu, u0, sub, carry, w) || (nu <= 16 && off > w.pass_end)) { bad = true; break; }
            const u64 e = w.end, s = w.end - w.len;   // the whole extent
            const u64 base = w.on ? base_offs[w.id] : 0;
            const u64 aw = off > s ? off : s, bw = hiw < e ? hiw : e;
            if (w.on && aw < bw) {
                const uint32_t xa = (uint32_t)(aw - s), xb = (uint32_t)(bw - s);
                const u64 d0 = base + w.id - 1, da = d0 + (w.st ? w.len - xb : xa), db = d0 + (w.st ? w.len - xa : xb);
                if (db < delta_words) {   // (da < db: both inside the unitig's len + 1 words)
                    atomicAdd(delta + da, 1u);
                    atomicAdd(delta + db, 0xFFFFFFFFu);
                    if (STRANDS && w.st == (rc ? 1u : 0u)) {   // (sB == 0, below)
                        atomicAdd(delta_f + da, 1u);
                        atomicAdd(delta_f + db, 0xFFFFFFFFu);
                    }
                }
            }
            // what the compare needs of lane v's unitig: its extent in read positions, cst, and where a base of the store counts
            const uint32_t sB = rc ? (w.st ^ 1u) : w.st;   // the half of the store the read runs along
            const int64_t cst = !rc ? (int64_t)(w.F + (w.st ? w.len : 0u)) + (int64_t)off - (int64_t)s
                                    : (int64_t)(w.F + (w.st ? 0u : w.len) + w.len) + (int64_t)s - (int64_t)off - (int64_t)L;
            const int64_t cnt_k = sB ? (int64_t)(base + w.F + 2ull * w.len) - 1 : (int64_t)base - (int64_t)w.F;   // base index = sB ? cnt_k - B : cnt_k + B
            int64_t ra = !rc ? (int64_t)s - (int64_t)off : (int64_t)L - ((int64_t)e - (int64_t)off);
            int64_t rb = !rc ? (int64_t)e - (int64_t)off : (int64_t)L - ((int64_t)s - (int64_t)off);
            ra = ra < 0 ? 0 : ra; rb = rb > (int64_t)L ? (int64_t)L : rb;
            if (!w.on || ra > rb) { ra = 0; rb = 0; }
            const uint32_t ext_a = (uint32_t)ra, ext_b = (uint32_t)rb;
            const u64 first_s = grp_get64(s, 0);
            const u64 lo = first_s > off ? first_s : off, hi = w.pass_end < hiw ? w.pass_end : hiw;   // walk positions of this pass that lie under the read
            if (lo < hi) {
                const uint32_t tlo = !rc ? (uint32_t)(lo - off) : L - (uint32_t)(hi - off), thi = !rc ? (uint32_t)(hi - off) : L - (uint32_t)(lo - off);
                const uint32_t cnt = w.last + 1;
                for (uint32_t c0 = tlo >> 4; 16 * (u64)c0 < thi; c0 += 16) {   // (every lane takes every turn: the shuffles below need them all)
                    const uint32_t t0 = 16 * (c0 + sub);
                    const bool mine = t0 < thi;
                    const uint32_t ca = tlo > t0 ? tlo : t0, cb = thi < t0 + 16 ? thi : t0 + 16;   // the read positions [ca, cb) of these 16
                    uint32_t ch[4] = {0, 0, 0, 0};
                    uint32_t rcodes = 0, nm2 = 0;   // planes: character i at bits 31 - 2 i, 30 - 2 i; 3 on every N
                    if (mine) {
                        if (SRC == kSrcPlanes) {
                            const u64 fw = rd.fw3[wbase + (t0 >> 5)];
                            rcodes = (t0 & 16) ? (uint32_t)fw : (uint32_t)(fw >> 32);
                            if (hasN) { const u64 nw = rd.nmw[wbase + (t0 >> 5)]; nm2 = (t0 & 16) ? (uint32_t)nw : (uint32_t)(nw >> 32); }
                        } else {
                            const u64 left = rd.ascii_bytes - (src + t0);   // (bytes of the buffer, not of the read: what lies behind the read is masked out)
                            load16p<false>(rd.ascii + src + t0, left < 16 ? (uint32_t)left : 16u, ch);
                        }
                    }
                    for (uint32_t v = 0; v < cnt; ++v) {
                        const uint32_t va = (uint32_t)__shfl((int)ext_a, (int)v, 16), vb = (uint32_t)__shfl((int)ext_b, (int)v, 16);
                        const uint32_t vS = (uint32_t)__shfl((int)sB, (int)v, 16);
                        const int64_t cv = (int64_t)grp_get64((u64)cst, v), kv = (int64_t)grp_get64((u64)cnt_k, v);
                        const uint32_t xa = va > ca ? va : ca, xb = vb < cb ? vb : cb;
                        if (mine && xa < xb) {
                            const uint32_t a = xa - t0, b = xb - t0;
                            const uint32_t codes = (uint32_t)(win32(g.seq, (u64)((int64_t)xa + cv)) >> 32) >> (2 * a);   // base of character i at bits 31 - 2 i, 30 - 2 i
                            uint32_t mis;   // bit i: character i differs
                            if (SRC == kSrcPlanes) {
                                const uint32_t x = (rcodes ^ codes) | nm2;
                                uint32_t m2 = (x | (x >> 1)) & 0x55555555u, m = 0;
#pragma unroll
                                for (int i = 0; i < 16; ++i) m |= ((m2 >> (30 - 2 * i)) & 1u) << i;
                                mis = m;
                            } else {
                                mis = ~eq16_acgt(ch, codes);
                            }
                            mis &= ((b < 32 ? (1u << b) : 0u) - 1u) & ~((1u << a) - 1u) & 0xFFFFu;
                            while (mis) {
                                const uint32_t i = (uint32_t)__ffs((int)mis) - 1;
                                mis &= mis - 1;
                                const uint32_t sc = (codes >> (30 - 2 * i)) & 3u;   // the store's base, the unitig's own on its forward strand
                                const uint32_t ref = vS ? 3u - sc : sc;
                                uint32_t code;   // the read's character on the unitig's forward strand; 4 = outside ACGT
                                if (SRC == kSrcPlanes) {
                                    const uint32_t q = (rcodes >> (30 - 2 * i)) & 3u;
                                    code = ((nm2 >> (30 - 2 * i)) & 1u) ? 4u : (vS ? 3u - q : q);
                                } else {
                                    const uint32_t c = (ch[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                                    const uint32_t q = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
                                    code = q == 4u ? 4u : (vS ? 3u - q : q);
                                }
                                const int64_t B = (int64_t)(t0 + i) + cv;
                                const u64 idx = 4 * (u64)(vS ? kv - B : kv + B) + (code == 4u ? ref : code);
                                if (idx < alt_words) {
                                    atomicAdd(alt + idx, 1u);
                                    if (STRANDS && !vS) atomicAdd(alt_f + idx, 1u);
                                }
                            }
                        }
                    }
                }
            }
        }
        if (bad && sub == 0) atomicAdd(skipped, 1ull);
    }
}

namespace bgr {

template <bool WIDE, bool STRANDS>
static void launch_src(int src, uint32_t blocks, hipStream_t stream, const BgrDeviceGraph& g, uint32_t nu, uint64_t total_bases, const uint2* results, const int32_t* arena,
                       uint64_t arena_ints, const uint64_t* read_offs, uint32_t n_reads, const PileupReads& rd, const uint64_t* base_offs, uint32_t* alt, uint32_t* delta,
                       unsigned long long* skipped, uint32_t* alt_f, uint32_t* delta_f) {
    const u64* ro = reinterpret_cast<const u64*>(read_offs);
    const u64* bo = reinterpret_cast<const u64*>(base_offs);
    if (src == kSrcAscii)
        hipLaunchKernelGGL((bgr_pileup_kernel<WIDE, kSrcAscii, STRANDS>), dim3(blocks), dim3(256), 0, stream, g, nu, (u64)total_bases, results, arena, (u64)arena_ints, ro, n_reads, rd, bo, alt, delta, skipped, alt_f, delta_f);
    else if (src == kSrcText)
        hipLaunchKernelGGL((bgr_pileup_kernel<WIDE, kSrcText, STRANDS>), dim3(blocks), dim3(256), 0, stream, g, nu, (u64)total_bases, results, arena, (u64)arena_ints, ro, n_reads, rd, bo, alt, delta, skipped, alt_f, delta_f);
    else
        hipLaunchKernelGGL((bgr_pileup_kernel<WIDE, kSrcPlanes, STRANDS>), dim3(blocks), dim3(256), 0, stream, g, nu, (u64)total_bases, results, arena, (u64)arena_ints, ro, n_reads, rd, bo, alt, delta, skipped, alt_f, delta_f);
}

hipError_t launch_pileup(const BgrDeviceGraph& g, uint64_t n_unitigs, uint64_t total_bases, const uint2* results, const int32_t* arena, uint64_t arena_ints,
                         const uint64_t* read_offs, uint32_t n_reads, const PileupReads& reads, const uint64_t* base_offs, uint32_t* table, uint32_t* table_fwd, uint32_t num_cus,
                         hipStream_t stream) {
    if (n_reads == 0) return hipSuccess;
    if (n_unitigs >= 0x40000000ull || !table || !base_offs || !read_offs) return hipErrorInvalidValue;
    if (!reads.ascii && !(reads.fw3 && reads.nmw && reads.hasn)) return hipErrorInvalidValue;
    const int src = reads.ascii ? (reads.src_off ? kSrcText : kSrcAscii) : kSrcPlanes;
    if (!num_cus) num_cus = 256;
    const uint64_t groups = 256 / kPileupLanes;   // a grid-stride loop over the reads, sixteen per workgroup and turn
    uint64_t blocks = (n_reads + groups - 1) / groups;
    if (blocks > (uint64_t)num_cus * 64) blocks = (uint64_t)num_cus * 64;
    uint32_t* alt = table;
    uint32_t* delta = table + pileup_alt_words(total_bases);
    unsigned long long* skipped = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(table) + pileup_tail_byte(total_bases, n_unitigs));
    uint32_t* alt_f = table_fwd;   // (null: the kernel without the second table)
    uint32_t* delta_f = table_fwd ? table_fwd + pileup_alt_words(total_bases) : nullptr;
#define BGR_PILEUP_LAUNCH(W, S) launch_src<W, S>(src, (uint32_t)blocks, stream, g, (uint32_t)n_unitigs, total_bases, results, arena, arena_ints, read_offs, n_reads, reads, base_offs, alt, delta, skipped, alt_f, delta_f)
    if (g.k > 33) { if (table_fwd) BGR_PILEUP_LAUNCH(true, true); else BGR_PILEUP_LAUNCH(true, false); }
    else { if (table_fwd) BGR_PILEUP_LAUNCH(false, true); else BGR_PILEUP_LAUNCH(false, false); }
#undef BGR_PILEUP_LAUNCH
    return hipGetLastError();
}

}  // namespace bgr
