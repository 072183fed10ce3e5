// inside_kernels.hip -- the fallback pass of greedy mode: reads that lie wholly inside one unitig hold no overlap (k-1)-mer, so the mapping passes
// leave them with status NOANCHOR.  Behind those passes one kernel visits every such read with sixteen lanes (four reads per wave):
//   stage    the read's 2-bit words and its N words into LDS, from wherever the launch has its characters (PileupReads: ASCII end to end, ASCII
//            scattered in a text piece, or the 2-bit planes);
//   probe    per round of sixteen windows lane i takes window i0 + i: its k-mer word, the canonical form, m = bgr_mix64 -- and only a window
//            the hash selects (one in four) and that holds no N goes to the table (inside_index.h: linear probing over 16-byte entries, the
//            key compared).  The four reads of a wave and the lanes of each keep their probes in flight side by side;
//   verify   the hits of the round in window order (a ballot inside the sixteen), each a diagonal (unitig, strand, start s): skipped when it
//            is the diagonal tested last or the read would hang over an end, else the lanes compare the read with the unitig's strand in the
//            2-bit store, 32 bases per lane and turn -- XOR, fold the bit pairs, OR the N word in, popcount, a DPP sum over the sixteen.  Both
//            strands of a unitig are stored, so nothing is reversed.  The first diagonal with at most max_mismatch differences decides;
//   write    the row [s, +-id]: the workgroup sums what its reads need and takes it with ONE atomic on cursor[0] per turn (a read-by-read
//            atomic on one address would cost more than the pass), each read then writes its two ints and its result word.
// The launch runs over all reads and leaves at the status word: the reads are in no list, and on a graph of short unitigs one read in seven
// takes the pass.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "inside_kernels.h"

namespace bgr {
namespace {

constexpr int kSrcAscii = 0, kSrcText = 1, kSrcPlanes = 2;

}  // namespace
}  // namespace bgr

using bgr::u64;

template <int SRC>
__global__ void __launch_bounds__(256) bgr_align_inside_kernel(BgrDeviceGraph g, const BgrInsideEntry* tab, u64 slots, bgr::InsideLaunch io, unsigned long long* count, uint32_t W) {
    using namespace bgr;
    extern __shared__ u64 lds[];
    __shared__ uint32_t s_n, s_base;
    const uint32_t sub = threadIdx.x & 15, grp = threadIdx.x >> 4, per_block = blockDim.x >> 4, row = threadIdx.x & 48;
    u64* FW = lds + (size_t)grp * 2 * W;   // W words each: the read's, then a zero word
    u64* NM = FW + W;
    const uint32_t k = g.k, sh = 64 - 2 * k;
    for (uint32_t base = blockIdx.x * per_block; base < io.n_reads; base += gridDim.x * per_block) {   // (uniform in the workgroup: the barriers below)
        if (threadIdx.x == 0) s_n = 0;
        const uint32_t r = base + grp;
        bool active = r < io.n_reads;
        if (active) active = ((io.results[r].y >> 24) & BGR_ST_MASK) == BGR_ST_NOANCHOR;
        u64 ro = 0;
        uint32_t L = 0;
        if (active) {
            ro = io.read_offs[r];
            const u64 L64 = io.read_offs[r + 1] - ro;
            L = (uint32_t)L64;
            active = L64 >= k && ((L64 + 31) >> 5) < W;
        }
        if (active) {
            const uint32_t Wr = (L + 31) >> 5;
            const u64 src = SRC == kSrcText ? (u64)io.reads.src_off[r] : ro;
            const uint32_t wbase = (uint32_t)((ro >> 5) + r);
            const bool hasN = SRC == kSrcPlanes && ((io.reads.hasn[r >> 5] >> (r & 31)) & 1u);
            for (uint32_t j = sub; j <= Wr; j += 16) {
                u64 f = 0, nm = 0;
                if (j < Wr) {
                    if (SRC == kSrcPlanes) {
                        f = io.reads.fw3[wbase + j];
                        if (hasN) nm = io.reads.nmw[wbase + j];
                    } else {
                        uint32_t chars = 0;
                        f = ascii_word(io.reads.ascii, src + 32ull * j, L - 32 * j, io.reads.ascii_bytes, &chars);
                        if (chars & 0x08080808u) nm = ascii_nmask_word(io.reads.ascii, src + 32ull * j, L - 32 * j, io.reads.ascii_bytes);
                    }
                }
                FW[j] = f;
                NM[j] = nm;
            }
        }
        __syncthreads();
        bool found = false;
        int32_t row_s = 0, row_id = 0;
        if (active) {
            const uint32_t nwin = L - k + 1;
            uint32_t last_id = 0, last_fwd = 0;
            int64_t last_s = -1;
            for (uint32_t i0 = 0; i0 < nwin && !found; i0 += 16) {
                const uint32_t i = i0 + sub;
                u64 val = 0;
                uint32_t wcanon = 0;
                bool hit = false;
                if (i < nwin && (lds_win32(NM, i) >> sh) == 0) {
                    const u64 x = lds_win32(FW, i) >> sh, rc = rcb_fast(x, k);
                    const u64 c = x < rc ? x : rc, m = bgr_mix64(c);
                    if (x != rc && bgr_jump_selects(m)) {
                        wcanon = x < rc ? 1u : 0u;
                        for (u64 s = bgr_inside_slot(m, slots);; s = s + 1 == slots ? 0 : s + 1) {   // (ends: the table is at most half full)
                            const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(tab + s);
                            if (e.x == c) { hit = true; val = e.y; break; }
                            if (e.x == BGR_EMPTY_KEY) break;
                        }
                    }
                }
                uint32_t hits = (uint32_t)(__builtin_amdgcn_ballot_w64(hit) >> row) & 0xFFFFu;
                while (hits && !found) {
                    const uint32_t hl = (uint32_t)__ffs((int)hits) - 1;
                    hits &= hits - 1;
                    const u64 v = ((u64)(uint32_t)__shfl((int)(val >> 32), (int)hl, 16) << 32) | (uint32_t)__shfl((int)val, (int)hl, 16);
                    const uint32_t wc = (uint32_t)__shfl((int)wcanon, (int)hl, 16);
                    const uint32_t id = bgr_inside_id(v), j = bgr_inside_off(v), fwd = wc == (uint32_t)(v & BGR_INSIDE_FWD_CANON) ? 1u : 0u;
                    const u64 len = g.meta[id].len, F = g.meta[id].F;
                    // the window lies at j of the forward strand, at len - k - j of the other: the read starts i0 + hl characters before it
                    const int64_t s = (fwd ? (int64_t)j : (int64_t)len - (int64_t)k - (int64_t)j) - (int64_t)(i0 + hl);
                    if (s < 0 || (u64)s + L > len) continue;
                    if (id == last_id && s == last_s && fwd == last_fwd) continue;
                    last_id = id; last_s = s; last_fwd = fwd;
                    const u64 B = F + (fwd ? 0 : len) + (u64)s;
                    uint32_t cnt = 0;
                    for (uint32_t t = 32 * sub; t < L; t += 512) {
                        const uint32_t n = L - t < 32 ? L - t : 32;
                        const u64 x = (FW[t >> 5] ^ win32(g.seq, B + t)) | NM[t >> 5];
                        u64 d = (x | (x >> 1)) & EVEN_BITS;
                        if (n < 32) d &= ~0ULL << (64 - 2 * n);
                        cnt += (uint32_t)__popcll(d);
                    }
                    cnt = row16_sum(cnt);
                    if (cnt <= io.max_mismatch) { found = true; row_s = (int32_t)s; row_id = fwd ? (int32_t)id : -(int32_t)id; }
                }
            }
        }
        uint32_t mine = 0;
        if (found && sub == 0) mine = atomicAdd(&s_n, 1u);
        __syncthreads();
        if (threadIdx.x == 0 && s_n) {
            s_base = atomicAdd(io.cursor + kCurArena, 2 * s_n);
            atomicAdd(count, (unsigned long long)s_n);
        }
        __syncthreads();
        if (found && sub == 0) {
            const u64 at = (u64)io.arena_own + s_base + 2 * mine;
            if (at + 2 <= io.arena_cap) {
                io.arena[at] = row_s;
                io.arena[at + 1] = row_id;
                io.results[r] = make_uint2((uint32_t)at, 2u | ((uint32_t)BGR_ST_ALIGNED << 24));
            } else {
                io.cursor[kCurOverflow] = 1;   // reported by the host as an error
            }
        }
        __syncthreads();
    }
}

namespace bgr {

hipError_t launch_inside(const BgrDeviceGraph& g, const BgrInsideEntry* table, uint64_t slots, const InsideLaunch& io, unsigned long long* count, uint32_t num_cus,
                         hipStream_t stream) {
    if (io.n_reads == 0) return hipSuccess;
    if (!table || !slots || !count || !io.results || !io.arena || !io.cursor || !io.read_offs || g.k > BGR_NARROW_MAX_K || io.max_read_len > kInsideMaxReadLen) return hipErrorInvalidValue;
    if (!io.reads.ascii && !(io.reads.fw3 && io.reads.nmw && io.reads.hasn)) return hipErrorInvalidValue;
    const int src = io.reads.ascii ? (io.reads.src_off ? kSrcText : kSrcAscii) : kSrcPlanes;
    if (!num_cus) num_cus = 256;
    const uint32_t W = io.max_read_len / 32 + 2;
    const uint32_t threads = 256u * W <= 65536u ? 256u : 64u;   // sixteen reads per workgroup while their words fit 64 KiB of LDS, else four
    const uint32_t groups = threads / kInsideLanes, lds_bytes = groups * 2 * W * 8;
    uint64_t blocks = ((uint64_t)io.n_reads + groups - 1) / groups;
    if (blocks > (uint64_t)num_cus * 32) blocks = (uint64_t)num_cus * 32;
    if (src == kSrcAscii)
        hipLaunchKernelGGL((bgr_align_inside_kernel<kSrcAscii>), dim3((uint32_t)blocks), dim3(threads), lds_bytes, stream, g, table, (u64)slots, io, count, W);
    else if (src == kSrcText)
        hipLaunchKernelGGL((bgr_align_inside_kernel<kSrcText>), dim3((uint32_t)blocks), dim3(threads), lds_bytes, stream, g, table, (u64)slots, io, count, W);
    else
        hipLaunchKernelGGL((bgr_align_inside_kernel<kSrcPlanes>), dim3((uint32_t)blocks), dim3(threads), lds_bytes, stream, g, table, (u64)slots, io, count, W);
    return hipGetLastError();
}

}  // namespace bgr
