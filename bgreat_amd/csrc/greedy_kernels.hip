// greedy_kernels.hip -- greedy mode (alignReadGreedy, alignerGreedy.cpp:35-57,167-364) on gfx950.
//   bgr_align_greedy_multi_kernel  sixteen reads per wavefront (lanes per read: a template parameter): the position scans two at a time on
//                             32 lanes each (key table in LDS; else one at a time on all 64 lanes), the extensions side by side, 4 lanes each
//                             (both walks of an anchor at once); settles the common shapes, lists the rest
//   bgr_align_greedy_kernel   the general kernel: one read per wavefront, every anchor, both strands, N planes, any path length
//   bgr_align_greedy_wide_kernel  the same over two-word overlap keys (graphs with k > 32, or built under test.wide_keys); only the
//                             position scan and the anchor's key differ, the walk is the same
#include "device_common.h"
#include "scan_take_word.h"

namespace bgr {
namespace {

// The general kernel's body.  WIDE: the graph's keys are two words (graph_layout.h BgrKeyEntryWide): the scan builds each window's
// (k-1)-mer as (hi, lo), its reverse complement with rcb_wide, and looks it up with find_key_wide; no filter in front of the table.
template <bool STAGE, bool WIDE>
__device__ __forceinline__ void greedy_general(const BgrDeviceGraph& g, const BatchIO& io, const KernelParams& prm) {
    extern __shared__ u64 lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    const uint32_t W = io.words_per_read;
    const uint32_t K1 = g.k - 1;
    // as the second pass behind bgr_align_greedy_multi_kernel it maps only the reads that kernel listed (count in cursor[subset_ctr])
    const uint32_t total = io.subset ? io.cursor[io.subset_ctr] : io.n_reads;
    if ((uint32_t)(blockIdx.x * waves) >= total) return;  // nothing for this workgroup (before it copies the cascade into LDS)
    uint32_t ktab_words;
    const uint32_t* ktab = block_prologue<STAGE>(g, lds, &ktab_words);
    const uint32_t per_wave_words = 4 * W + io.path_cap / 2;
    u64* FW3 = lds + 64 + ktab_words + (u64)wave * per_wave_words;
    u64* FWQ = FW3 + W;
    u64* RCW = FWQ + W;
    u64* NM = RCW + W;
    int32_t* PATH = reinterpret_cast<int32_t*>(NM + W);

    uint32_t c_lane = 0;                    // per-lane status counter (a VGPR: the kernel is short of SGPRs, not of VGPRs)
    uint32_t chunk_pos = 0, chunk_end = 0;  // this wave's slice of the path arena
    // getNOverlap(read, 0) still looks at position 0 before testing the count (aligner.cpp:349-368)
    const uint32_t effort = prm.effort ? prm.effort : 1;

    for (uint32_t it = blockIdx.x * waves + wave; it < total; it += gridDim.x * waves) {
        const uint32_t r = io.subset ? io.subset[it] : it;
        const u64 off = io.read_offs[r];
        const uint32_t L = (uint32_t)(io.read_offs[r + 1] - off);
        // (prefetching the next read one iteration ahead was measured: no gain at 24 waves/CU, it only added spills)
        const bool hasN = load_packed(io, r, off, L, W, FW3, NM, lane);
        bool derived = false;

        // ---- passes: forward read, then its reverse complement (alignerGreedy.cpp:54) -----------
        uint32_t status = BGR_ST_NOANCHOR, p_lo = 0, p_n = 0;
        uint32_t npos = L >= K1 ? L - K1 + 1 : 0;
        if (!prm.effort && npos > 1) npos = 1;
#ifdef BGR_PHASE_TIMING  /* diagnostic builds: env BGR_DEBUG_STOP = 1 stops after packing, 2 after the position scan */
        if (prm.debug_stop == 1) npos = 0;
#endif
        // (minimizer filter in front of a key table that is not staged: a scan step covers 65 - w positions, device_common.h)
        const uint32_t mmx_w = (!WIDE && !STAGE && g.bloom && g.filter_kind == BGR_FILTER_MINIMIZER) ? K1 + 1 - BGR_MMX_BASES : 0u;
        const uint32_t scan_step = mmx_w ? 65 - mmx_w : 64;
        for (int pass = 0; pass < 2; ++pass) {
            if ((pass == 1 || hasN) && !derived) { derive_streams(L, W, K1, FW3, FWQ, RCW, NM, lane); derived = true; }
            // A read without N: FWQ == FW3 and the rolling reverse k-mer == rcb(forward k-mer), so pass 0 needs FW3 only.
            const bool plain = (pass == 0) && !hasN;
            const u64* A = pass ? RCW : (plain ? FW3 : FWQ);   // forward-strand k-mers of this pass
            const u64* B = pass ? FW3 : RCW;                   // reverse-strand k-mers (rolling nuc2intrc: N -> 0)
            const u64* CMP = pass ? RCW : FW3;                 // characters compared by missmatchNumber
            const bool useN = (pass == 0) && hasN;
            uint32_t tried = 0;
            bool done = false;
            for (uint32_t base = 0; base < npos && !done && tried < effort; base += scan_step) {
                const uint32_t i = base + lane;
                const bool valid = i < npos && (uint32_t)lane < scan_step;
                uint32_t idx;
                if constexpr (WIDE) {  // the window's (k-1)-mer and the rolling reverse one as (hi, lo); the smaller is looked up
                    u64 nh = 0, nl = 0, rh = 0, rl = 0;
                    if (valid) {
                        lds_key_wide(A, i, K1, &nh, &nl);
                        if (plain) rcb_wide(nh, nl, K1, &rh, &rl);
                        else lds_key_wide(B, L - K1 - i, K1, &rh, &rl);
                    }
                    const bool fw = key_lt_wide(nh, nl, rh, rl);
                    idx = find_key_wide<!STAGE>(g, ktab, fw ? nh : rh, fw ? nl : rl, valid);
                } else {
                u64 num = 0, rcn = 0, win = 0;
                if (valid || (mmx_w && i + BGR_MMX_BASES <= L)) win = lds_win32(A, i);
                if (valid) {
                    num = win >> (64 - 2 * K1);
                    rcn = plain ? rcb_fast(num, K1) : lds_win32(B, L - K1 - i) >> (64 - 2 * K1);
                }
                const u64 rep = num < rcn ? num : rcn;
                uint32_t mblock = 0;
                if (!STAGE && mmx_w) {  // (a read with an N: the key looked up need not be the canonical form of the window -- its own 16-mers then)
                    mblock = plain ? scan_mblock(g, win, i + BGR_MMX_BASES <= L, mmx_w) : bgr_mmx_block(bgr_mmx_of_key(rep, K1), g.bloom_mask);
                }
                idx = find_key<!STAGE>(g, ktab, rep, valid, mblock);
                }
                u64 mask = __ballot(idx != BGR_NONE);
#ifdef BGR_PHASE_TIMING
                if (prm.debug_stop == 2) { if (mask) { ++tried; done = true; p_n = 0; } mask = 0; }
#endif
                while (mask && tried < effort) {
                    const int src = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    ++tried;
                    // the anchor's k-mers are re-read from LDS (uniform) rather than kept in two 64-bit VGPRs across the walk
                    const uint32_t a_pos = base + (uint32_t)src;
                    uint32_t a_rec;
                    bool a_canon;
                    if constexpr (WIDE) {
                        u64 nh, nl, rh, rl, ch, cl;
                        lds_key_wide(A, a_pos, K1, &nh, &nl);
                        nh = rl64(nh, 0); nl = rl64(nl, 0);
                        if (plain) rcb_wide(nh, nl, K1, &rh, &rl);
                        else { lds_key_wide(B, L - K1 - a_pos, K1, &rh, &rl); rh = rl64(rh, 0); rl = rl64(rl, 0); }
                        a_rec = rl32(idx, src);
                        rcb_wide(nh, nl, K1, &ch, &cl);  // getBegin/getEnd's own rcb (aligner.cpp:149,211), as below
                        if (ch != rh || cl != rl) {
                            const bool fw = key_lt_wide(nh, nl, ch, cl);
                            a_rec = find_key_wide<!STAGE>(g, ktab, fw ? nh : ch, fw ? nl : cl, true);
                        }
                        a_canon = !key_lt_wide(ch, cl, nh, nl);
                        if (a_rec != BGR_NONE) a_rec *= 2;  // (wide entry s: its handles are BgrKeyEntry 2 s, what the walk's half_handle reads)
                    } else {
                    const u64 a_num = rl64(lds_win32(A, a_pos) >> (64 - 2 * K1), 0);
                    const u64 a_rcn = plain ? rcb_fast(a_num, K1) : rl64(lds_win32(B, L - K1 - a_pos) >> (64 - 2 * K1), 0);
                    a_rec = rl32(idx, src);
                    // getBegin/getEnd recompute rc = rcb(num) (aligner.cpp:149,211); it differs from the
                    // rolling rcnum only when an N was rolled into the window.
                    const u64 rc2 = rcb_fast(a_num, K1);
                    if (rc2 != a_rcn) {
                        const u64 key2 = a_num < rc2 ? a_num : rc2;
                        a_rec = find_key<!STAGE>(g, ktab, key2, true, (!STAGE && mmx_w) ? bgr_mmx_block(bgr_mmx_of_key(key2, K1), g.bloom_mask) : 0u);
                    }
                    a_canon = a_num <= rc2;
                    }
                    if (greedy_from_anchor(g, CMP, NM, useN, L, K1, a_rec, a_canon, a_pos, prm.max_mismatch, PATH, &p_lo, &p_n, lane)) {
                        done = true;
                        break;
                    }
                }
            }
            if (done) { status = BGR_ST_ALIGNED | (pass ? BGR_ST_RC : 0); break; }
            if (tried == 0) { status = BGR_ST_NOANCHOR | (pass ? BGR_ST_RC : 0); break; }  // ++noOverlapRead, no retry
            status = BGR_ST_FAILED | BGR_ST_RC;  // all anchors failed: retry on the reverse complement once
        }
        // ---- stage D: publish ---------------------------------------------------------------------
        wave_sync();
        uint32_t abase = 0;
        if ((status & BGR_ST_MASK) == BGR_ST_ALIGNED) abase = publish_path(io, PATH, p_lo, p_n, &chunk_pos, &chunk_end, lane);
        else p_n = 0;
        if (lane == 0) io.results[r] = make_uint2(abase, p_n | (status << 24));
        c_lane += (uint32_t)lane == (status & BGR_ST_MASK);  // lane s counts the reads that ended with status s
        wave_sync();
    }
    {   // aligner.h:68 counters: [0] readNumber [1] noOverlapRead [2] alignedRead [3] notAligned
        unsigned long long* counters = reinterpret_cast<unsigned long long*>(io.cursor + kCurCounters);
        const uint32_t total = rl32(c_lane, BGR_ST_NOANCHOR) + rl32(c_lane, BGR_ST_FAILED) + rl32(c_lane, BGR_ST_ALIGNED);
        if (lane == 0 && total) atomicAdd(&counters[0], (unsigned long long)total);
        if (lane == BGR_ST_NOANCHOR && c_lane) atomicAdd(&counters[1], (unsigned long long)c_lane);
        if (lane == BGR_ST_ALIGNED && c_lane) atomicAdd(&counters[2], (unsigned long long)c_lane);
        if (lane == BGR_ST_FAILED && c_lane) atomicAdd(&counters[3], (unsigned long long)c_lane);
    }
}

template <bool STAGE>
__global__ void __launch_bounds__(1024, BGR_GREEDY_OCC) bgr_align_greedy_kernel(BgrDeviceGraph g, BatchIO io, KernelParams prm) {
    greedy_general<STAGE, false>(g, io, prm);
}
// (its own name: the one-word kernel's mangled and profiler names stay as they were)
template <bool STAGE>
__global__ void __launch_bounds__(1024, BGR_GREEDY_OCC) bgr_align_greedy_wide_kernel(BgrDeviceGraph g, BatchIO io, KernelParams prm) {
    greedy_general<STAGE, true>(g, io, prm);
}

// ================================= greedy, several reads per wavefront ====================================
// bgr_align_greedy_kernel above walks one read per wave: a walk step is two dependent loads (slot, bases) scored by at
// most 4 candidates x a few 32-base chunks, i.e. a handful of the 64 lanes, and per read there are ~3 such steps in a row.
// Here a wave takes 64 / GL reads, GL lanes each (GL = 4: SIXTEEN reads; round 2 started with GL = 16, four reads, and ended with 8):
// their position scans still run one after the other on all 64 lanes (a scan is lane-efficient: one (k-1)-mer per lane), then
// the extensions run side by side, GL lanes each (at GL = 4: the left walk on lanes 0-1, the right walk on lanes 2-3, one lane per
// candidate slot; g2_step), so thirty-two slot/base load chains are in flight per wave and every wave instruction of a walk step serves
// sixteen reads (a quad of reads needs max-over-4 = 3.4 steps, an octet 3.7: the instructions per read nearly halve
// with every doubling).  Path ints go straight into the read's own row of the arena (kG4PathInts ints: left walk downwards from the
// middle, right walk upwards), so there are no path registers, no per-wave arena chunks and no copy when a walk ends.
//
// The reference's retry ladder (alignerGreedy.cpp:41-56: the next anchors of getNOverlap's list, then once the reverse
// complement) runs INSIDE the launch (round 3; round 2 re-launched the kernel twice over lists): an ITEM is one strand of
// one read from one scan position on.  A wave first takes its share of the batch (items = whole reads, forward strand, position
// 0); an item whose anchors fail leaves a follow-up item -- the same strand from behind the anchor tried last, or the reverse
// complement from its first position -- in the wave's own queue (a ring in HBM, written and read by this wave only), and once
// the wave's share of the batch is done it works its queue off in dense groups until nothing is left.  A reverse-complement item
// stages reverseComplements(read) (utils.cpp:66-73) as its words, so both strands run the same code.  What the kernel does not
// take at all -- N in the read, more than kG4PathInts / 2 path ints per direction, reads of a mixed batch that are too long for one lane per
// word -- goes on a list for bgr_align_greedy_kernel, which maps those reads from scratch right behind.
#ifndef BGR_G4_OCC
#define BGR_G4_OCC 8
#endif

// where an item stands: which strand (the reference maps the reverse complement once every forward anchor has failed,
// alignerGreedy.cpp:54), how many anchors of that strand have been tried (getNOverlap hands out the first `effort` of them)
// and the position the scan resumes from
#define G4_ST_RC (1u << 31)
#define G4_ST_TRIED_SHIFT 20
#define G4_ST_POS_MASK 0xFFFFFu

// GL = lanes per read (kG4GroupLanes, align_kernels.h): 16 = four reads per wave, 8 = eight, 4 = sixteen.
// The walk step is g2_step: g4_step's lean form (no exception-plane code) on two lanes, the left and the right walk of a read on the two
// pairs of its quad (so GL = 4 only).  The launch planner sends a graph with unitig bases outside ACGT (BGR_GF_HAS_EXC) to
// bgr_align_greedy_kernel only (launch_plan.h, fast_pass).
template <bool STAGE, int GL, bool ASCII>
__global__ void __launch_bounds__(1024, BGR_G4_OCC) bgr_align_greedy_multi_kernel(BgrDeviceGraph g, BatchIO io, KernelParams prm) {
    static_assert(GL == 4, "the two-pair walk takes four lanes per read");
    constexpr uint32_t RPW = 64 / GL;  // reads per wave
    extern __shared__ u64 lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    const uint32_t W = io.words_per_read;  // <= 16 (set by the host): one lane per word of a read
    const uint32_t K1 = g.k - 1;
    const uint32_t total = io.n_reads;
    if ((uint32_t)(blockIdx.x * waves) * RPW >= total) return;  // nothing for this workgroup (before it copies the key table into LDS)
    // the workgroup's counts of settled reads: four words at the start of the LDS (summed into HBM once per workgroup at the end: one
    // global atomic per wave and counter, all on the same four addresses, cost a launch of 131 k reads a third of its time)
    uint32_t* wg_counts = reinterpret_cast<uint32_t*>(lds);
    if (threadIdx.x < 4) wg_counts[threadIdx.x] = 0;
    task_stock_init(lds, (total + RPW - 1) / RPW);
#ifdef BGR_PHASE_TIMING  /* tools/wave_times.sh: when does a wave start, have its table, finish its share of the batch, finish its queue */
    const unsigned long long wt0 = wall_clock64();
    unsigned long long wt2 = 0;
    uint32_t dbg_steps = 0, dbg_items = 0, dbg_groups = 0;  // tools/scan_steps.py: scan steps, items scanned, groups of items taken
    uint32_t dbg_jumped = 0, dbg_raised = 0;                // items the jump settled without a scan step, items whose resume position it raised
    uint32_t dbg_far = 0, dbg_bounded = 0;                  // of the settled ones: by the far entry; items left a range the jump cut at either end
#endif
    uint32_t ktab_words;
    const uint32_t* ktab = block_prologue<STAGE>(g, lds, &ktab_words);
#ifdef BGR_PHASE_TIMING
    const unsigned long long wt1 = wall_clock64();
#endif
    u64* RD = lds + 64 + ktab_words + (u64)wave * (RPW * W);
    const uint32_t grp = (uint32_t)lane / GL, sub = (uint32_t)lane % GL;
    const uint32_t m = prm.max_mismatch;
    const uint32_t eff = prm.effort ? prm.effort : 1;  // getNOverlap(read, 0) still takes a hit at position 0 (aligner.cpp:349-368)
    // (minimizer filter in front of a key table that is not staged: a scan step covers 65 - w positions, device_common.h)
    const uint32_t mmx_w = (!STAGE && g.bloom && g.filter_kind == BGR_FILTER_MINIMIZER) ? K1 + 1 - BGR_MMX_BASES : 0u;
    const bool wide_scan = io.wide_scan && mmx_w && scan_mblock_is_wide(mmx_w);   // (k = 31 / 32: the filter block in all 64 lanes, scan_mblock_wide)
    const uint32_t scan_step = (mmx_w && !wide_scan) ? 65 - mmx_w : 64;

    // Path ints go straight into the arena: read r owns the row arena[r * kG4PathInts ...] (the host keeps n_reads rows in front of the
    // chunks the cursor serves to the other kernels).  Left int number i (near -> far, offset last) at row[PH - 1 - i], right int number
    // i at row[PH + i], so reverse(left) ++ right is the slice row[PH - nl, PH + nr) -- no allocation, no copy when a walk ends.
    const uint32_t wid = (uint32_t)(blockIdx.x * waves + wave);
    // this wave's queue of follow-up items {read, state}: a ring of io.q_cap (>= 2 RPW) entries in HBM, written and read by this wave only.
    // A wave takes a dense group of RPW items off its queue as soon as it holds that many, else its next task of fresh reads (claim_task:
    // whichever wave is free takes the next one), and what is left of the queue when the launch has no task left.  An item leaves at most
    // one follow-up item behind, so the ring never holds more than 2 RPW - 1 entries.
    const uint32_t q_base = wid * io.q_cap;
    uint32_t q_rd = 0, q_wr = 0, q_cnt = 0;
    const uint32_t n_tasks = (total + RPW - 1) / RPW;
    uint32_t pool_open = 1;

    // (per-lane flags are kept as 0/1 words in VGPRs on purpose: as `bool`s they become 64-bit lane masks in SGPRs, and this
    // kernel is short of SGPRs, not of VGPRs)
    for (;;) {
        uint32_t r = BGR_NONE, st = 0;  // r == BGR_NONE: the group has no item
        uint32_t task = BGR_NONE;
        if (q_cnt < RPW && pool_open) {
            task = claim_task(lds, io.cursor + io.task_ctr, n_tasks, lane);
            if (task == BGR_NONE) {
                pool_open = 0;
#ifdef BGR_PHASE_TIMING
                if (!wt2) wt2 = wall_clock64();
#endif
            }
        }
        if (task != BGR_NONE) {  // fresh reads
            if (task * RPW + grp < total) r = task * RPW + grp;
        } else {                 // the queue: a full group, or -- no task left -- what remains
            if (q_cnt == 0) break;
            const uint32_t take = q_cnt < RPW ? q_cnt : RPW;
            if (grp < take) {
                uint32_t at = q_rd + grp;
                if (at >= io.q_cap) at -= io.q_cap;
                // (written by this wave some iterations ago; read past the CU's vector cache all the same)
                r = __hip_atomic_load(&io.queue[q_base + at].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                st = __hip_atomic_load(&io.queue[q_base + at].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            q_rd += take;
            if (q_rd >= io.q_cap) q_rd -= io.q_cap;
            q_cnt -= take;
        }
        uint32_t L = 0, act = 0;  // act: the group takes part (its item is one this kernel maps)
        u64* F = RD + grp * W;
        {   // stage the item's 2-bit words: the lanes of a group bring the words of its read -- or of reverseComplements(read)
            // (utils.cpp:66-73), word j of which is the reversed complement of bases [L - 32 (j + 1), L - 32 j)
            const u64* src = io.fw3;
            u64 a0 = 0;  // (ASCII staging: where the read's characters start)
            if (r != BGR_NONE) {
                const u64 off = io.read_offs[r];
                L = (uint32_t)(io.read_offs[r + 1] - off);
                act = ASCII ? 1u : ((io.hasn[r >> 5] >> (r & 31)) & 1u) ^ 1u;  // a read with an N goes to the general kernel
                if (((L + 31) >> 5) >= W) act = 0;               // so does a read too long for one lane per word (a batch of mixed lengths)
                if (ASCII) a0 = ascii_start(io, r, off);
                else src += packed_word_offset(off, r);
            }
            const uint32_t Wr = (L + 31) >> 5;
            uint32_t chars = 0;
            // (the lane's first word is worked out from the lane number here, behind an empty asm: what the loop derives from `sub` would
            // otherwise be hoisted out of the kernel's loop and held in registers through the scan and the extension, which have none to spare)
            uint32_t j0 = threadIdx.x;
            asm volatile("" : "+v"(j0));
            for (uint32_t j = j0 % GL; j < W; j += GL) {
                u64 f = 0;
                if (act && j < Wr) {
                    if (ASCII) {
                        // no pre-pass, no planes: the words straight from the characters (a launch handed ASCII reads: 150 B in instead of 40 B of planes
                        // that a pre-pass wrote and this kernel read back; ~11 vector instructions per read)
                        // (reads end to end: what follows a read in its last 32-byte window are the next read's bases -- no character is masked;
                        // reads scattered in a text: a newline and a header follow, masked off precisely)
                        u64 fw;
                        const int32_t p = (st >> 31) ? (int32_t)L - 32 * ((int32_t)j + 1) : 0;
                        const u64 at = (st >> 31) ? a0 + (uint32_t)(p > 0 ? p : 0) : a0 + 32ull * j;
                        const uint32_t vv = (st >> 31) ? (p >= 0 ? 32u : (uint32_t)(32 + p)) : L - 32 * j;
                        if (io.ascii_src) fw = ascii_word<false>(io.ascii, at, vv, io.ascii_bytes, &chars);
                        else fw = ascii_word<true>(io.ascii, at, vv, io.ascii_bytes, &chars);
                        if (!(st >> 31)) f = fw;
                        else if (p >= 0) f = ~rev2_fast(fw);
                        else f = (~rev2_fast(fw >> (64 - 2 * vv))) & (~0ULL << (64 - 2 * vv));
                    } else if (!(st >> 31)) f = src[j];
                    else {
                        const int32_t p = (int32_t)L - 32 * ((int32_t)j + 1);
                        if (p >= 0) f = ~rev2_fast(win32(src, (u64)(uint32_t)p));
                        else { const uint32_t v = (uint32_t)(32 + p); f = (~rev2_fast(src[0] >> (64 - 2 * v))) & (~0ULL << (64 - 2 * v)); }
                    }
                }
                F[j] = f;
            }
            if (ASCII) {  // an N anywhere in the read (bit 3 of a character): the general kernel
                uint32_t n8 = chars & 0x08080808u;
                n8 |= quad_xor1(n8);
                if (GL >= 4) n8 |= quad_xor2(n8);
                if (GL >= 8) n8 |= half_row_mirror(n8);
                if (GL == 16) n8 |= (uint32_t)__builtin_amdgcn_mov_dpp((int)n8, 0x140, 0xF, 0xF, true);  // row_mirror
                if (n8) act = 0;
            }
        }
        wave_sync();

        // ---- anchors (getNOverlap, aligner.cpp:345-378): the next overlap (k-1)-mer of each item from where its scan stands;
        // record | canonical << 28
        uint32_t a_pos = 0, a_rec = BGR_NONE;
        if constexpr (STAGE) {
            // Two scanners per wave: lanes 0-31 scan one item, lanes 32-63 another, 32 positions per step each.  A half is done with its
            // item once it has seen the item's first hit or has passed npos; it then takes the next item in group order, so a step rarely
            // spends lanes beyond the hit an item needs (E. coli scale: 22.7 -> 19.1 steps per sixteen reads, tools/scan_halves.py).  A step
            // still looks up 64 (k-1)-mers.
            // Per half, all uniform: the item's group hq, the step's first position hb and the item's npos hn (0: the half is idle).
            // `pend`: bit GL q = group q's item is still to be scanned (an item with nothing left to scan never gets there: no anchor).
            uint32_t g_from = st & G4_ST_POS_MASK;  // where the group's item resumes: the first position it may report
            uint32_t g_npos = L >= K1 ? L - K1 + 1 : 0;
            if (!prm.effort && g_npos > 1) g_npos = 1;
            uint32_t to_scan = (act != 0 && g_from < g_npos) ? 1u : 0u;
            // The jump (graph_layout.h, jump index): most positions a scan looks up are interior (k-1)-mers of the unitig the read lies on, and
            // under property P none of those is a key.  For all sixteen items at once: the four lanes of an item hash the item's first
            // BGR_JUMP_NEAR windows and BGR_JUMP_FAR windows that share no base with them (a substitution under the near windows loses every one
            // of them, and the far ones with it unless they lie clear of it).  Of either set the first window whose hash selects it (one in
            // BGR_JUMP_STRIDE does, and only those are in the index) is probed, both loads in flight together; the near entry is used when it hits,
            // else the far one.  A hit names a unitig and an offset, i.e. a diagonal: the strand occupies read positions [A, A + len), A below,
            // at or above the resume position (a far window often lies in the NEXT unitig).  The lanes compare the read with `seq` along it over
            // [cs, ce) = [max(A, resume), min(A + len, L)), past every mismatch, and keep the first and the last one.  A window is VERIFIED iff
            // all its k-1 bases lie in the stretch and none is a mismatch: it is the strand's own (k-1)-mer, a key exactly at strand offset 0 and
            // len - (k-1).  The verified windows in front of the first mismatch and behind the last one are what counts: fb = the smallest
            // verified key position, and the scan is left the range [lo, hi) -- from the first unverified window to one past the last unverified
            // window below fb (below npos without one) -- with a_pos / a_rec pre-set to fb: the range's first hit overwrites them, as the plain
            // scan's would.  An empty range settles the item.  Verified windows between two mismatches are scanned needlessly; they are no keys.
            // The index is only a hint: nothing is concluded from a window that was not compared in full, and an item without a hit is scanned
            // as it always was.
#ifdef BGR_PHASE_TIMING
            if ((g.flags & BGR_GF_JUMP) && prm.debug_stop != 1) {  // (1 = stops behind the staging of the reads)
#else
            if (g.flags & BGR_GF_JUMP) {
#endif
                // (where the index and `meta` lie is read from the blob's header here, once per sixteen items, three scalar loads: as kernel
                // arguments they would stay in SGPRs through the scan and the walks, which have none to spare)
                const BgrBlobHeader* jh = g.hdr;
                asm volatile("" : "+s"(jh));
                const uint4* jtab = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(jh) + jh->off_jump);
                const BgrUnitigMeta* jmeta = reinterpret_cast<const BgrUnitigMeta*>(reinterpret_cast<const char*>(jh) + jh->off_meta);
                const uint32_t jnb = (uint32_t)jh->jump_buckets;
                // lane `sub` looks at the near positions g_from + sub + 4 j and at the far ones, k-1 further on (the first far window starts behind
                // the last near window's last base); my_rel / my_far: its first selected window of either set, counted from g_from (none: 255),
                // with the window's tag in bits 8-15 and "it is its own canonical form" in bit 31; my_bk / my_fbk: the bucket.  A far window
                // past the read's last one is not looked at: a short read has none.
                static_assert(BGR_JUMP_NEAR % GL == 0 && BGR_JUMP_FAR % GL == 0 && BGR_JUMP_NEAR + BGR_JUMP_FAR + 32u < 255u, "whole rounds of the quad; the offset fits its byte");
                uint32_t my_rel = 255u, my_bk = 0, my_far = 255u, my_fbk = 0;
#pragma unroll 1
                for (uint32_t r0 = 0; r0 < BGR_JUMP_NEAR + BGR_JUMP_FAR; r0 += GL) {
                    const uint32_t far = r0 >= BGR_JUMP_NEAR ? 1u : 0u;
                    const uint32_t rel = r0 + sub + (far ? K1 : 0u);
                    if (to_scan && (far ? my_far : my_rel) == 255u && g_from + rel < g_npos) {
                        const u64 num = lds_win32(F, g_from + rel) >> (64 - 2 * K1);
                        const u64 rcn = rcb_fast(num, K1);
                        const u64 mx = bgr_mix64(num < rcn ? num : rcn);
                        if (bgr_jump_selects(mx) && num != rcn) {
                            const uint32_t v = rel | (bgr_tab_fp(mx) << 8) | (num < rcn ? 0x80000000u : 0u);
                            const uint32_t bk = __umulhi((uint32_t)mx, jnb);
                            if (far) { my_far = v; my_fbk = bk; }
                            else { my_rel = v; my_bk = bk; }
                        }
                    }
                }
                // the quad's first selected window of either set: the lane that holds it probes (two lanes: one load instruction for both)
                uint32_t n_sub = my_rel & 255u, f_sub = my_far & 255u;
                { const uint32_t o = quad_xor1(n_sub); n_sub = o < n_sub ? o : n_sub; }
                { const uint32_t o = quad_xor1(f_sub); f_sub = o < f_sub ? o : f_sub; }
                { const uint32_t o = quad_xor2(n_sub); n_sub = o < n_sub ? o : n_sub; }
                { const uint32_t o = quad_xor2(f_sub); f_sub = o < f_sub ? o : f_sub; }
                uint4 bn = make_uint4(0, 0, 0, 0), bf = make_uint4(0, 0, 0, 0);
                if ((my_rel & 255u) == n_sub && n_sub != 255u) bn = jtab[my_bk];
                if ((my_far & 255u) == f_sub && f_sub != 255u) bf = jtab[my_fbk];
                // the entry whose tag is the window's (tags are 1 .. 255: a lane that did not load matches nothing); bit 31 of idc: the read's
                // window is its own canonical form
                auto entry = [](const uint4& b, uint32_t mine, uint32_t& idc, uint32_t& tt) {
                    const uint32_t tag = (mine >> 8) & 0xFFu;
                    const bool first = (b.y & 0xFFu) == tag;
                    tt = first ? b.y : (b.w & 0xFFu) == tag ? b.w : 0u;
                    idc = tt ? ((first ? b.x : b.z) & 0x7FFFFFFFu) | (mine & 0x80000000u) : 0u;
                };
                uint32_t w_idc, w_tt, f_idc, f_tt;
                entry(bn, my_rel, w_idc, w_tt);
                entry(bf, my_far, f_idc, f_tt);
                uint32_t near_hit = w_tt;  // (one lane of the quad holds an entry: into all four)
                near_hit |= quad_xor1(near_hit); near_hit |= quad_xor2(near_hit);
                if (!near_hit) { w_tt = f_tt; w_idc = f_idc; }
                w_tt |= quad_xor1(w_tt); w_tt |= quad_xor2(w_tt);
                w_idc |= quad_xor1(w_idc); w_idc |= quad_xor2(w_idc);
                const uint32_t w_sub = near_hit ? n_sub : f_sub;  // the probed window, counted from g_from
                // the diagonal: the read on strand rcs of the unitig (0: forward, 1: the copy at F + len); the stretch starts at read position
                // cs = max(A, g_from), which is offset soff of that strand (soff == 0: A >= g_from, cs == g_from: A <= g_from), and ends at ce
                // (0: no diagonal).  The strand's (k-1)-mers are keys at offset 0 -- read position cs when soff == 0 -- and at len - (k-1) -- read
                // position p1 -- and nowhere else.  rec0, rec1: what the two are as anchors (strand offset 0 is the unitig's beg forward and rc(end)
                // on the other strand, the far end the other way round); BGR_NONE: not among the item's positions [g_from, npos), or, the far end,
                // behind the read's last base
                uint32_t rec0 = BGR_NONE, rec1 = BGR_NONE, p1 = 0, cs = g_from, ce = 0;
                uint32_t sw = 0, ss = 0;  // base cs of the read lies at bit ss of seq word sw (the store stays below 2^32 bytes)
                if (w_tt) {
                    const BgrUnitigMeta* mp = jmeta + (w_idc & BGR_SLOT_ID_MASK);
                    const uint4 m0 = *reinterpret_cast<const uint4*>(mp);  // len, flags, rec_beg, rec_end
                    const u64 Fm = mp->F;
                    const uint32_t ulen = m0.x;
                    const uint32_t t = w_tt >> 8;
                    const uint32_t rcs = ((w_idc >> 31) ^ (w_idc >> 30)) & 1u;
                    if (t + K1 <= ulen) {
                        const uint32_t u = rcs ? ulen - K1 - t : t;  // the probed window's offset on that strand
                        const uint32_t soff = u > w_sub ? u - w_sub : 0u;
                        cs = g_from + (w_sub > u ? w_sub - u : 0u);
                        const u64 sbase = Fm + (rcs ? ulen : 0u) + soff;
                        sw = (uint32_t)(sbase >> 5);
                        ss = 2u * ((uint32_t)sbase & 31u);
                        const uint32_t room = ulen - soff;           // bases of the strand from soff on
                        ce = L - cs < room ? L : cs + room;
                        p1 = cs + (room - K1);
                        if (soff == 0 && cs < g_npos) rec0 = (rcs ? m0.w : m0.z) | ((m0.y & (rcs ? BGR_META_CANON_RCEND : BGR_META_CANON_BEG)) ? G4_CANON : 0u);
                        if (ce == cs + room && p1 < g_npos) rec1 = (rcs ? m0.z : m0.w) | ((m0.y & (rcs ? BGR_META_CANON_RCBEG : BGR_META_CANON_END)) ? G4_CANON : 0u);
                    }
                }
                // compare: lane `sub` takes the 64-base chunks sub, sub + 4, ... of [cs, ce) -- three words of either side, two windows --
                // so reads of up to 256 bases behind cs take one round; e1 = the first mismatch, or ce; eL = the last one, or -1.  The third
                // word is read only when the chunk's second half is needed: the read's row and `seq` hold it then (scan_take_word.h: a row
                // has a word to spare; the store ends in two pad words).  What a chunk holds from ce on is no part of the stretch: masked off.
                uint32_t e1 = ce;
                int32_t eL = -1;
                const uint32_t fs = 2u * (cs & 31u);
                for (uint32_t c0 = 0; __any(cs + 64u * c0 < ce); c0 += GL) {
                    const uint32_t rp = cs + 64u * (c0 + sub);
                    if (rp < ce) {
                        const uint32_t nv = ce - rp;  // the chunk's bases inside the stretch (64: or more)
                        const bool two = nv > 32u;
                        const u64* fp = F + (rp >> 5);
                        const u64* sp = g.seq + sw + 2u * (c0 + sub);
                        const u64 f0 = fp[0], f1 = fp[1], f2 = two ? fp[2] : 0;
                        const u64 s0 = sp[0], s1 = sp[1], s2 = two ? sp[2] : 0;
                        u64 xa = ((f0 << fs) | ((f1 >> 1) >> (63 - fs))) ^ ((s0 << ss) | ((s1 >> 1) >> (63 - ss)));
                        u64 xb = two ? ((f1 << fs) | ((f2 >> 1) >> (63 - fs))) ^ ((s1 << ss) | ((s2 >> 1) >> (63 - ss))) : 0;
                        // (the stretch ends in the chunk's first half, nv < 32, or in its second, 32 < nv < 64: one mask, for that half)
                        const u64 keep = ~0ULL << (2u * ((0u - (nv < 64u ? nv : 64u)) & 31u));
                        if (two) xb &= keep;
                        else xa &= keep;
                        if (xa | xb) {
                            const uint32_t q = xa ? rp + ((uint32_t)__builtin_clzll(xa) >> 1) : rp + 32u + ((uint32_t)__builtin_clzll(xb) >> 1);
                            const uint32_t z = xb ? rp + 63u - ((uint32_t)__builtin_ctzll(xb) >> 1) : rp + 31u - ((uint32_t)__builtin_ctzll(xa) >> 1);
                            e1 = q < e1 ? q : e1;
                            eL = (int32_t)z > eL ? (int32_t)z : eL;
                        }
                    }
                }
                { const uint32_t o = quad_xor1(e1); e1 = o < e1 ? o : e1; }
                { const int32_t o = (int32_t)quad_xor1((uint32_t)eL); eL = o > eL ? o : eL; }
                { const uint32_t o = quad_xor2(e1); e1 = o < e1 ? o : e1; }
                { const int32_t o = (int32_t)quad_xor2((uint32_t)eL); eL = o > eL ? o : eL; }
                uint32_t jumped = 0, raised = 0, by_far = 0, bounded = 0;
                if (ce) {
                    // the key at the stretch's first window is verified iff no mismatch lies in it, the one at its last window iff the last
                    // mismatch lies in front of it
                    const uint32_t v0 = e1 >= cs + K1 ? 1u : 0u;  // the stretch's first window is verified, and all up to e1 - (k-1)
                    uint32_t fb = BGR_NONE;
                    if (rec0 != BGR_NONE && v0) { fb = cs; a_rec = rec0; }
                    else if (rec1 != BGR_NONE && eL < (int32_t)p1) { fb = p1; a_rec = rec1; }
                    if (fb != BGR_NONE) a_pos = fb;
                    // [lo, hi): from the first unverified window to one past the last unverified window below fb (below npos without one).  The
                    // window below the limit is verified iff it lies in the stretch behind the last mismatch: so are all down to that mismatch.
                    const uint32_t lo = (cs == g_from && v0) ? e1 - K1 + 1u : g_from;
                    const uint32_t lim = fb != BGR_NONE ? fb : g_npos;
                    const int32_t t = (int32_t)lim - 1;
                    uint32_t hi = lim;
                    if (t >= (int32_t)cs && (uint32_t)t + K1 <= ce && eL < t) hi = (uint32_t)(eL + 1) > cs ? (uint32_t)(eL + 1) : cs;
                    if (lo >= hi) { to_scan = 0; jumped = 1; by_far = near_hit ? 0u : 1u; }  // nothing left to scan: the anchor is fb, or there is none
                    else {
                        raised = lo > g_from ? 1u : 0u;
                        bounded = (raised || hi < g_npos) ? 1u : 0u;
                        g_from = lo;
                        g_npos = hi;
                    }
                }
#ifdef BGR_PHASE_TIMING
                dbg_jumped += (uint32_t)__popcll(__ballot(jumped != 0 && sub == 0));
                dbg_raised += (uint32_t)__popcll(__ballot(raised != 0 && sub == 0));
                dbg_far += (uint32_t)__popcll(__ballot(by_far != 0 && sub == 0));
                dbg_bounded += (uint32_t)__popcll(__ballot(bounded != 0 && sub == 0));
#endif
                (void)jumped; (void)raised; (void)by_far; (void)bounded;
            }
            u64 pend = __ballot(to_scan != 0 && sub == 0);
#ifdef BGR_PHASE_TIMING
            if (prm.debug_stop == 1) pend = 0;  // 1 = stops behind the staging of the reads
            dbg_items += (uint32_t)__popcll(pend);
            ++dbg_groups;
#endif
            // The lane's own copy of its half's state, set when the half takes an item and stepped per 32 positions (no per-step selects
            // between the halves' uniforms).  A half starts at a multiple of 16 -- the item's resume position rounded down -- so lane j
            // always holds a position = j mod 16: the bit its window starts at inside a dword is the lane's constant, and the window is
            // three dwords and three shifts (lds_win32_fixed).  The lane keeps
            //   li = (its position - the resume position) << 6 | the window's shift, ln = (npos - the resume position) << 6 (0: idle):
            //        li < ln, unsigned, says that the position is one of the item's AND not below where the item resumes (the lanes below
            //        wrap around; they are off in the item's first step only, so an anchor that has failed is never seen again);
            //   wa, wb = the LDS byte addresses of the dword its window starts in and of the next one.
            // What a half needs of an item is worked out for all sixteen groups at once, here, as ONE word per group (scan_take_word.h: resume
            // position, positions left, the item's dword counted from the wave's first read word, 16 - resume position % 16), and fetched by
            // one readlane when the half takes the item; the half's uniforms and the lanes' li, ln, wa, wb all come out of that word.
            static_assert(RPW == kTakeGroups, "scan_take_word.h counts sixteen groups per wave");
            const bool hi = lane >= 32;
            // (the lane's two constants are worked out here, once per sixteen items, behind an empty asm that keeps the compiler from
            // hoisting them out of the kernel's loop: they would cost the extension below two registers it does not have)
            uint32_t sl = threadIdx.x;
            asm volatile("" : "+v"(sl));
            // li = lcm + ((16 - resume position % 16) << 6): the lane's position in its half, less 16, and the window's shift
            const uint32_t lcm = (((sl & 31u) << 6) | (32u - 2u * (sl & 15u))) - (16u << 6);
            // the wave's first read word (RD, worked out again from the lane number: as lds_addr(RD) it would be hoisted as well); lanes 16-31
            // of a half start one dword further on
            const uint32_t c4w = lds_addr(lds + 64 + ktab_words) + (sl >> 6) * (RPW * W * 8u) + 4u * ((sl >> 4) & 1u);
            const uint32_t g_tw = take_word_pack(g_from, g_npos - g_from, ((sl & 63u) / GL) * (W * 2u) + (g_from >> 4));
            uint32_t li = 0, ln = 0, wa = 0, wb = 0;
            auto take = [&](bool h, uint32_t& hq, uint32_t& hb, uint32_t& hn) {
                uint32_t s_res = 16, s_left = 0, s_dw = 0;  // (no item left: the half idles, parked on the wave's first read word)
                hn = 0;
                if (pend) {
                    const int at = __ffsll((long long)pend) - 1;
                    pend &= pend - 1;
                    const uint32_t w = rl32(g_tw, at);
                    s_res = take_word_res(w);
                    s_left = take_word_left(w);
                    s_dw = take_word_dword(w);
                    hq = (uint32_t)at / GL;
                    hb = take_word_resume(w) & ~15u;
                    hn = take_word_resume(w) + s_left;
                }
                if (hi == h) {
                    li = lcm + (s_res << 6);
                    ln = s_left << 6;
                    // dword d of an item's words, in base order, is dword d ^ 1 in memory: the words start at a multiple of 8 bytes
                    const uint32_t t = c4w + (s_dw << 2);
                    wa = t ^ 4u;
                    wb = (t + 4u) ^ 4u;
                }
            };
            uint32_t q0 = 0, b0 = 0, n0 = 0, q1 = 0, b1 = 0, n1 = 0;
            take(false, q0, b0, n0);
            take(true, q1, b1, n1);
            while (n0 | n1) {
#ifdef BGR_PHASE_TIMING
                ++dbg_steps;
#endif
                const bool valid = li < ln;
                u64 num = 0;
                if (valid) num = lds_win32_fixed(wa, wb, li) >> (64 - 2 * K1);
                const u64 rcn = rcb_fast(num, K1);  // no N in the read: the rolling reverse k-mer is rcb of the forward one
                uint32_t idx = scan_find_key(g, ktab, num < rcn ? num : rcn, valid, (uint32_t)lane);
                const u64 mask = __ballot(idx != BGR_NONE);
                li += 32u << 6;
                wa += 8;
                wb += 8;
                if (mask) {
                    if (idx != BGR_NONE && num <= rcn) idx |= G4_CANON;
                    // each half's first hit goes to its item's group: a readlane of the hit lane, a select on grp
                    auto settle = [&](uint32_t mh, int off, uint32_t hq, uint32_t hb, uint32_t& hn) {
                        if (mh) {
                            const uint32_t f = (uint32_t)__builtin_ctz(mh);
                            const uint32_t h = rl32(idx, off + (int)f);
                            if (grp == hq) { a_pos = hb + f; a_rec = h; }
                            hn = 0;
                        }
                    };
                    if (n0) settle((uint32_t)mask, 0, q0, b0, n0);
                    if (n1) settle((uint32_t)(mask >> 32), 32, q1, b1, n1);
                }
                b0 += 32;
                if (b0 >= n0) n0 = 0;
                b1 += 32;
                if (b1 >= n1) n1 = 0;
                if (!n0) take(false, q0, b0, n0);  // (both halves done: the low one takes first)
                if (!n1) take(true, q1, b1, n1);
            }
        } else {
            // key table in L2 (minimizer filter: a window maximum across the whole wave): one item per step on all 64 lanes
            for (uint32_t q = 0; q < RPW; ++q) {
                if (!rl32(act, (int)(GL * q))) continue;
#ifdef BGR_PHASE_TIMING
                if (prm.debug_stop == 1) continue;  // 1 = stops behind the staging of the reads
#endif
                const uint32_t Lq = rl32(L, (int)(GL * q)), stq = rl32(st, (int)(GL * q));
                const u64* A = RD + q * W;
                uint32_t npos = Lq >= K1 ? Lq - K1 + 1 : 0;
                if (!prm.effort && npos > 1) npos = 1;
                for (uint32_t base = stq & G4_ST_POS_MASK; base < npos; base += scan_step) {
                    const uint32_t i = base + (uint32_t)lane;
                    const bool valid = i < npos && (uint32_t)lane < scan_step;
                    u64 num = 0, win = 0;
                    if (valid || (mmx_w && i + BGR_MMX_BASES <= Lq)) win = lds_win32(A, i);
                    if (valid) num = win >> (64 - 2 * K1);
                    const u64 rcn = rcb_fast(num, K1);  // no N in the read: the rolling reverse k-mer is rcb of the forward one
                    const uint32_t mblock = !mmx_w ? 0u
                                          : wide_scan ? scan_mblock_wide(g, win, i + BGR_MMX_BASES <= Lq, i + 2 * BGR_MMX_BASES <= Lq, mmx_w)
                                                      : scan_mblock(g, win, i + BGR_MMX_BASES <= Lq, mmx_w);
                    uint32_t idx = find_key<true>(g, ktab, num < rcn ? num : rcn, valid, mblock);
                    const u64 mask = __ballot(idx != BGR_NONE);
                    if (mask) {
                        if (idx != BGR_NONE && num <= rcn) idx |= G4_CANON;
                        const int s1 = __ffsll((long long)mask) - 1;
                        const uint32_t h1 = rl32(idx, s1);
                        if (grp == q) { a_pos = base + (uint32_t)s1; a_rec = h1; }
                        break;
                    }
                }
            }
        }

        // ---- extension (alignReadGreedy's loop body, alignerGreedy.cpp:41-52), the wave's items abreast; a group whose anchor fails
        // leaves a follow-up item that scans on behind it, while the others go on ----
        // phase: 1 left walk, 2 first right step, 3 later right steps; 0 the walk is over (aligned, or there was no anchor),
        // 4 the path outgrew the registers, 5 every anchor seen failed.  `tried` counts on in the item's state word.
        // The two walks of an anchor run at the same time on the two lane pairs of the group (g2_step): lanes 0-1 walk left, lanes 2-3
        // walk right, each with its own phase, position, half, miss count and path ints, so the wave waits for the longest SIDE of its
        // sixteen reads rather than for the longest left + right (E. coli scale, a CPU model that counts only the forward first items that align,
        // tools/walk_sides.py: 2.9 instead of 3.9 loop iterations per sixteen reads).
        // The right walk's steps do not depend on the left walk: a step's choice ignores the budget (which only decides whether the
        // chosen candidate is accepted), and misses are >= 0, so "every step fits what is left of m" == "the running total stays <= m".
        // Each pair stops once its own total passes m; the read is settled from both behind the loop, as the sequential walk would end.
        constexpr uint32_t PH = kG4PathInts / 2;
        // the read's row in the arena, left ints from lane 0, right ints from lane 2 (an index, as `gbase` below: a 64-bit pointer costs a VGPR spill)
        const uint32_t PT0 = (r == BGR_NONE ? 0u : r) * kG4PathInts;
        const uint32_t side = (sub >> 1) & 1u;  // 0: the left walk, 1: the right walk
        uint32_t phase = (act && a_rec != BGR_NONE) ? 1u + side : 0u;
#ifdef BGR_PHASE_TIMING  /* diagnostic builds (tools/phase_cost.sh): knob DEBUG_STOP = 2 stops behind the anchor scan */
        if (prm.debug_stop == 2) phase = 0;
#endif
        // rec: the half the next step reads (handle | canonical << 28).  An anchor is a key entry: its left walk starts from the half that
        // getEnd reads for it, its right walk from the one getBegin reads -- both handles sit in the key entry, fetched by ONE 8-byte load
        uint32_t rec = G4_REC_MASK;
        if (phase) {
            const uint32_t cn = (a_rec >> 28) & 1u;
            const uint2 h = *reinterpret_cast<const uint2*>(&g.keys[a_rec & G4_REC_MASK].hL);
            rec = ((cn ^ side) ? h.y : h.x) | (cn ? G4_CANON : 0u);
        }
        uint32_t pos = a_pos, cum = 0, ni = 0;  // cum: the pair's misses so far; ni: the path ints it has pushed
        for (;;) {
            if (phase == 1 && pos == 0) {  // the left walk reached the read's first base: push 0
                if (sub == 0) io.arena[PT0 + PH - 1 - ni] = 0;
                ++ni;
                phase = 0;
            }
            if (phase == 2 && L - pos - K1 == 0) phase = 0;  // nothing right of the anchor
            if (phase == 3 && L - pos < K1 + 1) phase = 0;   // |readLeft| < k
            if ((phase == 1 && ni > PH - 2) || ((phase == 2 || phase == 3) && ni > PH - 1)) phase = 4;  // path too long for the row (a left step may push two ints)
            const uint32_t on = (phase - 1u < 3u) ? phase : 0u;
            if (!__any(on != 0)) break;
            uint32_t miss, ext;
            int32_t sid;
            const uint32_t w1 = g2_step(g, F, L, K1, on, rec & G4_REC_MASK, (rec >> 28) & 1u, pos, m - cum, lane, &miss, &ext, &sid);
            if (on != 0) {
                if (!(w1 & G4_FOUND)) phase = 5;
                else {
                    if ((sub & 1u) == 0) io.arena[PT0 + (phase == 1 ? PH - 1 - ni : PH + ni)] = sid;
                    ++ni;
                    cum += miss;
                    if (w1 & G4_FITS) {
                        if (phase == 1) {
                            if (sub == 0) io.arena[PT0 + PH - 1 - ni] = (int32_t)(ext - pos);
                            ++ni;
                        }
                        phase = 0;
                    } else if (phase == 1) { pos -= ext; rec = w1; }
                    else { pos += ext; rec = w1; phase = 3; }
                }
            }
        }
        // Settle the read as the left-then-right walk would have ended (phase: 0 aligned, 4 general kernel, 5 failed): the left walk's
        // overflow or failure decides alone; then a right overflow goes to the general kernel only if the steps done so far fit m
        // together with the left walk's misses (else the sequential walk would have failed before it); then a right failure, or both
        // totals together above m, fail the anchor.
        const uint32_t o_phase = quad_xor2(phase), o_cum = quad_xor2(cum), o_ni = quad_xor2(ni);  // (the other pair: lanes l ^ 2)
        const uint32_t lph = side ? o_phase : phase, rph = side ? phase : o_phase;
        const uint32_t tot = cum + o_cum;
        const uint32_t nl = side ? o_ni : ni, nr = side ? ni : o_ni;
        if (lph == 4 || lph == 5) phase = lph;
        else if (rph == 4) phase = tot <= m ? 4u : 5u;
        else phase = (rph == 5 || tot > m) ? 5u : 0u;
        // (the next anchor of getNOverlap's list is taken up by a follow-up item that resumes behind this one -- rounds 3-4 restarted the
        // walk in this loop, which kept all sixteen groups' loop going for one walk: profiles/r05_scan_schemes.txt)
        if (phase == 5) st += 1u << G4_ST_TRIED_SHIFT;

        // ---- what became of each item (alignerGreedy.cpp:35-57) ---------------------------------------------------------------
        // 0 = aligned, 1 = no anchor on this strand and none tried before (++noOverlapRead), 2 = not aligned (both strands done),
        // 3 = a follow-up item `nst` goes into the wave's queue, 4 = general kernel (N in the read, path too long for the registers)
        uint32_t outcome = 4, nst = 0;
        const uint32_t rc = st >> 31;
        if (act) {
            const uint32_t tried = (st >> G4_ST_TRIED_SHIFT) & 0x7FFu;
            const uint32_t npos_g = (L >= K1 ? L - K1 + 1 : 0);
            const uint32_t npos_e = (!prm.effort && npos_g > 1) ? 1u : npos_g;
            if (phase == 4) outcome = 4;
            else if (a_rec != BGR_NONE && phase != 5) outcome = 0;
            else if (a_rec == BGR_NONE && tried == 0) outcome = 1;
            else {
                // the strand's anchors are used up when `effort` of them have been tried or the scan has passed the last position
                const uint32_t resume = a_pos + 1;  // (a_pos = the anchor tried last; unused when the scan found none)
                const uint32_t used_up = (a_rec == BGR_NONE || tried >= eff || resume >= npos_e) ? 1u : 0u;
                if (!used_up) { outcome = 3; nst = (st & ~G4_ST_POS_MASK) | resume; }
                else if (!rc) { outcome = 3; nst = G4_ST_RC; }  // the reverse complement, from its first position
                else outcome = 2;
                if (tried >= 0x7FEu || resume > G4_ST_POS_MASK) outcome = 4;  // (an item tries at most two anchors: the count stays inside its field)
            }
        }
        const uint32_t have = r != BGR_NONE ? 1u : 0u;

        // ---- publish: the path is the slice [PH - nl, PH + nr) of the read's row ----------------------------------------------------
        const uint32_t aligned = outcome == 0 ? 1u : 0u;
        const uint32_t p_n = aligned ? nl + nr : 0;
        const uint32_t gbase = (r == BGR_NONE ? 0u : r) * kG4PathInts + PH - nl;
        if (sub == 0 && have) {
            if (outcome <= 2) {
                const uint32_t code = (outcome == 0 ? BGR_ST_ALIGNED : outcome == 1 ? BGR_ST_NOANCHOR : BGR_ST_FAILED) | (rc ? BGR_ST_RC : 0u);
                io.results[r] = make_uint2(aligned ? gbase : 0u, p_n | (code << 24));
            } else if (outcome == 4) {
                io.gen_list[atomicAdd(io.cursor + io.gen_ctr, 1u)] = r;
            }
        }
        {   // follow-up items into the wave's queue
            const bool listed = sub == 0 && have && outcome == 3;
            const u64 lm = __ballot(listed);
            if (lm) {
                const uint32_t cnt = (uint32_t)__popcll(lm);
                if (listed) {
                    uint32_t at = q_wr + __builtin_amdgcn_mbcnt_hi((uint32_t)(lm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lm, 0u));  // listed lanes below this one
                    if (at >= io.q_cap) at -= io.q_cap;
                    io.queue[q_base + at] = make_uint2(r, nst);
                }
                q_wr += cnt;
                if (q_wr >= io.q_cap) q_wr -= io.q_cap;
                q_cnt += cnt;
            }
        }
        // what became of the read: counted per workgroup in LDS (wg_counts[outcome]: aligned, no anchor, not aligned, follow-up item)
        if (sub == 0 && have && outcome <= 3) atomicAdd(&wg_counts[outcome], 1u);
        wave_sync();
    }
#ifdef BGR_PHASE_TIMING
    if (io.wave_times && lane == 0) {
        unsigned long long* w = io.wave_times + 4ull * (blockIdx.x * waves + wave);
        w[0] = wt0; w[1] = wt1; w[2] = wt2; w[3] = wall_clock64();
        // behind the time stamps of all waves: the wave's scan counts (two-scanner instances; 0 steps for the others)
        unsigned long long* c = io.wave_times + 4ull * (gridDim.x * waves) + 4ull * (blockIdx.x * waves + wave);
        c[0] = dbg_steps; c[1] = (unsigned long long)dbg_items | ((unsigned long long)dbg_far << 32);
        c[2] = (unsigned long long)dbg_groups | ((unsigned long long)dbg_bounded << 32); c[3] = (unsigned long long)dbg_jumped | ((unsigned long long)dbg_raised << 32);
    }
#endif
    __syncthreads();
    if (threadIdx.x == 0) {  // aligner.h:68 counters: [0] readNumber [1] noOverlapRead [2] alignedRead [3] notAligned
        unsigned long long* counters = reinterpret_cast<unsigned long long*>(io.cursor + kCurCounters);
        const uint32_t al = wg_counts[0], noov = wg_counts[1], na = wg_counts[2], qa = wg_counts[3];  // (indexed by `outcome`)
        if (al | noov | na) atomicAdd(&counters[0], (unsigned long long)(al + noov + na));
        if (noov) atomicAdd(&counters[1], (unsigned long long)noov);
        if (al) atomicAdd(&counters[2], (unsigned long long)al);
        if (na) atomicAdd(&counters[3], (unsigned long long)na);
        if (qa) atomicAdd(io.cursor + kCurFollowUps, qa);  // follow-up items of the launch (bgr_aligner_pass_counts)
    }
}

}  // namespace

const void* greedy_kernel(KernelId k, bool stage, bool ascii) {
    constexpr int GL = (int)kG4GroupLanes;
    switch (k) {
        case KernelId::kGreedyMulti:
            if (ascii) return stage ? kernel_ptr(bgr_align_greedy_multi_kernel<true, GL, true>) : kernel_ptr(bgr_align_greedy_multi_kernel<false, GL, true>);
            return stage ? kernel_ptr(bgr_align_greedy_multi_kernel<true, GL, false>) : kernel_ptr(bgr_align_greedy_multi_kernel<false, GL, false>);
        case KernelId::kGreedyWide: return stage ? kernel_ptr(bgr_align_greedy_wide_kernel<true>) : kernel_ptr(bgr_align_greedy_wide_kernel<false>);
        case KernelId::kGreedy: return stage ? kernel_ptr(bgr_align_greedy_kernel<true>) : kernel_ptr(bgr_align_greedy_kernel<false>);
        default: return nullptr;
    }
}

}  // namespace bgr
