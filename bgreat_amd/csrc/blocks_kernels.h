// blocks_kernels.h -- launch interface of blocks_kernels.hip: phased bubble pairs chained into haplotype blocks (bgr_block_entry in
// include/bgreat_gpu.h has the definition; blocks_host.h the node readings and the decision), where the two lists lie in HBM.
#ifndef BGREAT_AMD_BLOCKS_KERNELS_H
#define BGREAT_AMD_BLOCKS_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bgreat_gpu.h"
#include "blocks_host.h"

namespace bgr {

// The neighbour relation of the decided phase records is a set of linked lists and rings over the 2 n nodes (node 2 i = bubble record i, node
// 2 i + 1 = its mate), so chaining is list ranking with a parity carried along.  The passes, each its own launch on the caller's stream (no
// workgroup ever waits for another; a launch never reads a word that another thread of the same launch writes, except through the atomics of 1, 2):
//   1  index    one thread per node x: node_of_source[o(source(x))] = x by atomicCAS from "none" (the table is memset to it): an entry already
//               taken sets a bit of the error word
//   2  link     one thread per phase record: an undecided one is skipped; X = node_of_source[o(source)], Y = node_of_source[o(via)]; the error
//               word is set when either is missing, X's sink, branches or Y's branches, sink differ from the record, or next[X], prev[Y] or those
//               of the mate link are taken (each claimed by one atomicCAS from "none"); else next / prev hold the link X -> Y and the mate link
//               mate(Y) -> mate(X); the parity travels in bit 31 of the prev word
//   3  rank     pointer jumping towards the head: a state {pointer, links jumped, xor of their parities | done, smallest node of the span} per node,
//               ceil(log2(2 n)) rounds over ping-pong buffers.  A node that has met a head is done: pointer = the head, links = its place in the
//               chain, parity = its haplotype.  A node not done after the last round lies on a ring, and its span has covered the whole ring:
//               the smallest node is the ring's first
//   4  open     every ring is cut at the link that enters its first node (the node keeps the removed link's parity in its ring word), and pass 3
//               runs once more for all nodes: now every component is a path
//   5  tail     a node without a successor hands its head the chain's size, its tail, and the ring's flags
//   6  count    per tile of BGR_BLOCKS_TILE nodes: the reported heads (a path's head h < mate(tail), a ring's first node when it is even: the
//               mate ring's first is mate(h)) and the sum of their sizes
//   7  scan     both counts: the variants' scan as it stands, one workgroup each
//   8  place    pass 6 again: every reported head learns its block's ordinal and the offset of its first entry; then one thread per node writes
//               its 24-byte entry at offset(head) + place
// The entries come out in (first node, chain order) by construction: no sort, no atomics on the output.  The host has checked the ids of both lists
// before any of this runs (blocks_check); the kernels check them again wherever one indexes a table, and a place beyond the output is not written.
const uint32_t kBlocksTile = BGR_BLOCKS_TILE;
const uint32_t kBlocksThreads = 256;   // each thread owns kBlocksTile / kBlocksThreads = 4 consecutive nodes
const uint32_t kBlocksNone = 0xFFFFFFFFu;
// the error word's bits
enum : uint32_t { kBlocksErrSource = 1, kBlocksErrMissing = 2, kBlocksErrDiffers = 4, kBlocksErrTaken = 8, kBlocksErrPlace = 16, kBlocksErrId = 32 };

inline uint64_t blocks_tiles(uint64_t n_bubbles) { return (2 * n_bubbles + kBlocksTile - 1) / kBlocksTile; }
inline uint32_t blocks_rounds(uint64_t n_bubbles) { uint32_t k = 0; while ((1ull << k) < 2 * n_bubbles) ++k; return k; }

// scratch of one call (N = 2 n_bubbles nodes, T tiles), in this order: uint4 sa[N], sb[N], meta[N]; u64 offs_s[T + 1 or + 2], offs_b[likewise];
// u32 node_of_source[2 (n_unitigs + 1)], next[N], prev[N] (these three are memset to "none" in one go), ring[N], hoff[T x tile], hblk[T x tile],
// counts_s[T], counts_b[T], err[4] -- 136 bytes per bubble and 8 per unitig
struct BlocksScratch {
    uint4 *sa, *sb, *meta;
    uint64_t *offs_s, *offs_b;
    uint32_t *nos, *next, *prev, *ring, *hoff, *hblk, *counts_s, *counts_b, *err;
    uint64_t bytes, none_bytes;   // the whole scratch; the stretch from nos that starts as "none"
    BlocksScratch(void* p, uint64_t n_bubbles, uint64_t n_unitigs) {
        const uint64_t N = 2 * n_bubbles, T = blocks_tiles(n_bubbles), W = (T + 2) & ~1ull;
        sa = static_cast<uint4*>(p); sb = sa + N; meta = sb + N;
        offs_s = reinterpret_cast<uint64_t*>(meta + N); offs_b = offs_s + W;
        nos = reinterpret_cast<uint32_t*>(offs_b + W); next = nos + 2 * (n_unitigs + 1); prev = next + N; ring = prev + N;
        hoff = ring + N; hblk = hoff + T * kBlocksTile; counts_s = hblk + T * kBlocksTile; counts_b = counts_s + T; err = counts_b + T;
        none_bytes = (2 * (n_unitigs + 1) + 2 * N) * 4;
        bytes = 3 * N * 16 + 2 * W * 8 + (2 * (n_unitigs + 1) + 3 * N + 2 * T * kBlocksTile + 2 * T + 4) * 4;
    }
};
inline uint64_t blocks_scratch_bytes(uint64_t n_bubbles, uint64_t n_unitigs) {
    const uint64_t N = 2 * n_bubbles, T = blocks_tiles(n_bubbles), W = (T + 2) & ~1ull;
    return 3 * N * 16 + 2 * W * 8 + (2 * (n_unitigs + 1) + 3 * N + 2 * T * kBlocksTile + 2 * T + 4) * 4;
}

// All of them: n_bubbles in 1 .. 2^30 - 1, n_unitigs below 2^30, the same scratch (16-byte aligned, blocks_scratch_bytes), one stream.
// passes 1 - 2 behind the memsets: the error word (BlocksScratch::err[0]) is final when the stream has run them
hipError_t launch_blocks_link(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_phase* phase, uint64_t n_phase, uint64_t n_unitigs, uint64_t min_phase, void* scratch,
                              hipStream_t stream);
// passes 3 - 4
hipError_t launch_blocks_rank(uint64_t n_bubbles, uint64_t n_unitigs, void* scratch, hipStream_t stream);
// passes 5 - 7: the number of entries lies in offs_s[tiles] when the stream has run them (n_bubbles, or the lists were none that blocks_check passes)
hipError_t launch_blocks_count(uint64_t n_bubbles, uint64_t n_unitigs, void* scratch, hipStream_t stream);
// pass 8: `out` has room for n_bubbles entries
hipError_t launch_blocks_place(uint64_t n_bubbles, uint64_t n_unitigs, void* scratch, bgr_block_entry* out, hipStream_t stream);

}  // namespace bgr

#endif
