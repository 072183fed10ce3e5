// bubbles_kernels.h -- launch interface of bubbles_kernels.hip: the bubbles of the graph that a set of counted links spans (bgr_bubble in
// include/bgreat_gpu.h has the definition; bubbles_host.h the rule), called where the links lie in HBM.
#ifndef BGREAT_AMD_BUBBLES_KERNELS_H
#define BGREAT_AMD_BUBBLES_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bgreat_gpu.h"
#include "bubbles_host.h"

namespace bgr {

// The input is an array of {u64 key, u64 count} pairs (links_pack's key, links_kernels.h), key 0 = an empty pair: an aligner's live table
// (links_capacity pairs, mostly empty) and a dense uploaded list have this shape, so one set of kernels serves both.
//
// The passes, each its own launch on the caller's stream (no workgroup ever waits for another), the last three over tiles of BGR_BUBBLES_TILE
// oriented ids o(x) = 2 (|x| - 1) + (x < 0):
//   1  adjacency   one thread per pair: a pair with count >= min_link is the oriented edge from -> to and, unless to == -from, its strand mate
//                  -to -> -from; per edge one 32-bit atomicAdd on deg[o(from)], and when it returns r < 2 the pair {to, count} goes into successor
//                  slot r of `from`.  A third and later successor only counts.  in(x) is not kept: it is as large as out(-x).
//   2  count       every oriented id is classified (bubble_at, bubbles_host.h); counts[t] = the tile's bubbles
//   3  scan        offs[t] = sum of counts[0 .. t - 1], offs[tiles] = the number of bubbles: the variants' scan as it stands, one workgroup
//   4  emit        pass 2 again, writing each 48-byte record at offs[t] + its rank inside the tile
// The records come out in (|source|, source < 0) order by construction: no sort, no atomics on the output, the number is known before pass 4 runs.
// Which of its two successors took slot 0 depends on the order the atomics arrived in; bubble_at orders the branches, so it shows nowhere.
// A key that names a unitig outside 1 .. n_unitigs adds nothing (no aligner writes one; the C-ABI refuses such a list before it is uploaded).
const uint32_t kBubblesTile = BGR_BUBBLES_TILE;
const uint32_t kBubblesThreads = 256;   // each thread owns kBubblesTile / kBubblesThreads = 4 consecutive oriented ids

inline uint64_t bubbles_tiles(uint64_t n_unitigs) { return (2 * n_unitigs + kBubblesTile - 1) / kBubblesTile; }
// scratch of one call, in this order: u64 cnt[4 n], u64 offs[tiles + 1 or + 2], i32 to[4 n], u32 deg[tiles x tile] (whole tiles: the tail reads as 0),
// u32 counts[tiles] -- 56 bytes per unitig: 222 MB on the chr1-scale graph's 3 966 085
struct BubblesScratch {
    uint64_t* cnt; uint64_t* offs; int32_t* to; uint32_t* deg; uint32_t* counts;
    BubblesScratch(void* p, uint64_t n) {
        const uint64_t tiles = bubbles_tiles(n);
        cnt = static_cast<uint64_t*>(p); offs = cnt + 4 * n;
        to = reinterpret_cast<int32_t*>(offs + ((tiles + 2) & ~1ull));   // (offs rounded up to an even number of words: deg stays 16-byte aligned for its dwordx4 loads)
        deg = reinterpret_cast<uint32_t*>(to + 4 * n); counts = deg + tiles * kBubblesTile;
    }
};
inline uint64_t bubbles_scratch_bytes(uint64_t n_unitigs) {
    const uint64_t tiles = bubbles_tiles(n_unitigs);
    return 4 * n_unitigs * 8 + ((tiles + 2) & ~1ull) * 8 + 4 * n_unitigs * 4 + tiles * kBubblesTile * 4 + tiles * 4;
}
inline const uint64_t* bubbles_total_word(const void* scratch, uint64_t n_unitigs) { return BubblesScratch(const_cast<void*>(scratch), n_unitigs).offs + bubbles_tiles(n_unitigs); }

// passes 1 - 3 (behind a memset of deg on the same stream): the number of bubbles lies in *bubbles_total_word(scratch, n_unitigs) when the stream
// has run them.  pairs: 16-byte aligned, n_pairs of them (0: no pass 1).  Launches nothing for n_unitigs == 0.  after: null, or three events,
// recorded one behind each launch.
hipError_t launch_bubbles_count(const unsigned long long* pairs, uint64_t n_pairs, uint64_t n_unitigs, uint64_t min_link, void* scratch, hipStream_t stream, hipEvent_t* after);
// pass 4, behind launch_bubbles_count on the same stream with the same scratch: `out` has room for the number of bubbles
hipError_t launch_bubbles_emit(uint64_t n_unitigs, const void* scratch, bgr_bubble* out, hipStream_t stream);

}  // namespace bgr

#endif
