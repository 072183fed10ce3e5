// recompact_kernels.h -- launch interface of recompact_kernels.hip: a kept subset of the graph's unitigs compacted into maximal non-branching chains
// and spelled from the 2-bit store where it lies in HBM (bgr_chain in include/bgreat_gpu.h has the definition; recompact_host.h the host's checks).
#ifndef BGREAT_AMD_RECOMPACT_KERNELS_H
#define BGREAT_AMD_RECOMPACT_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bgreat_gpu.h"
#include "graph_layout.h"

namespace bgr {

// A node is an oriented unitig, indexed by its order key o = 2 (u - 1) + (x < 0); N = 2 n nodes; the mate of node o is o ^ 1.  The end (k-1)-mers
// of a node are named by meta alone: (key index, orientation bit) with the bit 0 where the end is its own canonical form (a palindrome has both
// flags of its pair set: bit 0 either way) -- equal pairs are equal strings, so no pass hashes or compares sequence.
// The passes, each its own launch on the caller's stream (no workgroup ever waits for another; atomics only on the scratch table of pass 1, and the
// order in which they land shows nowhere: a count is a sum, an id is read only where the count is 1):
//   1  ends     one thread per kept node: count + 1 and id = x at the table entry of its BEGIN key
//   2  succ     one thread per kept node: out(x) = the count under its END key; succ[x] = the id there when out(x) == 1, out(-y) == 1 and |x| != |y|.
//               pred(o) = succ[o ^ 1] ^ 1 needs no array
//   3  rank     pointer jumping towards the heads over two buffers of {pointer, distance, done, smallest node of the span}, ceil(log2 N) rounds; a
//               node that has met no head lies on a ring and knows the ring's smallest node; the ring whose smallest node is forward is cut at the
//               link that enters it, its mate at the mate link (a thread writes its own succ word only); everything is ranked once more
//   4  place    tails hand their heads {size, tail}; a head is emitting when head < tail ^ 1; per node the emitting heads' sizes and a 1, both scanned
//               over the node index (a 64-bit scan over tiles of kRecompactTile items, this unit's own) to walk offsets and chain ordinals; every
//               node of an emitting chain writes its id and its piece {base offset in seq, length} at walk offset + distance; the piece lengths
//               scanned in walk order are the character offsets
//   5  spell    by output: a workgroup takes an aligned tile of kRecompactSpellTile bytes, finds the pieces of its first and last byte by binary
//               search once; a thread finds its 16 bytes' piece, gathers from seq, walks over piece borders, writes one aligned 16-byte store; the
//               tail goes out in bytes.  Nothing beyond the total is written.  No atomics
//   6  records  one thread per node; an emitting head writes its 32-byte record at its ordinal
// Every id is checked where it indexes meta or seq, every key index against the table, every place against the arrays: a violation sets a bit of the
// error word and the place is not written.
const uint32_t kRecompactTile = 1024;         // items per tile of the scans
const uint32_t kRecompactThreads = 256;       // each thread owns four consecutive items
const uint32_t kRecompactSpellTile = 16384;   // output bytes per workgroup of the spell pass
const uint32_t kRecompactNone = 0xFFFFFFFFu;
enum : uint32_t { kRecompactErrKey = 1, kRecompactErrId = 2, kRecompactErrSeq = 4, kRecompactErrPlace = 8, kRecompactErrLen = 16 };   // the error word's bits

inline uint64_t recompact_tiles(uint64_t items) { return (items + kRecompactTile - 1) / kRecompactTile; }
inline uint32_t recompact_rounds(uint64_t n_unitigs) { uint32_t r = 0; while ((1ull << r) < 2 * n_unitigs) ++r; return r; }

// scratch of one call (n unitigs, N = 2 n nodes, T = tiles of N + 1 items, Q = n_keys), one allocation, in this order:
//   uint4  sa[N], sb[N]                                           the ranking's two buffers
//   u64    hoff[N + 1], hord[N + 1], ioff[n + 1], pbase[n], tsum[T], toff[T + 1], words[2]
//   uint2  tab[2 Q], meta[N]
//   u32    succ[N], ring[N], hsize[N], hflag[N], plen[n];  i32 walk[n];  u8 keep[n]
// -- 169 bytes per unitig and 16 per key
struct RecompactScratch {
    uint4 *sa, *sb;
    uint64_t *hoff, *hord, *ioff, *pbase, *tsum, *toff, *words;
    uint2 *tab, *meta;
    uint32_t *succ, *ring, *hsize, *hflag, *plen;
    int32_t* walk;
    uint8_t* keep;
    RecompactScratch(void* p, uint64_t n, uint64_t n_keys) {
        const uint64_t N = 2 * n, T = recompact_tiles(N + 1);
        sa = static_cast<uint4*>(p); sb = sa + N;
        hoff = reinterpret_cast<uint64_t*>(sb + N); hord = hoff + N + 1; ioff = hord + N + 1; pbase = ioff + n + 1; tsum = pbase + n; toff = tsum + T; words = toff + T + 1;
        tab = reinterpret_cast<uint2*>(words + 2); meta = tab + 2 * n_keys;
        succ = reinterpret_cast<uint32_t*>(meta + N); ring = succ + N; hsize = ring + N; hflag = hsize + N; plen = hflag + N;
        walk = reinterpret_cast<int32_t*>(plen + n);
        keep = reinterpret_cast<uint8_t*>(walk + n);
    }
};
inline uint64_t recompact_scratch_bytes(uint64_t n_unitigs, uint64_t n_keys) {
    const uint64_t n = n_unitigs, N = 2 * n, T = recompact_tiles(N + 1);
    return 2 * N * 16 + (2 * (N + 1) + (n + 1) + n + T + (T + 1) + 2) * 8 + (2 * n_keys + N) * 8 + (4 * N + n) * 4 + n * 4 + n + 16;
}

// All of them: n_unitigs in 1 .. 2^30 - 1, the same scratch (16-byte aligned, recompact_scratch_bytes) with keep[] already in it (queued on the
// same stream), one stream; `dg` the graph on the stream's device.
// passes 1 - 2
hipError_t launch_recompact_links(const BgrDeviceGraph& dg, uint64_t n_unitigs, uint64_t n_keys, void* scratch, hipStream_t stream);
// pass 3
hipError_t launch_recompact_rank(uint64_t n_unitigs, uint64_t n_keys, void* scratch, hipStream_t stream);
// pass 4: hord[N] = the chains, hoff[N] = the walk's ints, ioff[n] = the characters, words[1] = the error word, all final when the stream has run them
hipError_t launch_recompact_place(const BgrDeviceGraph& dg, uint64_t n_unitigs, uint64_t n_keys, uint64_t total_bases, void* scratch, hipStream_t stream);
// pass 5: `out` is 16-byte aligned with room for `total` = ioff[n] bytes; walk_n = hoff[N]
hipError_t launch_recompact_spell(const BgrDeviceGraph& dg, uint64_t n_unitigs, uint64_t n_keys, uint64_t walk_n, uint64_t total, void* scratch, char* out, hipStream_t stream);
// pass 6: `out` has room for n_records = hord[N] records
hipError_t launch_recompact_records(uint64_t n_unitigs, uint64_t n_keys, void* scratch, bgr_chain* out, uint64_t n_records, hipStream_t stream);

}  // namespace bgr

#endif
