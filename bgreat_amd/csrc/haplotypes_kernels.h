// haplotypes_kernels.h -- launch interface of haplotypes_kernels.hip: the two sequences every haplotype block stands for, spelled from the graph's
// 2-bit store where it lies in HBM (bgr_haplotype in include/bgreat_gpu.h has the definition; haplotypes_host.h the oriented ids and the checks).
#ifndef BGREAT_AMD_HAPLOTYPES_KERNELS_H
#define BGREAT_AMD_HAPLOTYPES_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bgreat_gpu.h"
#include "graph_layout.h"
#include "haplotypes_host.h"

namespace bgr {

// Every unitig lies in `seq` in both strands (graph_layout.h), so an oriented unitig is (base offset, length) and spelling is a scan plus a gather.
// The passes, each its own launch on the caller's stream (no workgroup ever waits for another; a launch never reads a word that another thread of
// the same launch writes):
//   1  items    an item is (entry, hap) at place 2 * first entry of its block + hap * size + index, so a block's A items precede its B items.
//               One thread per item: up to three pieces {base offset in seq, length} -- the whole source (index 0 only), the branch without its
//               first k - 1 bases, the sink without them --, the item's length (0 when the block is below min_block: its pieces are empty), 1 for the
//               A head of a kept block; the item's two junctions (source | branch, branch | sink) compared in the 2-bit store as two-word windows,
//               the bad ones added to one 64-bit counter (an atomic only where one differs)
//   2  scan     the lengths to 64-bit character offsets, the head counts to block ordinals: sums per tile of kHapTile items, one workgroup over
//               the tiles' sums, then offsets per tile (a 64-bit scan of this unit's own: a tile's sum of unitig lengths is not bounded by 2^32)
//   3  spell    by output: a workgroup takes an aligned tile of kHapSpellTile bytes and finds the items of its first and last byte by binary search
//               over the item offsets once (two LDS words); a thread finds its 16 bytes' item between them, gathers the characters from `seq`
//               ((word >> (62 - 2 (b & 31))) & 3 -> ACGT), walks forward over piece borders inside its 16 bytes, and writes one aligned 16-byte
//               store; the tail beyond the last whole 16 bytes goes out in bytes.  Nothing beyond the total is written.  No atomics
//   4  records  one thread per entry that heads a kept block writes the block's two 32-byte records at 2 * ordinal
// The host has checked both lists before any of this runs (haplotypes_check); the kernels check every id again where it indexes `meta`, every piece
// against the end of `seq`, and a place beyond the items or the records is not written: each sets a bit of the error word.
const uint32_t kHapTile = 1024;          // items per tile of the scan
const uint32_t kHapThreads = 256;        // each thread owns kHapTile / kHapThreads = 4 consecutive items
const uint32_t kHapSpellTile = 16384;    // output bytes per workgroup of the spell pass: 256 threads x 4 stores of 16 bytes
enum : uint32_t { kHapErrId = 1, kHapErrEntry = 2, kHapErrSeq = 4, kHapErrPlace = 8 };   // the error word's bits

inline uint64_t hap_tiles(uint64_t n_entries) { return (2 * n_entries + kHapTile - 1) / kHapTile; }

// scratch of one call (I = 2 n_entries items, T tiles), in this order: u64 pbase[3 I], ilen[I], ioff[I + 1], iord[I + 1], tsum[2 T], toff[2 (T + 1)],
// words[2] (the bad junctions, then the error word in the low half of the second); u32 plen[3 I], head[I] -- 64 bytes per item, 128 per entry
inline uint64_t hap_scratch_bytes(uint64_t n_entries) {
    const uint64_t I = 2 * n_entries, T = hap_tiles(n_entries);
    return (3 * I + I + 2 * (I + 1) + 2 * T + 2 * (T + 1) + 2) * 8 + (3 * I + I) * 4;
}
struct HapScratch {
    uint64_t *pbase, *ilen, *ioff, *iord, *tsum, *toff, *words;
    uint32_t *plen, *head;
    HapScratch(void* p, uint64_t n_entries) {
        const uint64_t I = 2 * n_entries, T = hap_tiles(n_entries);
        pbase = static_cast<uint64_t*>(p); ilen = pbase + 3 * I; ioff = ilen + I; iord = ioff + I + 1; tsum = iord + I + 1; toff = tsum + 2 * T; words = toff + 2 * (T + 1);
        plen = reinterpret_cast<uint32_t*>(words + 2); head = plen + 3 * I;
    }
};

// All of them: n_entries in 1 .. 2^30 - 1, the same scratch (16-byte aligned, hap_scratch_bytes), one stream; `dg` the graph on the stream's device.
// passes 1 - 2 behind the memsets of the two words, the lengths and the head counts: ioff[I] = the bytes of all sequences, iord[I] = the kept blocks, words[0] = the bad junctions,
// words[1] = the error word, all final when the stream has run them
hipError_t launch_hap_items(const BgrDeviceGraph& dg, uint64_t n_unitigs, uint64_t total_bases, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries,
                            uint64_t n_entries, uint64_t min_block, void* scratch, hipStream_t stream);
// pass 3: `out` is 16-byte aligned with room for `total` = ioff[I] bytes
hipError_t launch_hap_spell(const BgrDeviceGraph& dg, uint64_t n_entries, uint64_t total, void* scratch, char* out, hipStream_t stream);
// pass 4: `out` has room for n_records = 2 iord[I] records
hipError_t launch_hap_records(const bgr_block_entry* entries, uint64_t n_entries, uint64_t min_block, void* scratch, bgr_haplotype* out, uint64_t n_records, hipStream_t stream);

}  // namespace bgr

#endif
