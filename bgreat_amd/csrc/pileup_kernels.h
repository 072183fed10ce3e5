// pileup_kernels.h -- launch interface of pileup_kernels.hip: per-base depth and mismatches on the unitigs of a greedy or anchors launch
// (bgr_pileup_base in include/bgreat_gpu.h has the definition).
#ifndef BGREAT_AMD_PILEUP_KERNELS_H
#define BGREAT_AMD_PILEUP_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "graph_layout.h"

namespace bgr {

// The table of one aligner, T = bases of the graph (sum of the unitig lengths), n = its unitigs, all words 32 bits wide:
//   alt    [4 T]     base b = base_offs[id] + pos owns four words, one per read code A C G T: reads that differ from the unitig there.  The word of
//                    the unitig's own base can receive nothing that way and counts the reads with a character outside ACGT (N) instead;
//   delta  [T + n]   unitig id owns len + 1 words from base_offs[id] + id - 1 on: +1 where a read's stretch begins, -1 (mod 2^32) behind its end;
//                    the depth at pos is the running sum of the words 0 .. pos, taken mod 2^32;
//   tail   [2]       one u64: mapped rows whose path spells no walk.
inline uint64_t pileup_alt_words(uint64_t total_bases) { return 4 * total_bases; }
inline uint64_t pileup_delta_words(uint64_t total_bases, uint64_t n_unitigs) { return total_bases + n_unitigs; }
inline uint64_t pileup_table_bytes(uint64_t total_bases, uint64_t n_unitigs) {
    return ((pileup_alt_words(total_bases) + pileup_delta_words(total_bases, n_unitigs) + 1) / 2) * 8 + 8;
}
inline uint64_t pileup_tail_byte(uint64_t total_bases, uint64_t n_unitigs) { return pileup_table_bytes(total_bases, n_unitigs) - 8; }

const uint32_t kPileupLanes = 16;   // lanes that share one read

// where the kernel finds a read's characters
struct PileupReads {
    const uint8_t* ascii = nullptr;     // ASCII: read r at ascii + read_offs[r] (src_off null) or at ascii + src_off[r] (reads scattered in a text)
    const uint32_t* src_off = nullptr;
    uint64_t ascii_bytes = 0;           // bytes of the buffer at `ascii`
    const uint64_t* fw3 = nullptr;      // ascii null: the 2-bit planes (read_pack.h), read r at word (read_offs[r] >> 5) + r
    const uint64_t* nmw = nullptr;
    const uint32_t* hasn = nullptr;
};

// base_offs: u64[n_unitigs + 2], base_offs[id] = sum of the lengths of the unitigs 1 .. id - 1 (base_offs[n_unitigs + 1] = T); table as above,
// added into.  arena_ints: ints the arena buffer holds (a row that would end beyond it is skipped).  Launches nothing for zero reads.
// table_fwd: null, or a second table of the same layout and size that receives the forward observations only (an occurrence whose read, as given
// in the input, is collinear with the strand the unitig file spells); its tail stays 0.  Null launches the kernel as it is without the switch.
hipError_t launch_pileup(const BgrDeviceGraph& g, uint64_t n_unitigs, uint64_t total_bases, const uint2* results, const int32_t* arena, uint64_t arena_ints,
                         const uint64_t* read_offs, uint32_t n_reads, const PileupReads& reads, const uint64_t* base_offs, uint32_t* table, uint32_t* table_fwd, uint32_t num_cus,
                         hipStream_t stream);

}  // namespace bgr

#endif
