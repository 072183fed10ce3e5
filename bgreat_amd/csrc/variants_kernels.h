// variants_kernels.h -- launch interface of variants_kernels.hip: SNV sites on the unitigs, called from one pileup table where it lies in HBM
// (bgr_variant_site in include/bgreat_gpu.h has the definition), and the sum of two pileup tables on one device.
#ifndef BGREAT_AMD_VARIANTS_KERNELS_H
#define BGREAT_AMD_VARIANTS_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bgreat_gpu.h"
#include "graph_layout.h"
#include "pileup_kernels.h"
#include "variants_host.h"

namespace bgr {

// The input is one table as pileup_kernels.h lays it out (alt[4 T], delta[T + n]), base_offs, and the graph's 2-bit seq / meta for the unitig's own
// letter.  The depth at (id, pos) is the running sum of the unitig's delta words 0 .. pos.
//
// THE SCAN NEEDS NO SEGMENTATION.  Every occurrence of a unitig in a read's path adds +1 and -1 (mod 2^32) inside that unitig's own len + 1 words,
// so the words of every unitig sum to 0 mod 2^32, and the flat running sum over all T + n words, taken mod 2^32, equals the per-unitig running
// sum at every word: what the unitigs in front contribute is 0.  (tests/test_variants_host.py checks the identity against the per-unitig sums.)
//
// The passes, each its own launch on the caller's stream (no workgroup ever waits for another), over tiles of BGR_VARIANTS_TILE delta words:
//   1  tile sums      sums[t] = sum of the tile's delta words
//   2  scan           carry[t] = sum of sums[0 .. t - 1], one workgroup
//   3  classify       every tile rescans its words from carry[t]; word index -> (id, pos) by one binary search per tile in base_offs[id] + id - 1
//                     and a walk from there; the extra word of a unitig (pos == len) is skipped; a base with depth >= min_depth reads its four
//                     alt words and the unitig's letter and is classified (variants_passing, variants_host.h); counts[t] = the tile's sites
//   4  scan           offs[t] = sum of counts[0 .. t - 1], offs[tiles] = the number of sites
//   5  emit           pass 3 again, writing each site's 32-byte record at offs[t] + its rank inside the tile
// The records come out in (unitig, pos) order by construction: no sort, no atomics on the output, and the number is known before pass 5 runs.
// Bytes from HBM per base: 4 (pass 1) + 2 x (4 + 16 for a covered base) + the 2-bit letter.
const uint32_t kVariantsTile = BGR_VARIANTS_TILE;
const uint32_t kVariantsThreads = 256;   // each thread owns kVariantsTile / kVariantsThreads = 8 consecutive words

inline uint64_t variants_tiles(uint64_t total_bases, uint64_t n_unitigs) { return (pileup_delta_words(total_bases, n_unitigs) + kVariantsTile - 1) / kVariantsTile; }
// scratch of one call: u64 carry[tiles + 1], u64 offs[tiles + 1], u32 sums[tiles], u32 counts[tiles]; with strands behind them the forward table's
// u64 carry_f[tiles + 1], u32 sums_f[tiles] (rounded up to 8 bytes)
inline uint64_t variants_scratch_bytes(uint64_t tiles, bool strands) { return (tiles + 1) * 16 + tiles * 8 + (strands ? (tiles + 1) * 8 + ((tiles + 1) / 2) * 8 : 0); }
inline const uint64_t* variants_total_word(const void* scratch, uint64_t tiles) { return static_cast<const uint64_t*>(scratch) + (tiles + 1) + tiles; }   // offs[tiles]

// table_fwd: null, or a forward table next to the total one (bgr_variant_strand_site).  With it pass 1 sums both difference arrays (a grid of
// tiles x 2), pass 2 scans both arrays of sums (two workgroups), passes 3 and 5 rescan both tables' words, read the forward alt words of a base
// that has a candidate allele, apply variants_strand_passing (variants_host.h) and write 64-byte records.  The forward words of a unitig sum to 0
// as the total's do: the forward scan runs flat too.  Still five launches, no sort, no atomics on the output, no workgroup waits for another.
// Without it prm.min_alt_strand is ignored.  scratch: variants_scratch_bytes(tiles, table_fwd != null).
// passes 1 - 4: the number of sites lies in *variants_total_word(scratch, tiles) when the stream has run them.  Launches nothing for an empty graph.
// after: null, or four events, recorded one behind each launch.
hipError_t launch_variants_count(const BgrDeviceGraph& g, uint64_t n_unitigs, uint64_t total_bases, const uint32_t* table, const uint32_t* table_fwd,
                                 const uint64_t* base_offs, const bgr_variant_strand_params& prm, void* scratch, hipStream_t stream, hipEvent_t* after);
// pass 5, behind launch_variants_count on the same stream with the same arguments: `out` has room for the number of sites (bgr_variant_site
// records, with table_fwd bgr_variant_strand_site records)
hipError_t launch_variants_emit(const BgrDeviceGraph& g, uint64_t n_unitigs, uint64_t total_bases, const uint32_t* table, const uint32_t* table_fwd,
                                const uint64_t* base_offs, const bgr_variant_strand_params& prm, const void* scratch, void* out, hipStream_t stream);
// the passes' scan by itself (passes 2 and 4 as they stand: one workgroup): out[t] = in[0] + .. + in[t - 1] for t = 0 .. n, 64-bit.  Other compactions
// (bubbles_kernels.hip) scan their tile counts with it.
hipError_t launch_variants_scan(const uint32_t* in, uint64_t n, uint64_t* out, hipStream_t stream);
// dst[i] += src[i] (mod 2^32) over n_words 32-bit words; with tail_u64 the last two words of both are one u64 counter (the table's tail) and are
// added as such.  Both on the device of `stream`; dst and src 16-byte aligned.
hipError_t launch_pileup_add(uint32_t* dst, const uint32_t* src, uint64_t n_words, bool tail_u64, uint32_t num_cus, hipStream_t stream);

}  // namespace bgr

#endif
