// inside_kernels.h -- launch interface of inside_kernels.hip: the fallback pass of greedy mode over the reads the mapping passes left without an
// anchor (bgr_aligner_inside_enable in include/bgreat_gpu.h has the definition; inside_index.h the table it probes).
#ifndef BGREAT_AMD_INSIDE_KERNELS_H
#define BGREAT_AMD_INSIDE_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inside_index.h"
#include "pileup_kernels.h"

namespace bgr {

const uint32_t kInsideLanes = 16;          // lanes that share one read
const uint32_t kInsideMaxReadLen = 32000;  // what four reads' words fit a workgroup's 64 KiB of LDS with; the greedy kernels take no longer read either

// What the pass reads and writes of a mapping launch: the rows (results, arena: `arena_cap` ints, of which the first `arena_own` belong to the
// waves of the first pass by number and cursor[0] hands out the rest; cursor[1] = the overflow word), the reads where the launch has them.
struct InsideLaunch {
    uint2* results;
    int32_t* arena;
    uint32_t* cursor;
    uint32_t arena_cap, arena_own;
    const uint64_t* read_offs;
    uint32_t n_reads, max_read_len, max_mismatch;
    PileupReads reads;
};

// Behind the mapping passes, on their stream: every read with status NOANCHOR and at least k characters gets the row [s, +-id] and status ALIGNED
// when the first valid candidate of its selected windows says so; *count += the reads mapped.  Launches nothing for zero reads.
hipError_t launch_inside(const BgrDeviceGraph& g, const BgrInsideEntry* table, uint64_t slots, const InsideLaunch& io, unsigned long long* count, uint32_t num_cus,
                         hipStream_t stream);

}  // namespace bgr

#endif
