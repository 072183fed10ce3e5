// exhaustive_rows_kernels.h -- launch interface of exhaustive_rows_kernels.hip: the view through which everything that reads the rows of the greedy
// modes reads the rows of an exhaustive launch (bgr_aligner_exhaustive_paths_enable in include/bgreat_gpu.h has the definition).
//
// An exhaustive row is [begin offset, +-u_1 .. +-u_n, end offset] (alignerExhaustive.cpp:96-104, 193-201, 249-257): a greedy row with one more int
// behind it.  The view is a second array of result words, one {off, w} pair per read, that names the same ints of the same arena without the last one:
//     {off, (n - 1) | st << 24}   when (st & BGR_ST_MASK) == BGR_ST_ALIGNED, n >= 3 and off + n <= arena_ints (the sum in 64 bits),
//     {off, st << 24}             otherwise: an empty row with the status as stored
// with n = w & 0xFFFFFF and st = w >> 24 of the launch's own pair.  Nothing in `results` or the arena changes: a fetch still delivers the row with its
// end offset.  tests/exhaustive_rows_ref.py is the same rule in Python.
#ifndef BGREAT_AMD_EXHAUSTIVE_ROWS_KERNELS_H
#define BGREAT_AMD_EXHAUSTIVE_ROWS_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bgreat_gpu.h"
#include "graph_layout.h"

namespace bgr {

// one entry of the view from one result pair (the kernel's body, and what a host twin would call)
BGR_HD uint2 exhaustive_row_view(uint2 res, uint64_t arena_ints) {
    const uint32_t n = res.y & 0xFFFFFFu, st = res.y >> 24;
    const bool whole = (st & BGR_ST_MASK) == BGR_ST_ALIGNED && n >= 3 && (uint64_t)res.x + n <= arena_ints;
    uint2 v;
    v.x = res.x;
    v.y = (whole ? n - 1 : 0u) | (st << 24);
    return v;
}

// view[r] = exhaustive_row_view(results[r]) for r < n_reads: one read per thread, an 8-byte load and an 8-byte store, no atomics, no LDS.  `view` is a
// buffer of its own (n_reads pairs), so the launch can be repeated.  Launches nothing for zero reads.
hipError_t launch_exhaustive_rows(const uint2* results, uint32_t n_reads, uint64_t arena_ints, uint2* view, hipStream_t stream);

}  // namespace bgr

#endif
