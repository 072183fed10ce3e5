// exhaustive_rows_kernels.hip -- the rows of an exhaustive launch as the readers of greedy rows take them (exhaustive_rows_kernels.h has the rule and
// the reason): one kernel behind a SETTLED exhaustive launch writes, per read, the result pair with its row one int shorter -- or empty where the row is
// not a whole [begin, ids .., end] row inside the arena -- into a buffer of the aligner's own.  The abundance, links, triples, pileup, path-stats,
// path-diffs, haplotag and GAF kernels then read that buffer where they would read `results`; the arena is the launch's, untouched.
//
// One read per thread: an 8-byte load, four integer operations, an 8-byte store.  It moves 16 bytes per read (4 MB for a launch of 262 144 reads), so
// its time is the launch latency; a grid-stride loop over at most 4 096 workgroups keeps the grid inside 32 bits for any n_reads.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "exhaustive_rows_kernels.h"

__global__ void __launch_bounds__(256) bgr_exhaustive_rows_kernel(const uint2* __restrict__ results, uint32_t n_reads, uint64_t arena_ints, uint2* __restrict__ view) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) view[r] = bgr::exhaustive_row_view(results[r], arena_ints);
}

namespace bgr {

hipError_t launch_exhaustive_rows(const uint2* results, uint32_t n_reads, uint64_t arena_ints, uint2* view, hipStream_t stream) {
    if (n_reads == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(4096, ((uint64_t)n_reads + 255) / 256);
    hipLaunchKernelGGL(bgr_exhaustive_rows_kernel, dim3(blocks), dim3(256), 0, stream, results, n_reads, arena_ints, view);
    return hipGetLastError();
}

}  // namespace bgr
