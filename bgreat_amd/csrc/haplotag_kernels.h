// haplotag_kernels.h -- launch interface of haplotag_kernels.hip: the tags (bgr_read_tag in include/bgreat_gpu.h has the definition) of the rows
// of a greedy or anchors launch, from a tag table resident on the device.  The per-row function is haplotag_device.h's, which the tagged GAF
// kernels (text_gaf.hip) share.
#ifndef BGREAT_AMD_HAPLOTAG_KERNELS_H
#define BGREAT_AMD_HAPLOTAG_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bgreat_gpu.h"

namespace bgr {

// out[i] = the tag of read i's row (zeros: not mapped, or a row that is not wholly inside the arena's arena_ints); one 16-lane group per read
hipError_t launch_haplotags(const uint32_t* table, uint64_t n_unitigs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n_reads, bgr_read_tag* out,
                            hipStream_t stream);

}  // namespace bgr

#endif
