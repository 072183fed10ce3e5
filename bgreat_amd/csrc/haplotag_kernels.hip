// haplotag_kernels.hip -- bgr_aligner_haplotags: the tag of every read of a greedy / anchors launch (gfx950).  One kernel reads every mapped
// read's row [off, id_1 .. id_n] from (results, arena) and gathers one word of the tag table per id; no read characters, no strand, no offset,
// no graph, so one kernel serves every k.  Geometry as the links kernel's: sixteen lanes share a read (haplotag_device.h has the function and
// why it needs no atomics and no LDS).  Gather-bound: a path is a handful of ids, the table a few hundred KB to a few MB.
#include "haplotag_kernels.h"

#include "haplotag_device.h"

namespace bgr {
namespace {

__global__ void __launch_bounds__(256) bgr_haplotags_kernel(const uint32_t* table, uint32_t n_unitigs, const uint2* results, const int32_t* arena, u64 arena_ints, uint32_t n_reads,
                                                            uint4* out) {
    const uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, sub = threadIdx.x & 15;
    if (r >= n_reads) return;   // (the whole group)
    const uint2 res = results[r];
    const uint32_t np = res.y & 0xFFFFFFu;
    bgr_read_tag t = {0, 0, 0, 0};
    if (np >= 2 && (u64)res.x + np <= arena_ints) {   // mapped, and the row lies in the arena (as the counting kernels skip one that does not)
        const int32_t* ids = arena + res.x + 1;
        const uint32_t n = np - 1;
        const uint32_t first = sub < n ? haplotag_vote(table, n_unitigs, ids[sub]) : 0u;
        t = haplotag_group(table, n_unitigs, ids, n, first, sub);
    }
    if (sub == 0) out[r] = make_uint4(t.block, t.a, t.b, t.others);
}

}  // namespace

hipError_t launch_haplotags(const uint32_t* table, uint64_t n_unitigs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n_reads, bgr_read_tag* out,
                            hipStream_t stream) {
    static_assert(sizeof(bgr_read_tag) == 16, "four words per read, written as one uint4");
    if (n_reads == 0) return hipSuccess;
    if (!table || n_unitigs >= 0x80000000ull || n_reads > 0x0FFFFFFFu) return hipErrorInvalidValue;   // (16 n_reads threads are counted in 32 bits)
    hipLaunchKernelGGL(bgr_haplotags_kernel, dim3((n_reads + 15) / 16), dim3(256), 0, stream, table, (uint32_t)n_unitigs, results, arena, (u64)arena_ints, n_reads,
                       reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

}  // namespace bgr
