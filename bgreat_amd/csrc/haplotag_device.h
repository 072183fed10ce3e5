// haplotag_device.h -- the tag of one mapped read's row (bgr_read_tag, include/bgreat_gpu.h) by the sixteen lanes of a group, shared by the
// stand-alone kernel behind bgr_aligner_haplotags (haplotag_kernels.hip) and the tagged instances of the GAF formatter (text_gaf.hip).
// haplotag_host.h has the plain C++ twin, tests/haplotag_ref.py the definition.  Included behind device_common.h by .hip files only.
//
// Lane i takes id i of a pass of sixteen: one 4-byte gather from the table per id.  The smallest block among the votes is a min-reduction over
// the row of 16, the three counts are sums over it.  A row of at most sixteen ids keeps its votes in a register (`first`, which the caller hands
// in: the GAF walk holds the path's first sixteen ids in its lanes already); a longer row walks its ids from the seventeenth on a second time
// for the counts, once the minimum is known.  No atomics, no LDS, nothing between groups: the reductions are DPP row operations, which stay
// inside the sixteen lanes, so a group whose read is unmapped may skip the function while its neighbours in the wave run it -- but all sixteen
// lanes of a group call it together, with the same ids and n.
#ifndef BGREAT_AMD_HAPLOTAG_DEVICE_H
#define BGREAT_AMD_HAPLOTAG_DEVICE_H

#include "device_common.h"
#include "walk_lanes.h"

namespace bgr {
namespace {

// the vote of one path int: table[|id|] when |id| (in 64 bits: INT32_MIN is 2^31) is a unitig of the graph, else 0
__device__ __forceinline__ uint32_t haplotag_vote(const uint32_t* table, uint32_t n_unitigs, int32_t sid) {
    const u64 u = (u64)(sid < 0 ? -(int64_t)sid : (int64_t)sid);
    return u >= 1 && u <= n_unitigs ? table[u] : 0u;
}

// ids: id_1 .. id_n of the row (n >= 1); first: this lane's vote of the first pass, haplotag_vote(ids[sub]) for sub < n and 0 beyond.
// -> the tag, in every lane
__device__ __forceinline__ bgr_read_tag haplotag_group(const uint32_t* table, uint32_t n_unitigs, const int32_t* ids, uint32_t n, uint32_t first, uint32_t sub) {
    uint32_t best = first ? first >> 1 : 0xFFFFFFFFu;
    for (uint32_t j = 16 + sub; j < n; j += 16) {
        const uint32_t v = haplotag_vote(table, n_unitigs, ids[j]);
        if (v && (v >> 1) < best) best = v >> 1;
    }
    best = row16_min(best);
    bgr_read_tag t = {0, 0, 0, 0};
    if (best == 0xFFFFFFFFu) return t;   // (no vote in any lane: the whole group leaves)
    uint32_t a = 0, b = 0, o = 0;
    if (first) { if ((first >> 1) != best) o = 1; else if (first & 1u) b = 1; else a = 1; }
    for (uint32_t j = 16 + sub; j < n; j += 16) {
        const uint32_t v = haplotag_vote(table, n_unitigs, ids[j]);
        if (!v) continue;
        if ((v >> 1) != best) ++o; else if (v & 1u) ++b; else ++a;
    }
    t.block = best;
    t.a = row16_sum(a);
    t.b = row16_sum(b);
    t.others = row16_sum(o);
    return t;
}

}  // namespace
}  // namespace bgr

#endif
