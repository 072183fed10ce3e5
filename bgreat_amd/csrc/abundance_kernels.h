// abundance_kernels.h -- launch interface of abundance_kernels.hip: per-unitig reads / bases / k-mers of a greedy or anchors launch
// (bgr_run_options.abundance in include/bgreat_gpu.h has the definition), and the choice between the kernel's two forms.
#ifndef BGREAT_AMD_ABUNDANCE_KERNELS_H
#define BGREAT_AMD_ABUNDANCE_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "graph_layout.h"

namespace bgr {

const uint32_t kAbundanceFormGlobal = 1;  // form A: every add is a 64-bit atomic on the table in HBM
const uint32_t kAbundanceFormLds = 2;     // form B: a table of 32-bit counters per workgroup in LDS, flushed once with 64-bit atomics
const uint32_t kAbundanceLanes = 16;      // lanes that share one read (one unitig of a pass of sixteen each)
const uint64_t kAbundanceLdsMax = 160 * 1024;  // LDS one workgroup can have on gfx950

// Automatic choice: form B while a workgroup of it sees at least one read per this many unitigs of the graph.  B pays a fixed price per
// workgroup -- clearing and flushing 3 x (n_unitigs + 1) counters, one global atomic per counter that is not zero -- and saves the global
// atomics of the reads that meet in a counter.  Measured on an MI355X (tools/abundance_rate.py, profiles/abundance_rate.txt: 262 144 reads of
// 150 bp per launch, k = 31): on a graph of 6 388 unitigs, where a workgroup of B (512 of them) sees 0.08 reads per unitig, the kernel takes
// 0.038 ms in form B against 0.073 ms in form A (1 648 - 1 689 against 1 360 Mreads/s for the whole launch); on six unitigs that every read lands
// on, 0.025 ms against 6.8 ms -- form A serialises on a handful of addresses.  So B runs from one read per sixteen unitigs and workgroup on, which
// covers every table that fits the LDS at that launch size; below that (few reads on a table of thousands of counters: the clear and the flush are
// all a workgroup would do) nothing was measured and form A stays.  Graphs whose table fits no workgroup have form A only: 0.070 ms on 98 866
// unitigs, 0.060 ms on 3 966 085 (the chr1-scale shape, where almost no two adds of a launch meet).
const uint64_t kAbundanceLdsUnitigsPerRead = 16;

struct AbundancePlan {
    uint32_t form = kAbundanceFormGlobal, blocks = 0, threads = 256, lds_bytes = 0;
};

// A pure function of the numbers (no device): want = 0 automatic, 1 form A, 2 form B where its table fits a workgroup's LDS and its 32-bit counters
// cannot wrap.  The latter from the launch's size: a walk position lies on at most k occurrences of a path (each starts at least one base behind the
// one before and k - 1 bases in front of that one's end), so no counter of a launch receives more than k x total_bases -- form B needs that below 2^32
// (k = 31: launches up to 138 M bases; bgr_align_all's pieces hold 45 M), and a larger launch takes form A whatever the knob says.
inline AbundancePlan plan_abundance(uint64_t n_unitigs, uint32_t k, uint64_t n_reads, uint64_t total_bases, uint32_t num_cus, uint64_t lds_per_cu, uint32_t want) {
    AbundancePlan p;
    if (!num_cus) num_cus = 256;
    if (!lds_per_cu) lds_per_cu = kAbundanceLdsMax;
    const uint64_t table_bytes = 3 * 4 * (n_unitigs + 1), lds_fit = (lds_per_cu < kAbundanceLdsMax ? lds_per_cu : kAbundanceLdsMax) - 64;  // (a little slack, as the mapping kernels keep)
    bool lds = want != kAbundanceFormGlobal && table_bytes <= lds_fit && total_bases < (1ull << 32) / (k ? k : 1);
    if (lds) {   // 1024 threads = 64 reads in flight per workgroup; two workgroups per CU where two tables fit
        p.threads = 1024;
        const uint64_t per_cu = 2 * table_bytes <= lds_fit ? 2 : 1, groups = p.threads / kAbundanceLanes;
        uint64_t blocks = (n_reads + groups - 1) / groups;
        if (blocks > num_cus * per_cu) blocks = num_cus * per_cu;
        if (want == 0 && n_reads * kAbundanceLdsUnitigsPerRead < blocks * (n_unitigs + 1)) lds = false;
        else { p.form = kAbundanceFormLds; p.blocks = (uint32_t)blocks; p.lds_bytes = (uint32_t)table_bytes; }
    }
    if (!lds) {  // a grid-stride loop over the reads, sixteen per workgroup and turn
        p.form = kAbundanceFormGlobal;
        p.threads = 256;
        const uint64_t groups = p.threads / kAbundanceLanes;
        uint64_t blocks = (n_reads + groups - 1) / groups;
        if (blocks > (uint64_t)num_cus * 64) blocks = (uint64_t)num_cus * 64;
        p.blocks = (uint32_t)blocks;
        p.lds_bytes = 0;
    }
    return p;
}

// table: u64[n_unitigs + 1][3] = {reads, bases, kmers} per unitig id (row 0 unused), added into.  arena_ints: ints the arena buffer holds (a row
// that would end beyond it is skipped).  Launches nothing for zero reads.
// before the first launch of form B on the current device: lets a workgroup of the kernel have as much LDS as plan_abundance may give its table
hipError_t prepare_abundance(uint64_t lds_per_cu);
hipError_t launch_abundance(const BgrDeviceGraph& g, uint64_t n_unitigs, const uint2* results, const int32_t* arena, uint64_t arena_ints, const uint64_t* read_offs,
                            uint32_t n_reads, unsigned long long* table, const AbundancePlan& plan, hipStream_t stream);

}  // namespace bgr

#endif
