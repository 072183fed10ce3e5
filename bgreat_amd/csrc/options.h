// options.h -- process-wide tuning and diagnostic options of the library.  Nothing in the library reads the environment: a host sets an
// option through bgr_set_option() (the CLI: --set name=value), before the objects that look at it are created.  Table: INTEGRATION.md 5.
#ifndef BGREAT_AMD_OPTIONS_H
#define BGREAT_AMD_OPTIONS_H

#include <stdint.h>
#include <string.h>

#include <atomic>

namespace bgr {

struct Option {
    const char* name;
    std::atomic<int64_t> value;
    int64_t lo, hi;
    const char* what;
};

// (a function-local table: one instance per process, whichever translation unit asks first)
inline Option* option_table(size_t* n) {
    static Option t[] = {
        {"timing", {0}, 0, 1, "per-stage timing lines on stderr (pipeline, text calls, index build)"},
        {"blocking_sync", {0}, 0, 1, "aligners wait for their stream with a blocking event (the thread sleeps) instead of spinning"},
        {"numa", {1}, 0, 1, "bgr_align_all pins its threads to the NUMA node of the devices they feed when all share one"},
        {"workers_per_device", {0}, 0, 16, "bgr_align_all: stream workers per device (0 = default: 2)"},
        {"extra_sets", {-1}, -1, 32, "bgr_align_all: staging sets beyond one per worker (-1 = default)"},
        {"fastq_gather", {1}, 0, 1, "FASTQ pieces cross PCIe without their '+' and quality lines"},
        {"overlap_streams", {4}, 2, 4, "bgr_align_batch of >= 512 k reads: internal streams"},
        {"huge_pinned", {1}, 0, 1, "bgr_host_alloc: buffers of 2 MB and more from huge-page mappings registered with the runtime"},
        {"exh_filter", {1}, 0, 1, "exhaustive mode probes large key tables through the minimizer filter"},
        {"build_filter", {-1}, -1, 2, "index build: filter in front of the key table: -1 by table size, 0 none, 1 one hash, 2 minimizer-blocked (forced onto small graphs by tests)"},
        {"build_jump", {1}, 0, 1, "index build: the jump index of the greedy anchor scan (graph_layout.h) where a graph qualifies: 1 = build it, 0 = none"},
        {"test.jump_drop", {0}, 0, INT64_MAX, "test hook: index build: every N-th sampled (k-1)-mer is left out of the jump index (the index is a hint: results must not change)"},
        {"poison_device_buffers", {0}, 0, 1, "diagnostic: every new device buffer is filled with a pattern (a kernel that reads what nothing wrote shows in any run)"},
        {"test.bases_cap", {0}, 0, INT64_MAX, "test hook: bases per batch of bgr_align_all (walks the cut of large batches with small inputs)"},
        {"test.lanes_on_one_device", {0}, 0, 1, "test hook: every lane of a split run / every device of --gpus N is device 0 (a one-GPU box walks the N-device code)"},
        {"test.wide_keys", {0}, 0, 1, "test hook: index build: every graph gets the two-word key layout of k > 32 (and the kernel that reads it), whatever its k"},
        {"test.links_capacity", {0}, 0, INT64_MAX, "test hook: slots of the table of links an aligner allocates when link counting is enabled (0 = from the graph's bound): a table that can fill"},
        {"test.triples_capacity", {0}, 0, INT64_MAX, "test hook: slots of the table of triples an aligner allocates when triple counting is enabled (0 = from the graph's bound): a table that can fill"},
        {"test.variants_stage_bytes", {0}, 0, 64 << 20, "test hook: bytes of the staging piece through which one pileup table is added into another (0 = one kernel on one device, 64 MiB pieces across devices); any value takes the staged way on one device too"},
        {"test.count_with_path_stats", {0}, 0, 1, "test hook: bgr_aligner_path_stats also queues every enabled counting kernel (abundance, links, triples, pileup) once over the rows the result buffers hold at that time, the read characters from its reads buffer: rows a test wrote there itself"},
        {"test.keep_rows", {0}, 0, 1, "test hook: a mapping launch (every route) sizes its buffers, makes its planes, queues the counting kernels and formats its text as ever, but runs none of the mapping passes: the result buffers keep the rows they hold, which a test wrote there itself behind a first launch of the same reads (another n_reads or arena size: BGR_E_ARG)"},
        {"test.text_epoch", {0}, 0, 0x3FFFFF, "test hook: the epoch the text form's chains start from when their state is (re)allocated (walks the 22-bit wrap with a few pieces)"},
    };
    *n = sizeof(t) / sizeof(t[0]);
    return t;
}
inline Option* find_option(const char* name) {
    size_t n;
    Option* t = option_table(&n);
    for (size_t i = 0; i < n; ++i)
        if (strcmp(t[i].name, name) == 0) return &t[i];
    return nullptr;
}
inline int64_t opt(const char* name) {
    Option* o = find_option(name);
    return o ? o->value.load(std::memory_order_relaxed) : 0;
}

}  // namespace bgr

#endif
