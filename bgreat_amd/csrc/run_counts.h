// run_counts.h -- how a whole run (pipeline.cpp, host code that knows the device side only through the C-ABI) reaches what the counting
// features keep: the graph's sticky switches, the aligners' tables on the device and the run's totals in the graph object (unitig abundance,
// links and their bubbles, triples and the bubbles' phase, blocks and haplotypes, the pileup with its SNV sites and strands: capi_abundance.hip,
// capi_links.hip (both count tables), capi_triples.hip (phase), capi_bubbles.hip, capi_blocks.hip, capi_haplotypes.hip, capi_pileup.hip,
// capi_variants.hip).  One unit of the library (capi_abundance.hip) fills the table below when the library is loaded; pipeline.cpp calls through
// it, so it needs no symbol beyond the ones it already used -- a build of pipeline.cpp against another implementation of the C-ABI
// (tests/sanitize_pipeline.cpp, tools/pipeline_bench.cpp) links as before, sees the table all null, counts nothing and refuses a run with
// bgr_run_options.abundance = 1.  Behind the five entries is one table of stages (capi_abundance.hip); the rules that walk it -- which switch
// implies which, in which order the stages end, what a failure does -- are run_stages.h's, plain C++ that tests/test_run_stages_host.py drives.
#ifndef BGREAT_AMD_RUN_COUNTS_H
#define BGREAT_AMD_RUN_COUNTS_H

#include "../../include/bgreat_gpu.h"

namespace bgr {

enum : uint32_t { kCountAbundance = 1, kCountLinks = 2, kCountPileup = 4, kCountVariants = 8, kCountStrands = 16, kCountBubbles = 32, kCountTriples = 64, kCountPhase = 128, kCountBlocks = 256, kCountHaplotypes = 512, kCountRecompact = 1024 };   // `what` a run counts
struct RunCounts {
    uint32_t (*wanted)(const bgr_graph* g);                        // the graph's sticky switches as a mask (links, triples and pileup imply abundance, bubbles imply links, phase implies bubbles and triples, blocks imply phase, haplotypes imply blocks)
    void (*begin)(bgr_graph* g, uint32_t what);                    // a new run: the totals of the one before are gone, whatever becomes of this one
    int (*enable)(bgr_aligner* a, uint32_t what);                  // every launch of this aligner counts
    int (*collect)(bgr_graph* g, bgr_aligner* a, uint32_t what);   // the aligner's tables (its streams waited for) join the run's totals: links, triples, pileup (+ variants), abundance, in that order
    int (*end)(bgr_graph* g, uint32_t what, bool ok);              // totals only of a run that ended well: abundance, links, triples, the bubbles behind the links, the phase behind both, the blocks behind the phase, the haplotypes behind the blocks, then the pileup behind the abundance totals (BGR_E_CAPACITY when a depth may have wrapped)
    // haplotags count nothing and are no stage of the run: the graph's tag table while bgr_graph_haplotag_enable is on (else null), and the call that puts
    // it on an aligner's device, whose GAF lines are tagged from then on; a run's host formatter tags from the same table (haplotag_host.h)
    const uint32_t* (*haplotag_table)(const bgr_graph* g, uint64_t* n_rows);
    int (*haplotag_enable)(bgr_aligner* a, const uint32_t* table, uint64_t n_rows);
    // the cs:Z: field of GAF lines, the same way: the graph's switch (bgr_graph_gaf_cs_enable) as 1 or 0, and the call that sets an aligner's; the host
    // formatter writes the same bytes (record_format.h)
    int (*gaf_cs_wanted)(const bgr_graph* g);
    int (*gaf_cs_enable)(bgr_aligner* a, int on);
    // the inside pass (bgr_graph_inside_enable), the same way: the graph's switch as 1 or 0, the start of a run's count, the call that sets an
    // aligner's switch (the index goes onto its device), and the call that adds a finished aligner's count to the run's
    int (*inside_wanted)(const bgr_graph* g);
    void (*inside_begin)(bgr_graph* g);
    int (*inside_enable)(bgr_aligner* a, int on);
    int (*inside_collect)(bgr_graph* g, bgr_aligner* a);
    // the paths of exhaustive mode as output (bgr_graph_exhaustive_paths_enable), the same way: the graph's switch as 1 or 0 and the call that sets an
    // aligner's; the host formatter reads the rows without their end offset by the same rule (record_format.h)
    int (*exhaustive_paths_wanted)(const bgr_graph* g);
    int (*exhaustive_paths_enable)(bgr_aligner* a, int on);
};
extern RunCounts g_run_counts;   // pipeline.cpp; all null until the library's C-ABI units have registered

}  // namespace bgr

#endif
