// run_pileup.h -- how a whole run on a graph with bgr_graph_pileup_enable (pipeline.cpp, host code that knows the device side only through the
// C-ABI) reaches the switch and the objects that hold the per-base counts (capi.hip: the aligners' tables on the device, the run's totals in the
// graph object).  As run_links.h: capi.hip fills the table below when the library is loaded and pipeline.cpp calls through it, so it needs
// no symbol beyond the ones it already used -- a build of pipeline.cpp against another implementation of the C-ABI leaves the table empty
// and no run of it counts a pileup.
#ifndef BGREAT_AMD_RUN_PILEUP_H
#define BGREAT_AMD_RUN_PILEUP_H

#include "../../include/bgreat_gpu.h"

namespace bgr {

struct RunPileup {
    bool (*wanted)(const bgr_graph* g);           // the graph's switches (pileup, variants): this run counts unitig abundance and the pileup
    void (*begin)(bgr_graph* g);                  // a new run: the totals of the one before are gone, whatever becomes of this one
    int (*enable)(bgr_aligner* a);                // every launch of this aligner counts
    int (*collect)(bgr_graph* g, bgr_aligner* a); // the aligner's table (its stream waited for) joins the run's totals in the graph
    int (*end)(bgr_graph* g, bool ok);            // totals only of a run that ended well; BGR_E_CAPACITY when a depth may have wrapped (behind the abundance's end)
    bool (*variants)(const bgr_graph* g);         // the graph's variants switch (bgr_graph_variants_enable) is among what `wanted` answers for: the run calls SNV sites (--vcf)
    bool (*strands)(const bgr_graph* g);          // a strands switch (bgr_graph_pileup_strands_enable, bgr_graph_variants_strands_enable) is on as well (--strands)
    int (*enable_strands)(bgr_aligner* a);        // `enable`, and every launch also counts the forward observations in a second table
};
extern RunPileup g_run_pileup;  // pipeline.cpp; all null until capi.hip has registered

}  // namespace bgr

#endif
