// run_abundance.h -- how a whole run with bgr_run_options.abundance (pipeline.cpp, host code that knows the device side only through the
// C-ABI) reaches the objects that hold the counts (capi.hip: the aligners' tables on the device, the run's totals in the graph object).
// capi.hip fills the table below when the library is loaded; pipeline.cpp calls through it, so it needs no symbol beyond the ones it already
// used -- a build of pipeline.cpp against another implementation of the C-ABI leaves the table empty and refuses such a run.
#ifndef BGREAT_AMD_RUN_ABUNDANCE_H
#define BGREAT_AMD_RUN_ABUNDANCE_H

#include "../../include/bgreat_gpu.h"

namespace bgr {

struct RunAbundance {
    void (*begin)(bgr_graph* g);                  // a new run: the totals of the one before are gone, whatever becomes of this one
    int (*enable)(bgr_aligner* a);                // every launch of this aligner counts
    int (*collect)(bgr_graph* g, bgr_aligner* a); // the aligner's table (its stream waited for) joins the run's totals in the graph
    void (*end)(bgr_graph* g, bool ok);           // totals only of a run that ended well
};
extern RunAbundance g_run_abundance;  // pipeline.cpp; all null until capi.hip has registered

}  // namespace bgr

#endif
