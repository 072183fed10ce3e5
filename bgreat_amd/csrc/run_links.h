// run_links.h -- how a whole run on a graph with bgr_graph_links_enable (pipeline.cpp, host code that knows the device side only through the
// C-ABI) reaches the switch and the objects that hold the link counts (capi.hip: the aligners' tables on the device, the run's totals in the
// graph object).  As run_abundance.h: capi.hip fills the table below when the library is loaded and pipeline.cpp calls through it, so it needs
// no symbol beyond the ones it already used -- a build of pipeline.cpp against another implementation of the C-ABI leaves the table empty
// and no run of it counts links.
#ifndef BGREAT_AMD_RUN_LINKS_H
#define BGREAT_AMD_RUN_LINKS_H

#include "../../include/bgreat_gpu.h"

namespace bgr {

struct RunLinks {
    bool (*wanted)(const bgr_graph* g);           // the graph's switch: this run counts unitig abundance and links
    void (*begin)(bgr_graph* g);                  // a new run: the totals of the one before are gone, whatever becomes of this one
    int (*enable)(bgr_aligner* a);                // every launch of this aligner counts
    int (*collect)(bgr_graph* g, bgr_aligner* a); // the aligner's table (its stream waited for) joins the run's totals in the graph
    void (*end)(bgr_graph* g, bool ok);           // totals only of a run that ended well
};
extern RunLinks g_run_links;  // pipeline.cpp; all null until capi.hip has registered

}  // namespace bgr

#endif
