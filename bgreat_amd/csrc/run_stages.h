// run_stages.h -- the rules by which a whole run (run_counts.h) walks its counting features, as plain C++: which features the graph's sticky
// switches imply, and in which order the features end and what a failure among them does.  No HIP and no object of the C-ABI in here (the
// handles stay opaque), so that a program without either drives the rules with stages of its own (tools/run_stages_main.cpp); the table of
// the real stages is capi_abundance.hip's.
#ifndef BGREAT_AMD_RUN_STAGES_H
#define BGREAT_AMD_RUN_STAGES_H

#include "run_counts.h"

namespace bgr {

// One counting feature of a run.  `tier` is when it ends: the end walks the table once per tier, in the table's order within a tier.
enum { kTierAbundance = 0, kTierTables = 1, kTierDerived = 2, kTierPileup = 3, kTiers = 4 };
struct RunStage {
    uint32_t bit;                                    // the stage takes part in a run whose `what` has it
    void (*begin)(bgr_graph* g);                     // what the run before left is gone
    int (*enable)(bgr_aligner* a, uint32_t what);    // null: no kernel behind the aligner's launches
    int (*collect)(bgr_graph* g, bgr_aligner* a);    // null: nothing of an aligner's joins the run's totals
    int (*end)(bgr_graph* g, bool ok);               // totals only with ok, and only when it returns BGR_OK; with false it forgets and returns BGR_OK
    int tier;
};

// A run's end.  The stages end in order with `ok`; after the first one that fails every later one ends with false, and every one that has ended
// by then -- the failed one included -- ends again with false: a failed run leaves no totals.  The first failure's code is returned.  Only the
// last tier's failure is its own (the pileup's BGR_E_CAPACITY: a depth may have wrapped, the other totals are as good as they were).
inline int end_stages(const RunStage* st, int n, bgr_graph* g, uint32_t what, bool ok) {
    int rc = BGR_OK;
    for (int tier = 0; tier < kTiers; ++tier)
        for (int i = 0; i < n; ++i) {
            if (st[i].tier != tier || !(what & st[i].bit)) continue;
            const int r = st[i].end(g, ok && rc == BGR_OK);
            if (r == BGR_OK || rc != BGR_OK) continue;
            rc = r;
            if (tier == kTierPileup) continue;
            for (int j = 0; j < n; ++j)
                if ((what & st[j].bit) && (st[j].tier < tier || (st[j].tier == tier && j <= i))) (void)st[j].end(g, false);
        }
    return rc;
}

// The graph's sticky switches as the mask of what a run counts: haplotypes imply blocks, blocks imply phase, phase implies bubbles and triples,
// bubbles imply links, variants imply the pileup, strands count only next to the pileup or variants switch they belong to, and whatever is
// counted implies abundance.
struct RunSwitches { bool links, bubbles, triples, phase, blocks, haplotypes, pileup, variants, pileup_strands, variants_strands, recompact; };
inline uint32_t counts_wanted(const RunSwitches& s) {
    const bool blocks = s.blocks || s.haplotypes, phase = s.phase || blocks, bubbles = s.bubbles || phase;
    uint32_t what = 0;
    if (s.links || bubbles) what |= kCountLinks;
    if (bubbles) what |= kCountBubbles;
    if (s.triples || phase) what |= kCountTriples;
    if (phase) what |= kCountPhase;
    if (blocks) what |= kCountBlocks;
    if (s.haplotypes) what |= kCountHaplotypes;
    if (s.pileup || s.variants) what |= kCountPileup;
    if (s.variants) what |= kCountVariants;
    if ((s.pileup && s.pileup_strands) || (s.variants && s.variants_strands)) what |= kCountStrands;
    if (s.recompact) what |= kCountRecompact;   // (it keeps unitigs by the abundance totals and counts nothing of its own)
    return what ? what | kCountAbundance : 0;
}

}  // namespace bgr

#endif
