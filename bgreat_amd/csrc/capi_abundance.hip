// capi_abundance.hip -- the C-ABI's unitig abundance (bgr_run_options.abundance in include/bgreat_gpu.h has the definition): the aligners'
// tables, the run's totals in the graph object, the writer; and the table through which a whole run (pipeline.cpp, run_counts.h) reaches
// every counting feature -- abundance is the one that all of them imply.
#include <cstdio>
#include <cstring>

#include "capi_internal.h"
#include "run_counts.h"
#pragma GCC visibility push(hidden)   // (the rules are no part of the interface; run_counts.h, above, is what pipeline.cpp shares)
#include "run_stages.h"
#pragma GCC visibility pop

namespace {  // the totals of a run with bgr_run_options.abundance
void graph_abundance_begin(bgr_graph* g) {  // a new run: the totals of the one before are gone, whatever becomes of this one
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->abundance.assign(g->header.n_unitigs, bgr_unitig_abundance{0, 0, 0});
    g->abundance_valid = false;
}
void graph_abundance_add(bgr_graph* g, const bgr_unitig_abundance* rows, uint64_t n) {  // one aligner's table
    std::lock_guard<std::mutex> l(g->abundance_m);
    for (uint64_t i = 0; i < n && i < g->abundance.size(); ++i) { g->abundance[i].reads += rows[i].reads; g->abundance[i].bases += rows[i].bases; g->abundance[i].kmers += rows[i].kmers; }
}
int graph_abundance_end(bgr_graph* g, bool ok) {  // totals only of a run that ended well
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (!ok) g->abundance.clear();
    g->abundance_valid = ok;
    return BGR_OK;
}
}  // namespace

// the geometry and form of the abundance kernel behind a launch of this size (bgr_aligner_abundance_plan reports what this returns)
bgr::AbundancePlan abundance_plan_of(const bgr_aligner* a, uint64_t n_reads, uint64_t total_bases) {
    return bgr::plan_abundance(a->graph->header.n_unitigs, a->dg.k, n_reads, total_bases, (uint32_t)a->num_cus, a->lds_per_cu, (uint32_t)a->sh->knob_abundance_form);
}

// ---- unitig abundance (bgr_run_options.abundance has the definition) ------------------------------------------------------------------
int abundance_table(bgr_aligner* a) {
    if (a->abundance.p) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(a->abundance.ensure((a->graph->header.n_unitigs + 1) * sizeof(bgr_unitig_abundance)));
    HIP_TRY(hipMemsetAsync(a->abundance.p, 0, a->abundance.cap, a->stream));   // (on the aligner's own stream, as bgr_aligner_reset_counters)
    HIP_TRY(hipStreamSynchronize(a->stream));
    HIP_TRY(bgr::prepare_abundance(a->lds_per_cu));   // (once per aligner, not per launch: form B's tables beyond 48 KB)
    return BGR_OK;
}

int bgr_aligner_abundance_enable(bgr_aligner* a, uint32_t on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_abundance_enable: null aligner");
    for (bgr_aligner* x = a; x && on; x = x->twin) { const int rc = abundance_table(x); if (rc != BGR_OK) return rc; }   // (one table per stream: a twin made later gets its own then)
    a->sh->abundance_on = on != 0;
    return BGR_OK;
}

int bgr_aligner_abundance(bgr_aligner* a, bgr_unitig_abundance* out, uint64_t n_rows) {
    static_assert(sizeof(bgr_unitig_abundance) == 24, "three u64 per unitig, as the kernel adds them");
    if (!a || (n_rows && !out)) return fail(BGR_E_ARG, "bgr_aligner_abundance: null argument");
    if (n_rows != a->graph->header.n_unitigs) return fail(BGR_E_ARG, "bgr_aligner_abundance: n_rows is not the graph's number of unitigs");
    if (!a->abundance.p) return fail(BGR_E_ARG, "bgr_aligner_abundance: abundance was never enabled on this aligner (bgr_aligner_abundance_enable)");
    if (n_rows == 0) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    memset(out, 0, n_rows * sizeof(bgr_unitig_abundance));
    std::vector<bgr_unitig_abundance> t(n_rows);
    for (bgr_aligner* x = a; x; x = x->twin) {  // its own table, and those of the streams that mapped the pieces of overlapped batches and un-waited launches
        if (!x->abundance.p) continue;
        if (const int rc = settle_pending(x); rc != BGR_OK) return rc;   // (an exhaustive launch whose counting is still to come)
        HIP_TRY(hipStreamSynchronize(x->stream));
        HIP_TRY(hipMemcpy(t.data(), x->abundance.as<bgr_unitig_abundance>() + 1, n_rows * sizeof(bgr_unitig_abundance), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n_rows; ++i) { out[i].reads += t[i].reads; out[i].bases += t[i].bases; out[i].kmers += t[i].kmers; }
    }
    return BGR_OK;
}

int bgr_aligner_abundance_plan(bgr_aligner* a, uint64_t n_reads, uint64_t total_bases, uint32_t out[4]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_abundance_plan: null argument");
    const bgr::AbundancePlan ap = abundance_plan_of(a, n_reads, total_bases);
    out[0] = ap.form; out[1] = ap.blocks; out[2] = ap.threads; out[3] = ap.lds_bytes;
    return BGR_OK;
}

int bgr_plan_abundance(uint64_t n_unitigs, uint32_t k, uint64_t n_reads, uint64_t total_bases, uint32_t num_cus, uint64_t lds_per_cu, uint32_t form_knob, uint32_t out[4]) {
    if (!out || form_knob > 2) return fail(BGR_E_ARG, "bgr_plan_abundance: null argument or a form beyond 2");
    const bgr::AbundancePlan ap = bgr::plan_abundance(n_unitigs, k, n_reads, total_bases, num_cus, lds_per_cu, form_knob);
    out[0] = ap.form; out[1] = ap.blocks; out[2] = ap.threads; out[3] = ap.lds_bytes;
    return BGR_OK;
}

int bgr_aligner_reset_abundance(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_reset_abundance: null aligner");
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) {
        if (!x->abundance.p) continue;
        HIP_TRY(hipMemsetAsync(x->abundance.p, 0, x->abundance.cap, x->stream));
        HIP_TRY(hipStreamSynchronize(x->stream));
    }
    return BGR_OK;
}

static int run_abundance_collect(bgr_graph* g, bgr_aligner* a) {   // a whole run: this aligner's table joins the run's totals in the graph
    std::vector<bgr_unitig_abundance> rows(g->header.n_unitigs);
    const int rc = bgr_aligner_abundance(a, rows.data(), rows.size());
    if (rc == BGR_OK) graph_abundance_add(g, rows.data(), rows.size());
    return rc;
}

int bgr_graph_abundance(const bgr_graph* g, bgr_unitig_abundance* out, uint64_t n_rows) {
    if (!g || (n_rows && !out)) return fail(BGR_E_ARG, "bgr_graph_abundance: null argument");
    if (!g->abundance_valid) return fail(BGR_E_ARG, "bgr_graph_abundance: no totals -- they are those of the last successful bgr_align_all with bgr_run_options.abundance = 1");
    if (n_rows != g->header.n_unitigs) return fail(BGR_E_ARG, "bgr_graph_abundance: n_rows is not the graph's number of unitigs");
    if (n_rows) memcpy(out, g->abundance.data(), n_rows * sizeof(bgr_unitig_abundance));
    return BGR_OK;
}

int bgr_write_abundance(const char* path, const bgr_graph* g, const bgr_unitig_abundance* rows, uint64_t n_rows) {
    if (!path || !g || (n_rows && !rows)) return fail(BGR_E_ARG, "bgr_write_abundance: null argument");
    if (n_rows != g->header.n_unitigs) return fail(BGR_E_ARG, "bgr_write_abundance: n_rows is not the graph's number of unitigs");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_write_abundance: the graph has no host blob (the unitig lengths are read from it)");
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
    return write_lines("bgr_write_abundance", path, "#unitig\tlength\treads\tbases\tkmers\n", n_rows, [&](uint64_t i, std::string* buf) {
        for (uint64_t x : {i + 1, (uint64_t)meta[i + 1].len, rows[i].reads, rows[i].bases}) { *buf += std::to_string(x); *buf += '\t'; }
        *buf += std::to_string(rows[i].kmers); *buf += '\n';
    });
}

// ---- what a whole run calls (run_counts.h) -------------------------------------------------------------------------------------
// The stages of a run (run_stages.h), and with them the two orders, kept here and nowhere else.
// The table's order is the order in which an aligner is collected: its links and pileup before its abundance (the pileup's snapshot reads the aligner's
// abundance table, and the first aligner's pileup table leaves it there).
// The tiers are the order in which the run ends: the abundance totals; the merged tables of links and triples; then what is derived from totals, each
// behind the one it reads -- the bubbles from the links, the phase from the bubbles and the triples, the blocks from the phase, the haplotypes from the
// blocks; last the pileup, behind the abundance totals, whose summed reads column guards the summed depths.  (The message of a failed run stays: only
// a refusal of a derived stage's or the pileup's end sets one.)
static int abundance_enable(bgr_aligner* a, uint32_t) { return bgr_aligner_abundance_enable(a, 1); }
static int links_enable(bgr_aligner* a, uint32_t) { return bgr_aligner_links_enable(a, 1); }
static int triples_enable(bgr_aligner* a, uint32_t) { return bgr_aligner_triples_enable(a, 1); }
static int pileup_enable(bgr_aligner* a, uint32_t what) { return what & bgr::kCountStrands ? bgr_aligner_pileup_strands_enable(a, 1) : bgr_aligner_pileup_enable(a, 1); }
static const bgr::RunStage kStages[] = {
    {bgr::kCountLinks, run_links_begin, links_enable, run_links_collect, run_links_end, bgr::kTierTables},
    {bgr::kCountBubbles, run_bubbles_begin, nullptr, run_bubbles_collect, run_bubbles_end, bgr::kTierDerived},
    {bgr::kCountTriples, run_triples_begin, triples_enable, run_triples_collect, run_triples_end, bgr::kTierTables},
    {bgr::kCountPhase, run_phase_begin, nullptr, nullptr, run_phase_end, bgr::kTierDerived},
    {bgr::kCountBlocks, run_blocks_begin, nullptr, nullptr, run_blocks_end, bgr::kTierDerived},
    {bgr::kCountHaplotypes, run_haplotypes_begin, nullptr, nullptr, run_haplotypes_end, bgr::kTierDerived},
    {bgr::kCountRecompact, run_recompact_begin, nullptr, run_recompact_collect, run_recompact_end, bgr::kTierDerived},
    {bgr::kCountPileup, run_pileup_begin, pileup_enable, run_pileup_collect, run_pileup_end, bgr::kTierPileup},
    {bgr::kCountAbundance, graph_abundance_begin, abundance_enable, run_abundance_collect, graph_abundance_end, bgr::kTierAbundance},
};
const int kNStages = sizeof(kStages) / sizeof(kStages[0]);

static uint32_t run_counts_wanted(const bgr_graph* g) {
    if (!g) return 0;
    return bgr::counts_wanted(bgr::RunSwitches{g->links.on, g->bubbles.on, g->triples.on, g->phase.on, g->blocks.on, g->haplotypes.on, g->pileup_on, g->variants_on, g->pileup_strands_on, g->variants_strands_on, g->recompact.on});
}
static void run_counts_begin(bgr_graph* g, uint32_t what) {
    for (const bgr::RunStage& s : kStages) if (what & s.bit) s.begin(g);
}
static int run_counts_enable(bgr_aligner* a, uint32_t what) {   // every launch of the aligner is followed by the kernels of what the run counts
    int rc = BGR_OK;
    for (const bgr::RunStage& s : kStages) if (rc == BGR_OK && (what & s.bit) && s.enable) rc = s.enable(a, what);   // (the tables are independent: the order decides nothing)
    return rc;
}
static int run_counts_collect(bgr_graph* g, bgr_aligner* a, uint32_t what) {
    int rc = BGR_OK;
    for (const bgr::RunStage& s : kStages) if (rc == BGR_OK && (what & s.bit) && s.collect) rc = s.collect(g, a);
    return rc;
}
static int run_counts_end(bgr_graph* g, uint32_t what, bool ok) { return bgr::end_stages(kStages, kNStages, g, what, ok); }
static const bool g_run_counts_registered = (bgr::g_run_counts = bgr::RunCounts{run_counts_wanted, run_counts_begin, run_counts_enable, run_counts_collect, run_counts_end, run_haplotag_table, bgr_aligner_haplotag_enable, bgr_graph_gaf_cs_enabled, bgr_aligner_gaf_cs_enable, bgr_graph_inside_enabled, run_inside_begin, bgr_aligner_inside_enable, run_inside_collect, bgr_graph_exhaustive_paths_enabled, bgr_aligner_exhaustive_paths_enable}, true);
