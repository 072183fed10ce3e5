// capi_abundance.hip -- the C-ABI's unitig abundance (bgr_run_options.abundance in include/bgreat_gpu.h has the definition): the aligners'
// tables, the run's totals in the graph object, the writer; and the table through which a whole run (pipeline.cpp, run_counts.h) reaches
// every counting feature -- abundance is the one that all of them imply.
#include <cstdio>
#include <cstring>

#include "capi_internal.h"
#include "run_counts.h"

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
void graph_abundance_end(bgr_graph* g, bool ok) {  // totals only of a run that ended well
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (!ok) g->abundance.clear();
    g->abundance_valid = ok;
}
}  // namespace

// the geometry and form of the abundance kernel behind a launch of this size (bgr_aligner_abundance_plan reports what this returns)
bgr::AbundancePlan abundance_plan_of(const bgr_aligner* a, uint64_t n_reads, uint64_t total_bases) {
    return bgr::plan_abundance(a->graph->header.n_unitigs, a->dg.k, n_reads, total_bases, (uint32_t)a->num_cus, a->lds_per_cu, a->knob_abundance_form);
}

// ---- unitig abundance (bgr_run_options.abundance has the definition) ------------------------------------------------------------------
int abundance_set(bgr_aligner* a, bool on) {
    if (on && !a->abundance.p) {
        HIP_TRY(hipSetDevice(a->device));
        HIP_TRY(a->abundance.ensure((a->graph->header.n_unitigs + 1) * sizeof(bgr_unitig_abundance)));
        HIP_TRY(hipMemsetAsync(a->abundance.p, 0, a->abundance.cap, a->stream));   // (on the aligner's own stream, as bgr_aligner_reset_counters)
        HIP_TRY(hipStreamSynchronize(a->stream));
        HIP_TRY(bgr::prepare_abundance(a->lds_per_cu));   // (once per aligner, not per launch: form B's tables beyond 48 KB)
    }
    a->abundance_on = on;
    return BGR_OK;
}

int bgr_aligner_abundance_enable(bgr_aligner* a, uint32_t on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_abundance_enable: null aligner");
    for (bgr_aligner* x = a; x; x = x->twin) { const int rc = abundance_set(x, on != 0); if (rc != BGR_OK) return rc; }
    return BGR_OK;
}

int bgr_aligner_abundance(bgr_aligner* a, bgr_unitig_abundance* out, uint64_t n_rows) {
    static_assert(sizeof(bgr_unitig_abundance) == 24, "three u64 per unitig, as the kernel adds them");
    if (!a || (n_rows && !out)) return fail(BGR_E_ARG, "bgr_aligner_abundance: null argument");
    if (n_rows != a->graph->header.n_unitigs) return fail(BGR_E_ARG, "bgr_aligner_abundance: n_rows is not the graph's number of unitigs");
    if (!a->abundance.p) return fail(BGR_E_ARG, "bgr_aligner_abundance: abundance was never enabled on this aligner (bgr_aligner_abundance_enable)");
    if (n_rows == 0) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    HIP_TRY(hipMemcpy(out, static_cast<const bgr_unitig_abundance*>(a->abundance.p) + 1, n_rows * sizeof(bgr_unitig_abundance), hipMemcpyDeviceToHost));
    std::vector<bgr_unitig_abundance> t;
    for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) {  // the pieces of overlapped batches its other streams mapped
        if (!tw->abundance.p) continue;
        t.resize(n_rows);
        HIP_TRY(hipStreamSynchronize(tw->stream));
        HIP_TRY(hipMemcpy(t.data(), static_cast<const bgr_unitig_abundance*>(tw->abundance.p) + 1, n_rows * sizeof(bgr_unitig_abundance), hipMemcpyDeviceToHost));
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
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string("bgr_write_abundance: cannot open ") + path);
    std::string buf = "#unitig\tlength\treads\tbases\tkmers\n";
    bool ok = true;
    for (uint64_t i = 0; i < n_rows && ok; ++i) {
        buf += std::to_string(i + 1); buf += '\t';
        buf += std::to_string(meta[i + 1].len); buf += '\t';
        buf += std::to_string(rows[i].reads); buf += '\t';
        buf += std::to_string(rows[i].bases); buf += '\t';
        buf += std::to_string(rows[i].kmers); buf += '\n';
        if (buf.size() > (1u << 20)) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); }
    }
    if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string("bgr_write_abundance: write to ") + path + " failed");
    return BGR_OK;
}

// ---- what a whole run calls (run_counts.h) -------------------------------------------------------------------------------------
// The orders are kept here and nowhere else: an aligner's links and pileup are collected before its abundance (the pileup's snapshot reads the
// aligner's abundance table, and the first aligner's pileup table leaves it there); the pileup ends behind the abundance, whose summed reads
// column guards the summed depths.
static uint32_t run_counts_wanted(const bgr_graph* g) {
    if (!g) return 0;
    uint32_t what = 0;
    const bool blocks = g->blocks_on || g->haplotypes_on;   // (the haplotypes' switch implies the blocks')
    const bool phase = g->phase_on || blocks;   // (the blocks' switch implies the phase's)
    if (g->links_on || g->bubbles_on || phase) what |= bgr::kCountLinks;
    if (g->bubbles_on || phase) what |= bgr::kCountBubbles;
    if (g->triples_on || phase) what |= bgr::kCountTriples;
    if (phase) what |= bgr::kCountPhase;
    if (blocks) what |= bgr::kCountBlocks;
    if (g->haplotypes_on) what |= bgr::kCountHaplotypes;
    if (g->pileup_on || g->variants_on) what |= bgr::kCountPileup;
    if (g->variants_on) what |= bgr::kCountVariants;
    if ((g->pileup_on && g->pileup_strands_on) || (g->variants_on && g->variants_strands_on)) what |= bgr::kCountStrands;
    return what ? what | bgr::kCountAbundance : 0;
}
static void run_counts_begin(bgr_graph* g, uint32_t what) {
    if (what & bgr::kCountAbundance) graph_abundance_begin(g);
    if (what & bgr::kCountLinks) run_links_begin(g);
    if (what & bgr::kCountBubbles) run_bubbles_begin(g);
    if (what & bgr::kCountTriples) run_triples_begin(g);
    if (what & bgr::kCountPhase) run_phase_begin(g);
    if (what & bgr::kCountBlocks) run_blocks_begin(g);
    if (what & bgr::kCountHaplotypes) run_haplotypes_begin(g);
    if (what & bgr::kCountPileup) run_pileup_begin(g);
}
static int run_counts_enable(bgr_aligner* a, uint32_t what) {   // every launch of the aligner is followed by the kernels of what the run counts
    int rc = what & bgr::kCountAbundance ? bgr_aligner_abundance_enable(a, 1) : BGR_OK;
    if (rc == BGR_OK && (what & bgr::kCountLinks)) rc = bgr_aligner_links_enable(a, 1);
    if (rc == BGR_OK && (what & bgr::kCountTriples)) rc = bgr_aligner_triples_enable(a, 1);
    if (rc == BGR_OK && (what & bgr::kCountPileup)) rc = what & bgr::kCountStrands ? bgr_aligner_pileup_strands_enable(a, 1) : bgr_aligner_pileup_enable(a, 1);
    return rc;
}
static int run_counts_collect(bgr_graph* g, bgr_aligner* a, uint32_t what) {
    int rc = what & bgr::kCountLinks ? run_links_collect(g, a) : BGR_OK;
    if (rc == BGR_OK && (what & bgr::kCountBubbles)) run_bubbles_collect(g, a);
    if (rc == BGR_OK && (what & bgr::kCountTriples)) rc = run_triples_collect(g, a);
    if (rc == BGR_OK && (what & bgr::kCountPileup)) rc = run_pileup_collect(g, a);
    if (rc == BGR_OK && (what & bgr::kCountAbundance)) rc = run_abundance_collect(g, a);
    return rc;
}
static int run_counts_end(bgr_graph* g, uint32_t what, bool ok) {   // (the message of a failed run stays: only a refusal of the bubbles' or the pileup's end sets one)
    if (what & bgr::kCountAbundance) graph_abundance_end(g, ok);
    if (what & bgr::kCountLinks) run_links_end(g, ok);
    if (what & bgr::kCountTriples) run_triples_end(g, ok);
    int brc = what & bgr::kCountBubbles ? run_bubbles_end(g, ok) : BGR_OK;   // (behind the links' end: it reads the merged links)
    if (brc == BGR_OK && (what & bgr::kCountPhase)) brc = run_phase_end(g, ok);   // (behind the bubbles' and the triples' end: it joins the two)
    if (what & bgr::kCountBlocks) brc = brc == BGR_OK ? run_blocks_end(g, ok) : (run_blocks_end(g, false), brc);   // (behind the phase's end: it chains the records)
    if (what & bgr::kCountHaplotypes) brc = brc == BGR_OK ? run_haplotypes_end(g, ok) : (run_haplotypes_end(g, false), brc);   // (behind the blocks' end: it spells the entries)
    if (brc != BGR_OK) {   // (the run has failed after all: it leaves no totals)
        graph_abundance_end(g, false); run_links_end(g, false);
        if (what & bgr::kCountTriples) run_triples_end(g, false);
        if (what & bgr::kCountPhase) (void)run_phase_end(g, false);
        if (what & bgr::kCountBlocks) (void)run_blocks_end(g, false);
        if (what & bgr::kCountHaplotypes) (void)run_haplotypes_end(g, false);
    }
    const int prc = what & bgr::kCountPileup ? run_pileup_end(g, ok && brc == BGR_OK) : BGR_OK;
    return brc != BGR_OK ? brc : prc;
}
static const bool g_run_counts_registered = (bgr::g_run_counts = bgr::RunCounts{run_counts_wanted, run_counts_begin, run_counts_enable, run_counts_collect, run_counts_end}, true);
