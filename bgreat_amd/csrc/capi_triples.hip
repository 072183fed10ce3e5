// capi_triples.hip -- the C-ABI's triples and read-backed phasing (bgr_triple and bgr_phase in include/bgreat_gpu.h have the definitions): the
// join of the run's bubbles with its triples (phase_host.h), the two writers.  The table of triples is capi_links.hip's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_internal.h"
#include "phase_host.h"
#include "triples_kernels.h"

// ---- triples (bgr_triple in include/bgreat_gpu.h has the definition; capi_links.hip has their table) ------------------------------------------
int bgr_triple_canonical(int32_t a, int32_t b, int32_t c, bgr_triple* out) {
    if (!out || !bgr::phase_id_ok(a) || !bgr::phase_id_ok(b) || !bgr::phase_id_ok(c)) return fail(BGR_E_ARG, "bgr_triple_canonical: null argument or an id that is 0 or beyond 2^30");
    const bgr::TripleKey k = bgr::triples_canonical(a, b, c);   // (the function the kernel calls)
    *out = bgr_triple{bgr::links_key_from(k.k0), bgr::links_key_to(k.k0), bgr::triples_key_to(k.k1), 0, 0};
    return BGR_OK;
}

int bgr_write_triples(const char* path, const bgr_graph* g, const bgr_triple* triples, uint64_t n) {
    if (!path || !g || (n && !triples)) return fail(BGR_E_ARG, "bgr_write_triples: null argument");
    const uint64_t nu = g->header.n_unitigs;
    for (uint64_t i = 0; i < n; ++i) {
        const bgr_triple& t = triples[i];
        for (int32_t x : {t.from, t.via, t.to})
            if (!bgr::phase_id_ok(x) || (uint64_t)bgr::bubbles_abs(x) > nu) return fail(BGR_E_ARG, "bgr_write_triples: record " + std::to_string(i) + " names a unitig the graph does not have");
        if (i && !(bgr::phase_key(triples[i - 1].from, triples[i - 1].via, triples[i - 1].to) < bgr::phase_key(t.from, t.via, t.to)))
            return fail(BGR_E_ARG, "bgr_write_triples: the triples are not sorted by key (record " + std::to_string(i) + ")");
    }
    return write_lines("bgr_write_triples", path, bgr::triples_header(), n, [&](uint64_t i, std::string* buf) { if (triples[i].count) bgr::triples_line(triples[i], buf); });
}

// ---- read-backed phasing of neighbouring bubbles (bgr_phase in include/bgreat_gpu.h has the definition) ---------------------------------------
int bgr_bubbles_phase(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_triple* triples, uint64_t n_triples, bgr_phase* out, uint64_t cap, uint64_t* n) {
    static_assert(sizeof(bgr_phase) == 64, "eight words of ids and four 64-bit counts");
    if (n) *n = 0;
    if (!n || (n_bubbles && !bubbles) || (n_triples && !triples) || (cap && !out)) return fail(BGR_E_ARG, "bgr_bubbles_phase: null argument");
    uint64_t bad = 0;
    if (const int what = bgr::phase_check(bubbles, n_bubbles, triples, n_triples, &bad)) {
        static const char* const msg[] = {"", "bubble %s names an id that is 0 or beyond 2^30", "triple %s names an id that is 0 or beyond 2^30", "triple %s is not canonical (bgr_triple_canonical)",
                                          "the triples are not strictly ascending by key (triple %s)"};
        std::string m = msg[what];
        m.replace(m.find("%s"), 2, std::to_string(bad));
        return fail(BGR_E_ARG, "bgr_bubbles_phase: " + m);
    }
    const std::vector<bgr_phase> recs = bgr::phase_of(bubbles, n_bubbles, triples, n_triples);
    return deliver_rows(recs, out, cap, n, "bgr_bubbles_phase", "neighbour pairs");
}

void run_phase_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->phase.forget();
}
int run_phase_end(bgr_graph* g, bool ok) {   // behind run_bubbles_end and run_triples_end: the run's bubbles and its merged, sorted triples
    std::lock_guard<std::mutex> l(g->abundance_m);
    return chain_stage_end(g, g->phase, ok, g->bubbles.valid && g->triples.valid, "phase records without the bubbles and the triples they are joined from", !g->bubbles.rows.empty(), "bubbles", [&] {
        std::vector<bgr_triple> t(g->triples.rows.size());
        triples_records(g->triples.rows, t.data());
        g->phase.rows = bgr::phase_of(g->bubbles.rows.data(), g->bubbles.rows.size(), t.data(), t.size());
        return BGR_OK;
    });
}

int bgr_graph_phase_enable(bgr_graph* g, uint32_t on, uint64_t min_link) {
    const ChainMins given = {min_link, 1, 1};
    if (const int rc = chain_refusal(g, "bgr_graph_phase_enable", on, given, "the tables of links and triples are sized from it",
                                     "phasing (--phase) joins bubbles, which need a graph of ACGT-only unitigs: on one with other characters a branch read backwards does not spell the reverse complement");
        rc != BGR_OK)
        return rc;
    g->phase.set(on, given);
    return BGR_OK;
}

int bgr_graph_phase_enabled(const bgr_graph* g) { return g && g->phase.on ? 1 : 0; }

int bgr_graph_phase(const bgr_graph* g, bgr_phase* out, uint64_t cap, uint64_t* n) { return graph_rows(g, &bgr_graph::phase, out, cap, n, "bgr_graph_phase", "neighbour pairs", "records"); }

int bgr_write_phase(const char* path, const bgr_graph* g, const bgr_phase* records, uint64_t n) {
    if (!path || !g || (n && !records)) return fail(BGR_E_ARG, "bgr_write_phase: null argument");
    const uint64_t nu = g->header.n_unitigs;
    for (uint64_t i = 0; i < n; ++i) {
        const bgr_phase& p = records[i];
        for (int32_t x : {p.via, p.source, p.in[0], p.in[1], p.out[0], p.out[1], p.sink})
            if (!bgr::phase_id_ok(x) || (uint64_t)bgr::bubbles_abs(x) > nu) return fail(BGR_E_ARG, "bgr_write_phase: record " + std::to_string(i) + " names a unitig the graph does not have");
    }
    return write_lines("bgr_write_phase", path, bgr::phase_header(), n, [&](uint64_t i, std::string* buf) { bgr::phase_line(records[i], buf); });
}
