// capi_triples.hip -- the C-ABI's triples and read-backed phasing (bgr_triple and bgr_phase in include/bgreat_gpu.h have the definitions): the
// aligners' hash tables, the run's totals in the graph object, the join of the run's bubbles with its triples (phase_host.h), the two writers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_internal.h"
#include "phase_host.h"
#include "triples_kernels.h"

typedef bgr_graph::TripleRow TripleRow;
static bool row_less(const TripleRow& x, const TripleRow& y) { return x.k0 < y.k0 || (x.k0 == y.k0 && x.k1 < y.k1); }

// ---- triples (bgr_triple in include/bgreat_gpu.h has the definition) -----------------------------------------------------------------------
static int graph_triples_bound(bgr_graph* g, uint64_t* bound) {
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_triples_bound: the graph has no host blob (the bound is counted over its unitigs' ends)");
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (!g->triples_bound_known) { g->triples_bound = bgr::triples_bound_of_blob(g->host.header(), g->host.base()); g->triples_bound_known = true; }
    *bound = g->triples_bound;
    return BGR_OK;
}
int bgr_graph_triples_bound(bgr_graph* g, uint64_t* bound) {
    if (!g || !bound) return fail(BGR_E_ARG, "bgr_graph_triples_bound: null argument");
    return graph_triples_bound(g, bound);
}

int bgr_triple_canonical(int32_t a, int32_t b, int32_t c, bgr_triple* out) {
    if (!out || !bgr::phase_id_ok(a) || !bgr::phase_id_ok(b) || !bgr::phase_id_ok(c)) return fail(BGR_E_ARG, "bgr_triple_canonical: null argument or an id that is 0 or beyond 2^30");
    const bgr::TripleKey k = bgr::triples_canonical(a, b, c);   // (the function the kernel calls)
    *out = bgr_triple{bgr::links_key_from(k.k0), bgr::links_key_to(k.k0), bgr::triples_key_to(k.k1), 0, 0};
    return BGR_OK;
}

void triples_share(bgr_aligner* a) {   // the twins add to the aligner's table
    for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) { tw->triples_tab = a->triples_tab; tw->triples_cap = a->triples_cap; tw->triples_bound = a->triples_bound; tw->triples_on = a->triples_on; }
}

int bgr_aligner_triples_enable(bgr_aligner* a, uint32_t on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_triples_enable: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_triples_enable: an internal stream of another aligner");
    if (on && !a->triples_tab) {
        if (a->graph->header.n_unitigs >= 0x40000000ull) return fail(BGR_E_ARG, "bgr_aligner_triples_enable: a graph of 2^30 unitigs or more (an id and its sign fit 31 bits of the key)");
        uint64_t bound = 0;
        const int rc = graph_triples_bound(a->graph, &bound);
        if (rc != BGR_OK) return rc;
        if (bound >= (1ull << 56)) return fail(BGR_E_NOMEM, "bgr_aligner_triples_enable: a bound of " + std::to_string(bound) + " triples: no device holds the table");
        uint64_t cap = bgr::triples_capacity(bound);
        if (const int64_t c = bgr::opt("test.triples_capacity")) { cap = 2; while (cap < (uint64_t)c) cap <<= 1; }
        HIP_TRY(hipSetDevice(a->device));
        const hipError_t e = a->triples.ensure(bgr::triples_table_bytes(cap));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            a->triples.release();   // (nothing stays allocated)
            return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, "bgr_aligner_triples_enable: " + std::to_string(bgr::triples_table_bytes(cap)) + " bytes for the table of triples: " + hipGetErrorString(e));
        }
        HIP_TRY(hipMemsetAsync(a->triples.p, 0, a->triples.cap, a->stream));   // (on the aligner's own stream, as bgr_aligner_reset_counters)
        HIP_TRY(hipStreamSynchronize(a->stream));
        a->triples_tab = static_cast<unsigned long long*>(a->triples.p);
        a->triples_cap = cap;
        a->triples_bound = bound;
    }
    a->triples_on = on != 0;
    triples_share(a);
    return BGR_OK;
}

// the words behind the aligner's table (triples_kernels.h), every stream that adds to it waited for; BGR_E_CAPACITY when the overflow word is set
static int triples_tail(bgr_aligner* a, const char* who, uint64_t* tail) {
    if (!a->triples_tab) return fail(BGR_E_ARG, std::string(who) + ": triples were never enabled on this aligner (bgr_aligner_triples_enable)");
    if (const int rc = sync_all(a); rc != BGR_OK) return rc;
    HIP_TRY(hipMemcpy(tail, a->triples_tab + bgr::kTriplesSlotWords * a->triples_cap, bgr::kTriplesTailWords * 8, hipMemcpyDeviceToHost));
    if (tail[0])
        return fail(BGR_E_CAPACITY, std::string(who) + ": the table of triples (" + std::to_string(a->triples_cap) + " slots) was full: " + std::to_string(tail[0]) +
                                        " traversals found no place; the counts are incomplete until bgr_aligner_reset_triples");
    return BGR_OK;
}
// ... and the table as it stands: the used slots (k1 != 0: the kernel leaves no slot half claimed), sorted by key.  Only if there are at most
// `room` of them, as links_snapshot
static int triples_snapshot(bgr_aligner* a, const char* who, uint64_t room, std::vector<TripleRow>& rows, uint64_t tail[bgr::kTriplesTailWords]) {
    const int rc = triples_tail(a, who, tail);
    if (rc != BGR_OK) return rc;
    rows.clear();
    if (tail[1] > room || tail[1] == 0) return BGR_OK;
    std::vector<uint64_t> t(bgr::kTriplesSlotWords * a->triples_cap);
    HIP_TRY(hipMemcpy(t.data(), a->triples_tab, t.size() * 8, hipMemcpyDeviceToHost));
    for (uint64_t s = 0; s < a->triples_cap; ++s)
        if (t[3 * s + 1]) rows.push_back(TripleRow{t[3 * s], t[3 * s + 1], t[3 * s + 2]});
    std::sort(rows.begin(), rows.end(), row_less);
    return BGR_OK;
}
static void triples_deliver(const std::vector<TripleRow>& rows, bgr_triple* out) {
    for (size_t i = 0; i < rows.size(); ++i) out[i] = bgr_triple{bgr::links_key_from(rows[i].k0), bgr::links_key_to(rows[i].k0), bgr::triples_key_to(rows[i].k1), 0, rows[i].count};
}

int bgr_aligner_triples(bgr_aligner* a, bgr_triple* out, uint64_t cap, uint64_t* n) {
    static_assert(sizeof(bgr_triple) == 24, "three ids, a reserved word and a 64-bit count");
    if (n) *n = 0;
    if (!a || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_aligner_triples: null argument");
    std::vector<TripleRow> rows;
    uint64_t tail[bgr::kTriplesTailWords];
    const int rc = triples_snapshot(a, "bgr_aligner_triples", cap, rows, tail);
    if (rc != BGR_OK) return rc;
    *n = tail[1];
    if (tail[1] > cap) return fail(BGR_E_CAPACITY, "bgr_aligner_triples: " + std::to_string(tail[1]) + " triples, room for " + std::to_string(cap));
    if (rows.size() != tail[1]) return fail(BGR_E_INTERNAL, "bgr_aligner_triples: the table's used slots and their counter disagree");
    triples_deliver(rows, out);
    return BGR_OK;
}

int bgr_aligner_triples_info(bgr_aligner* a, uint64_t out[4]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_triples_info: null argument");
    uint64_t tail[bgr::kTriplesTailWords] = {0, 0};
    const int rc = triples_tail(a, "bgr_aligner_triples_info", tail);
    if (rc != BGR_OK && rc != BGR_E_CAPACITY) return rc;   // (an overflow is what this call reports)
    out[0] = a->triples_cap; out[1] = a->triples_bound; out[2] = tail[0]; out[3] = tail[1];
    return BGR_OK;
}

int bgr_aligner_reset_triples(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_reset_triples: null aligner");
    if (!a->triples.p) return BGR_OK;
    if (const int rc = sync_all(a); rc != BGR_OK) return rc;   // (the twins add to the same table)
    HIP_TRY(hipMemsetAsync(a->triples.p, 0, a->triples.cap, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return BGR_OK;
}

// what a whole run calls (run_counts.h, through capi_abundance.hip)
void run_triples_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->triples.clear();
    g->triples_valid = false;
}
int run_triples_collect(bgr_graph* g, bgr_aligner* a) {
    std::vector<TripleRow> rows;
    uint64_t tail[bgr::kTriplesTailWords];
    const int rc = triples_snapshot(a, "bgr_align_all", ~0ull, rows, tail);
    if (rc != BGR_OK) return rc;
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->triples.insert(g->triples.end(), rows.begin(), rows.end());
    return BGR_OK;
}
void run_triples_end(bgr_graph* g, bool ok) {   // the aligners' tables, one behind the other: sorted, equal keys summed
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (!ok) g->triples.clear();
    else {
        std::sort(g->triples.begin(), g->triples.end(), row_less);
        size_t w = 0;
        for (size_t i = 0; i < g->triples.size(); ++i) {
            if (w && g->triples[w - 1].k0 == g->triples[i].k0 && g->triples[w - 1].k1 == g->triples[i].k1) g->triples[w - 1].count += g->triples[i].count;
            else g->triples[w++] = g->triples[i];
        }
        g->triples.resize(w);
    }
    g->triples_valid = ok;
}

int bgr_graph_triples_enable(bgr_graph* g, uint32_t on) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_triples_enable: null graph");
    if (on && g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_triples_enable: the graph has no host blob (the table of triples is sized from it)");
    g->triples_on = on != 0;
    return BGR_OK;
}

int bgr_graph_triples_enabled(const bgr_graph* g) { return g && g->triples_on ? 1 : 0; }

int bgr_graph_triples(const bgr_graph* g, bgr_triple* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!g || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_graph_triples: null argument");
    if (!g->triples_valid) return fail(BGR_E_ARG, "bgr_graph_triples: no totals -- they are those of the last successful bgr_align_all with bgr_graph_triples_enable on");
    *n = g->triples.size();
    if (g->triples.size() > cap) return fail(BGR_E_CAPACITY, "bgr_graph_triples: " + std::to_string(g->triples.size()) + " triples, room for " + std::to_string(cap));
    triples_deliver(g->triples, out);
    return BGR_OK;
}

// a file of lines: the header, then line(i) for i < n, in pieces of a megabyte
template <class Line>
static int write_lines(const char* who, const char* path, const char* header, uint64_t n, Line line) {
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string(who) + ": cannot open " + path);
    std::string buf = header;
    bool ok = true;
    for (uint64_t i = 0; i < n && ok; ++i) {
        line(i, &buf);
        if (buf.size() > (1u << 20)) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); }
    }
    if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string(who) + ": write to " + path + " failed");
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
    *n = recs.size();
    if (recs.size() > cap) return fail(BGR_E_CAPACITY, "bgr_bubbles_phase: " + std::to_string(recs.size()) + " neighbour pairs, room for " + std::to_string(cap));
    if (!recs.empty()) memcpy(out, recs.data(), recs.size() * sizeof(bgr_phase));
    return BGR_OK;
}

void run_phase_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->phase.clear();
    g->phase_valid = false;
}
int run_phase_end(bgr_graph* g, bool ok) {   // behind run_bubbles_end and run_triples_end: the run's bubbles and its merged, sorted triples
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->phase.clear();
    g->phase_valid = false;
    if (!ok) return BGR_OK;
    if (!g->bubbles_valid || !g->triples_valid) return fail(BGR_E_INTERNAL, "bgr_align_all: phase records without the bubbles and the triples they are joined from");
    std::vector<bgr_triple> t(g->triples.size());
    triples_deliver(g->triples, t.data());
    g->phase = bgr::phase_of(g->bubbles.data(), g->bubbles.size(), t.data(), t.size());
    g->phase_valid = true;
    return BGR_OK;
}

int bgr_graph_phase_enable(bgr_graph* g, uint32_t on, uint64_t min_link) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_phase_enable: null graph");
    if (on) {
        if (min_link == 0) return fail(BGR_E_ARG, "bgr_graph_phase_enable: min_link is at least 1");
        if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_phase_enable: the graph has no host blob (the tables of links and triples are sized from it)");
        if (g->header.has_exc)
            return fail(BGR_E_ARG, "bgr_graph_phase_enable: phasing (--phase) joins bubbles, which need a graph of ACGT-only unitigs: on one with other characters a branch read backwards does not spell the reverse complement");
        g->phase_min_link = min_link;
    }
    g->phase_on = on != 0;
    return BGR_OK;
}

int bgr_graph_phase_enabled(const bgr_graph* g) { return g && g->phase_on ? 1 : 0; }

int bgr_graph_phase(const bgr_graph* g, bgr_phase* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!g || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_graph_phase: null argument");
    if (!g->phase_valid) return fail(BGR_E_ARG, "bgr_graph_phase: no records -- they are those of the last successful bgr_align_all with bgr_graph_phase_enable on");
    *n = g->phase.size();
    if (g->phase.size() > cap) return fail(BGR_E_CAPACITY, "bgr_graph_phase: " + std::to_string(g->phase.size()) + " neighbour pairs, room for " + std::to_string(cap));
    if (!g->phase.empty()) memcpy(out, g->phase.data(), g->phase.size() * sizeof(bgr_phase));
    return BGR_OK;
}

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
