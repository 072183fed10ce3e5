// capi_links.hip -- the C-ABI's count tables, links and triples (bgr_link and bgr_triple in include/bgreat_gpu.h have the definitions): the
// aligners' hash tables and the run's totals in the graph object, once for both; what only the links have; the GFA writer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_internal.h"
#include "links_kernels.h"
#include "triples_kernels.h"

// ---- the count tables: links (W = 2 words a slot) and triples (W = 3) --------------------------------------------------------------------------
// One implementation serves both; what differs is in the descriptor.  A host row is the slot's W words: the key words, then the count.
struct TableDesc {
    const char* noun;              // what the messages and the names of the calls say
    const char* capacity_option;   // the test hook that sizes the table
    uint32_t used_word;            // a slot is used when this word of it is not 0 (the kernels leave no slot half claimed)
    uint32_t tail_words, tail_used;   // the words behind the slots: [0] = traversals that found no place, [tail_used] = used slots (= distinct keys)
    bool narrow_ids;               // an id and its sign fit 31 bits of the key: no graph of 2^30 unitigs, no bound of 2^56
    uint64_t (*bound_of_blob)(const BgrBlobHeader* h, const uint8_t* base);
    uint64_t (*capacity)(uint64_t bound);
    uint64_t (*table_bytes)(uint64_t capacity);
    const char* bound_clause;
};
template <size_t W> struct Table;
template <> struct Table<2> {
    static constexpr TableDesc d = {"links", "test.links_capacity", 0, bgr::kLinksTailWords, 2, false, bgr::links_bound_of_blob, bgr::links_capacity, bgr::links_table_bytes, "the bound is counted over its slots"};
    static CountTable& of(bgr_aligner* a) { return a->sh->links; }
    static CountRows<2>& of(bgr_graph* g) { return g->links; }
};
template <> struct Table<3> {
    static constexpr TableDesc d = {"triples", "test.triples_capacity", 1, bgr::kTriplesTailWords, 1, true, bgr::triples_bound_of_blob, bgr::triples_capacity, bgr::triples_table_bytes, "the bound is counted over its unitigs' ends"};
    static CountTable& of(bgr_aligner* a) { return a->sh->triples; }
    static CountRows<3>& of(bgr_graph* g) { return g->triples; }
};
static_assert(bgr::kTriplesSlotWords == 3, "a slot of the table of triples is a host row");
template <size_t W> using Rows = std::vector<std::array<uint64_t, W>>;
template <size_t W> static std::string name_of(const char* prefix, const char* suffix = "") { return std::string(prefix) + Table<W>::d.noun + suffix; }

template <size_t W>
static int graph_bound(bgr_graph* g, uint64_t* bound) {
    if (g->host.blob.empty()) return fail(BGR_E_ARG, name_of<W>("bgr_graph_", "_bound") + ": the graph has no host blob (" + Table<W>::d.bound_clause + ")");
    std::lock_guard<std::mutex> l(g->abundance_m);
    CountRows<W>& r = Table<W>::of(g);
    if (!r.bound_known) { r.bound = Table<W>::d.bound_of_blob(g->host.header(), g->host.base()); r.bound_known = true; }
    *bound = r.bound;
    return BGR_OK;
}
template <size_t W>
static int graph_bound_checked(bgr_graph* g, uint64_t* bound) {
    if (!g || !bound) return fail(BGR_E_ARG, name_of<W>("bgr_graph_", "_bound") + ": null argument");
    return graph_bound<W>(g, bound);
}

template <size_t W>
static int table_enable(bgr_aligner* a, uint32_t on) {
    const TableDesc& d = Table<W>::d;
    const std::string who = name_of<W>("bgr_aligner_", "_enable");
    if (!a) return fail(BGR_E_ARG, who + ": null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, who + ": an internal stream of another aligner");
    CountTable& t = Table<W>::of(a);
    if (on && !t.tab) {
        if (d.narrow_ids && a->graph->header.n_unitigs >= 0x40000000ull) return fail(BGR_E_ARG, who + ": a graph of 2^30 unitigs or more (an id and its sign fit 31 bits of the key)");
        uint64_t bound = 0;
        const int rc = graph_bound<W>(a->graph, &bound);
        if (rc != BGR_OK) return rc;
        if (d.narrow_ids && bound >= (1ull << 56)) return fail(BGR_E_NOMEM, who + ": a bound of " + std::to_string(bound) + " " + d.noun + ": no device holds the table");
        uint64_t cap = d.capacity(bound);
        if (const int64_t c = bgr::opt(d.capacity_option)) { cap = 2; while (cap < (uint64_t)c) cap <<= 1; }
        HIP_TRY(hipSetDevice(a->device));
        const hipError_t e = t.buf.ensure(d.table_bytes(cap));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            t.buf.release();   // (nothing stays allocated)
            return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, who + ": " + std::to_string(d.table_bytes(cap)) + " bytes for the table of " + d.noun + ": " + hipGetErrorString(e));
        }
        HIP_TRY(hipMemsetAsync(t.buf.p, 0, t.buf.cap, a->stream));   // (on the aligner's own stream, as bgr_aligner_reset_counters)
        HIP_TRY(hipStreamSynchronize(a->stream));
        t.tab = static_cast<unsigned long long*>(t.buf.p);
        t.cap = cap;
        t.bound = bound;
    }
    t.on = on != 0;
    return BGR_OK;
}

// the words behind the aligner's table, every stream that adds to it waited for; BGR_E_CAPACITY when the overflow word is set
template <size_t W>
static int table_tail(bgr_aligner* a, const char* who, uint64_t* tail) {   // (tail: d.tail_words words)
    const TableDesc& d = Table<W>::d;
    const CountTable& t = Table<W>::of(a);
    if (!t.tab) return fail(BGR_E_ARG, std::string(who) + ": " + d.noun + " were never enabled on this aligner (" + name_of<W>("bgr_aligner_", "_enable") + ")");
    if (const int rc = sync_all(a); rc != BGR_OK) return rc;
    HIP_TRY(hipMemcpy(tail, t.tab + W * t.cap, d.tail_words * 8, hipMemcpyDeviceToHost));
    if (tail[0])
        return fail(BGR_E_CAPACITY, std::string(who) + ": the table of " + d.noun + " (" + std::to_string(t.cap) + " slots) was full: " + std::to_string(tail[0]) +
                                        " traversals found no place; the counts are incomplete until " + name_of<W>("bgr_aligner_reset_"));
    return BGR_OK;
}
int links_tail(bgr_aligner* a, const char* who, uint64_t* tail) { return table_tail<2>(a, who, tail); }   // (capi_bubbles.hip calls it too)

// ... and the table as it stands: the used slots, sorted by key.  Only if there are at most `room` of them (the kernel counts the slots it claims):
// a caller that asks for the number first does not pay for the table's way to the host twice.  *used = their number
template <size_t W>
static int table_snapshot(bgr_aligner* a, const char* who, uint64_t room, Rows<W>& rows, uint64_t* used) {
    const TableDesc& d = Table<W>::d;
    const CountTable& t = Table<W>::of(a);
    uint64_t tail[4];
    const int rc = table_tail<W>(a, who, tail);
    if (rc != BGR_OK) return rc;
    rows.clear();
    *used = tail[d.tail_used];
    if (*used > room || *used == 0) return BGR_OK;
    Rows<W> slots(t.cap);
    HIP_TRY(hipMemcpy(slots.data(), t.tab, t.cap * W * 8, hipMemcpyDeviceToHost));
    for (const auto& s : slots)
        if (s[d.used_word]) rows.push_back(s);
    std::sort(rows.begin(), rows.end());   // (the keys of a table are distinct: the count never decides)
    return BGR_OK;
}
static bgr_link link_record(const std::array<uint64_t, 2>& r) { return bgr_link{bgr::links_key_from(r[0]), bgr::links_key_to(r[0]), r[1]}; }
static bgr_triple triple_record(const std::array<uint64_t, 3>& r) { return bgr_triple{bgr::links_key_from(r[0]), bgr::links_key_to(r[0]), bgr::triples_key_to(r[1]), 0, r[2]}; }
void triples_records(const Rows<3>& rows, bgr_triple* out) { std::transform(rows.begin(), rows.end(), out, triple_record); }

template <size_t W, class Out, class Conv>
static int table_deliver(bgr_aligner* a, Out* out, uint64_t cap, uint64_t* n, Conv conv) {
    const std::string who = name_of<W>("bgr_aligner_");
    if (n) *n = 0;
    if (!a || !n || (cap && !out)) return fail(BGR_E_ARG, who + ": null argument");
    Rows<W> rows;
    uint64_t used = 0;
    if (const int rc = table_snapshot<W>(a, who.c_str(), cap, rows, &used); rc != BGR_OK) return rc;
    if (const int rc = rows_refusal(used, cap, n, who.c_str(), Table<W>::d.noun); rc != BGR_OK) return rc;
    if (rows.size() != used) return fail(BGR_E_INTERNAL, who + ": the table's used slots and their counter disagree");
    std::transform(rows.begin(), rows.end(), out, conv);
    return BGR_OK;
}

template <size_t W>
static int table_info(bgr_aligner* a, uint64_t out[4]) {
    const std::string who = name_of<W>("bgr_aligner_", "_info");
    if (!a || !out) return fail(BGR_E_ARG, who + ": null argument");
    uint64_t tail[4] = {0, 0, 0, 0};
    const int rc = table_tail<W>(a, who.c_str(), tail);
    if (rc != BGR_OK && rc != BGR_E_CAPACITY) return rc;   // (an overflow is what this call reports)
    out[0] = Table<W>::of(a).cap; out[1] = Table<W>::of(a).bound; out[2] = tail[0]; out[3] = tail[1];
    return BGR_OK;
}

template <size_t W>
static int table_reset(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, name_of<W>("bgr_aligner_reset_") + ": null aligner");
    const DevBuf& b = Table<W>::of(a).buf;
    if (!b.p) return BGR_OK;
    if (const int rc = sync_all(a); rc != BGR_OK) return rc;   // (the twins add to the same table)
    HIP_TRY(hipMemsetAsync(b.p, 0, b.cap, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return BGR_OK;
}

// what a whole run calls (run_counts.h, through capi_abundance.hip)
template <size_t W>
static void run_table_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    Table<W>::of(g).forget();
}
template <size_t W>
static int run_table_collect(bgr_graph* g, bgr_aligner* a) {
    Rows<W> rows;
    uint64_t used = 0;
    if (const int rc = table_snapshot<W>(a, "bgr_align_all", ~0ull, rows, &used); rc != BGR_OK) return rc;
    std::lock_guard<std::mutex> l(g->abundance_m);
    Rows<W>& all = Table<W>::of(g).rows;
    all.insert(all.end(), rows.begin(), rows.end());
    return BGR_OK;
}
template <size_t W>
static int run_table_end(bgr_graph* g, bool ok) {   // the aligners' tables, one behind the other: sorted, equal keys summed
    std::lock_guard<std::mutex> l(g->abundance_m);
    CountRows<W>& t = Table<W>::of(g);
    if (!ok) t.forget();
    else {
        Rows<W>& r = t.rows;
        std::sort(r.begin(), r.end());
        size_t w = 0;
        for (size_t i = 0; i < r.size(); ++i) {
            if (w && std::equal(r[i].begin(), r[i].end() - 1, r[w - 1].begin())) r[w - 1][W - 1] += r[i][W - 1];
            else r[w++] = r[i];
        }
        r.resize(w);
    }
    t.valid = ok;
    return BGR_OK;
}

template <size_t W>
static int graph_table_enable(bgr_graph* g, uint32_t on) {
    const std::string who = name_of<W>("bgr_graph_", "_enable");
    if (!g) return fail(BGR_E_ARG, who + ": null graph");
    if (on && g->host.blob.empty()) return fail(BGR_E_ARG, who + ": the graph has no host blob (the table of " + Table<W>::d.noun + " is sized from it)");
    Table<W>::of(g).on = on != 0;
    return BGR_OK;
}

// ---- the two instances behind the interface's names ---------------------------------------------------------------------------------------------
int bgr_graph_links_bound(bgr_graph* g, uint64_t* bound) { return graph_bound_checked<2>(g, bound); }
int bgr_aligner_links_enable(bgr_aligner* a, uint32_t on) { return table_enable<2>(a, on); }
int bgr_aligner_links(bgr_aligner* a, bgr_link* out, uint64_t cap, uint64_t* n) {
    static_assert(sizeof(bgr_link) == 16, "two ids and a 64-bit count");
    return table_deliver<2>(a, out, cap, n, link_record);
}
int bgr_aligner_links_info(bgr_aligner* a, uint64_t out[4]) { return table_info<2>(a, out); }
int bgr_aligner_reset_links(bgr_aligner* a) { return table_reset<2>(a); }
void run_links_begin(bgr_graph* g) { run_table_begin<2>(g); }
int run_links_collect(bgr_graph* g, bgr_aligner* a) { return run_table_collect<2>(g, a); }
int run_links_end(bgr_graph* g, bool ok) { return run_table_end<2>(g, ok); }
int bgr_graph_links_enable(bgr_graph* g, uint32_t on) { return graph_table_enable<2>(g, on); }
int bgr_graph_links_enabled(const bgr_graph* g) { return g && g->links.on ? 1 : 0; }
int bgr_graph_links(const bgr_graph* g, bgr_link* out, uint64_t cap, uint64_t* n) { return graph_rows(g, &bgr_graph::links, out, cap, n, "bgr_graph_links", "links", "totals", link_record); }

int bgr_graph_triples_bound(bgr_graph* g, uint64_t* bound) { return graph_bound_checked<3>(g, bound); }
int bgr_aligner_triples_enable(bgr_aligner* a, uint32_t on) { return table_enable<3>(a, on); }
int bgr_aligner_triples(bgr_aligner* a, bgr_triple* out, uint64_t cap, uint64_t* n) {
    static_assert(sizeof(bgr_triple) == 24, "three ids, a reserved word and a 64-bit count");
    return table_deliver<3>(a, out, cap, n, triple_record);
}
int bgr_aligner_triples_info(bgr_aligner* a, uint64_t out[4]) { return table_info<3>(a, out); }
int bgr_aligner_reset_triples(bgr_aligner* a) { return table_reset<3>(a); }
void run_triples_begin(bgr_graph* g) { run_table_begin<3>(g); }
int run_triples_collect(bgr_graph* g, bgr_aligner* a) { return run_table_collect<3>(g, a); }
int run_triples_end(bgr_graph* g, bool ok) { return run_table_end<3>(g, ok); }
int bgr_graph_triples_enable(bgr_graph* g, uint32_t on) { return graph_table_enable<3>(g, on); }
int bgr_graph_triples_enabled(const bgr_graph* g) { return g && g->triples.on ? 1 : 0; }
int bgr_graph_triples(const bgr_graph* g, bgr_triple* out, uint64_t cap, uint64_t* n) { return graph_rows(g, &bgr_graph::triples, out, cap, n, "bgr_graph_triples", "triples", "totals", triple_record); }

// ---- links only (bgr_link in include/bgreat_gpu.h has the definition) -------------------------------------------------------------------------
int bgr_link_canonical(int32_t a, int32_t b, bgr_link* out, uint64_t* key) {
    if (!out || a == 0 || b == 0 || a == INT32_MIN || b == INT32_MIN || std::abs((int64_t)a) >= 0x40000000 || std::abs((int64_t)b) >= 0x40000000)
        return fail(BGR_E_ARG, "bgr_link_canonical: null argument or an id that is 0 or beyond 2^30");
    const uint64_t c = bgr::links_canonical(a, b);   // (the function the kernel calls)
    *out = bgr_link{bgr::links_key_from(c), bgr::links_key_to(c), 0};
    if (key) *key = c;
    return BGR_OK;
}

int bgr_aligner_links_plan(bgr_aligner* a, uint64_t n_reads, uint32_t out[4]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_links_plan: null argument");
    uint64_t bound = a->sh->links.bound;
    if (!a->sh->links.tab) { const int rc = graph_bound<2>(a->graph, &bound); if (rc != BGR_OK) return rc; }
    const bgr::LinksPlan lp = bgr::plan_links(bound, n_reads, (uint32_t)a->num_cus, (uint32_t)a->sh->knob_links_form);
    out[0] = lp.form; out[1] = lp.blocks; out[2] = lp.threads; out[3] = lp.lds_bytes;
    return BGR_OK;
}

int bgr_plan_links(uint64_t links_bound, uint64_t n_reads, uint32_t num_cus, uint32_t form_knob, uint32_t out[4]) {
    if (!out || form_knob > 2) return fail(BGR_E_ARG, "bgr_plan_links: null argument or a form beyond 2");
    const bgr::LinksPlan lp = bgr::plan_links(links_bound, n_reads, num_cus, form_knob);
    out[0] = lp.form; out[1] = lp.blocks; out[2] = lp.threads; out[3] = lp.lds_bytes;
    return BGR_OK;
}

int bgr_write_gfa(const char* path, const bgr_graph* g, const bgr_unitig_abundance* rows, uint64_t n_rows, const bgr_link* links, uint64_t n_links) {
    if (!path || !g || (n_rows && !rows) || (n_links && !links)) return fail(BGR_E_ARG, "bgr_write_gfa: null argument");
    if (n_rows != g->header.n_unitigs) return fail(BGR_E_ARG, "bgr_write_gfa: n_rows is not the graph's number of unitigs");
    if (g->ascii_offs.empty() && n_rows) return fail(BGR_E_ARG, "bgr_write_gfa: this graph was created from a blob and carries no unitig characters");
    for (uint64_t i = 0; i < n_links; ++i) {
        const bgr_link& l = links[i];
        if (l.from == 0 || l.to == 0 || l.from == INT32_MIN || l.to == INT32_MIN || (uint64_t)std::abs((int64_t)l.from) > n_rows || (uint64_t)std::abs((int64_t)l.to) > n_rows)
            return fail(BGR_E_ARG, "bgr_write_gfa: a link names a unitig the graph does not have");
        if (i && bgr::links_pack(links[i - 1].from, links[i - 1].to) >= bgr::links_pack(l.from, l.to)) return fail(BGR_E_ARG, "bgr_write_gfa: the links are not sorted by key");
    }
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string("bgr_write_gfa: cannot open ") + path);
    std::string buf = "H\tVN:Z:1.0\n";
    bool ok = true;
    auto drain = [&](bool all) { if (ok && (all ? !buf.empty() : buf.size() > (1u << 20))) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); } };
    for (uint64_t i = 0; i < n_rows && ok; ++i) {
        const uint64_t b = g->ascii_offs[i], e = g->ascii_offs[i + 1];
        buf += "S\t"; buf += std::to_string(i + 1); buf += '\t';
        buf.append(g->ascii.data() + b, e - b);
        buf += "\tLN:i:"; buf += std::to_string(e - b);
        buf += "\tRC:i:"; buf += std::to_string(rows[i].reads);
        buf += "\tKC:i:"; buf += std::to_string(rows[i].kmers); buf += '\n';
        drain(false);
    }
    const std::string overlap = std::to_string(g->header.k - 1) + "M";
    for (uint64_t i = 0; i < n_links && ok; ++i) {
        const bgr_link& l = links[i];
        if (!l.count) continue;
        buf += "L\t"; buf += std::to_string(std::abs((int64_t)l.from)); buf += l.from < 0 ? "\t-\t" : "\t+\t";
        buf += std::to_string(std::abs((int64_t)l.to)); buf += l.to < 0 ? "\t-\t" : "\t+\t";
        buf += overlap; buf += "\tRC:i:"; buf += std::to_string(l.count); buf += '\n';
        drain(false);
    }
    drain(true);
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string("bgr_write_gfa: write to ") + path + " failed");
    return BGR_OK;
}
