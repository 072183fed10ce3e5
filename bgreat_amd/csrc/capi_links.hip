// capi_links.hip -- the C-ABI's links (bgr_link in include/bgreat_gpu.h has the definition): the aligners' hash tables, the run's totals
// in the graph object, the GFA writer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_internal.h"
#include "links_kernels.h"

// ---- links (bgr_link in include/bgreat_gpu.h has the definition) ---------------------------------------------------------------------------
static int graph_links_bound(bgr_graph* g, uint64_t* bound) {
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_links_bound: the graph has no host blob (the bound is counted over its slots)");
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (!g->links_bound_known) { g->links_bound = bgr::links_bound_of_blob(g->host.header(), g->host.base()); g->links_bound_known = true; }
    *bound = g->links_bound;
    return BGR_OK;
}
int bgr_graph_links_bound(bgr_graph* g, uint64_t* bound) {
    if (!g || !bound) return fail(BGR_E_ARG, "bgr_graph_links_bound: null argument");
    return graph_links_bound(g, bound);
}

int bgr_link_canonical(int32_t a, int32_t b, bgr_link* out, uint64_t* key) {
    if (!out || a == 0 || b == 0 || a == INT32_MIN || b == INT32_MIN || std::abs((int64_t)a) >= 0x40000000 || std::abs((int64_t)b) >= 0x40000000)
        return fail(BGR_E_ARG, "bgr_link_canonical: null argument or an id that is 0 or beyond 2^30");
    const uint64_t c = bgr::links_canonical(a, b);   // (the function the kernel calls)
    *out = bgr_link{bgr::links_key_from(c), bgr::links_key_to(c), 0};
    if (key) *key = c;
    return BGR_OK;
}

void links_share(bgr_aligner* a) {   // the twins add to the aligner's table
    for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) { tw->links_tab = a->links_tab; tw->links_cap = a->links_cap; tw->links_bound = a->links_bound; tw->links_on = a->links_on; }
}

int bgr_aligner_links_enable(bgr_aligner* a, uint32_t on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_links_enable: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_links_enable: an internal stream of another aligner");
    if (on && !a->links_tab) {
        uint64_t bound = 0;
        const int rc = graph_links_bound(a->graph, &bound);
        if (rc != BGR_OK) return rc;
        uint64_t cap = bgr::links_capacity(bound);
        if (const int64_t c = bgr::opt("test.links_capacity")) { cap = 2; while (cap < (uint64_t)c) cap <<= 1; }
        HIP_TRY(hipSetDevice(a->device));
        const hipError_t e = a->links.ensure(bgr::links_table_bytes(cap));
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, "bgr_aligner_links_enable: " + std::to_string(bgr::links_table_bytes(cap)) + " bytes for the table of links: " + hipGetErrorString(e));
        HIP_TRY(hipMemsetAsync(a->links.p, 0, a->links.cap, a->stream));   // (on the aligner's own stream, as bgr_aligner_reset_counters)
        HIP_TRY(hipStreamSynchronize(a->stream));
        a->links_tab = static_cast<unsigned long long*>(a->links.p);
        a->links_cap = cap;
        a->links_bound = bound;
    }
    a->links_on = on != 0;
    links_share(a);
    return BGR_OK;
}

// the words behind the aligner's table (links_kernels.h), every stream that adds to it waited for; BGR_E_CAPACITY when the overflow word is set
int links_tail(bgr_aligner* a, const char* who, uint64_t* tail) {   // (tail: bgr::kLinksTailWords words; capi_bubbles.hip calls it too)
    if (!a->links_tab) return fail(BGR_E_ARG, std::string(who) + ": links were never enabled on this aligner (bgr_aligner_links_enable)");
    if (const int rc = sync_all(a); rc != BGR_OK) return rc;
    HIP_TRY(hipMemcpy(tail, a->links_tab + 2 * a->links_cap, bgr::kLinksTailWords * 8, hipMemcpyDeviceToHost));
    if (tail[0])
        return fail(BGR_E_CAPACITY, std::string(who) + ": the table of links (" + std::to_string(a->links_cap) + " slots) was full: " + std::to_string(tail[0]) +
                                        " traversals found no place; the counts are incomplete until bgr_aligner_reset_links");
    return BGR_OK;
}
// ... and the table as it stands: the used slots as {key, count}, sorted by key.  Only if there are at most `room` of them (the kernel counts the
// slots it claims): a caller that asks for the number first does not pay for the table's way to the host twice
static int links_snapshot(bgr_aligner* a, const char* who, uint64_t room, std::vector<std::pair<uint64_t, uint64_t>>& kv, uint64_t tail[bgr::kLinksTailWords]) {
    const int rc = links_tail(a, who, tail);
    if (rc != BGR_OK) return rc;
    kv.clear();
    if (tail[2] > room || tail[2] == 0) return BGR_OK;
    std::vector<uint64_t> t(2 * a->links_cap);
    HIP_TRY(hipMemcpy(t.data(), a->links_tab, t.size() * 8, hipMemcpyDeviceToHost));
    for (uint64_t s = 0; s < a->links_cap; ++s)
        if (t[2 * s]) kv.emplace_back(t[2 * s], t[2 * s + 1]);
    std::sort(kv.begin(), kv.end());
    return BGR_OK;
}
static void links_deliver(const std::vector<std::pair<uint64_t, uint64_t>>& kv, bgr_link* out) {
    for (size_t i = 0; i < kv.size(); ++i) out[i] = bgr_link{bgr::links_key_from(kv[i].first), bgr::links_key_to(kv[i].first), kv[i].second};
}

int bgr_aligner_links(bgr_aligner* a, bgr_link* out, uint64_t cap, uint64_t* n) {
    static_assert(sizeof(bgr_link) == 16, "two ids and a 64-bit count");
    if (n) *n = 0;
    if (!a || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_aligner_links: null argument");
    std::vector<std::pair<uint64_t, uint64_t>> kv;
    uint64_t tail[bgr::kLinksTailWords];
    const int rc = links_snapshot(a, "bgr_aligner_links", cap, kv, tail);
    if (rc != BGR_OK) return rc;
    *n = tail[2];
    if (tail[2] > cap) return fail(BGR_E_CAPACITY, "bgr_aligner_links: " + std::to_string(tail[2]) + " links, room for " + std::to_string(cap));
    if (kv.size() != tail[2]) return fail(BGR_E_INTERNAL, "bgr_aligner_links: the table's used slots and their counter disagree");
    links_deliver(kv, out);
    return BGR_OK;
}

int bgr_aligner_links_info(bgr_aligner* a, uint64_t out[4]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_links_info: null argument");
    uint64_t tail[bgr::kLinksTailWords] = {0, 0, 0};
    const int rc = links_tail(a, "bgr_aligner_links_info", tail);
    if (rc != BGR_OK && rc != BGR_E_CAPACITY) return rc;   // (an overflow is what this call reports)
    out[0] = a->links_cap; out[1] = a->links_bound; out[2] = tail[0]; out[3] = tail[1];
    return BGR_OK;
}

int bgr_aligner_links_plan(bgr_aligner* a, uint64_t n_reads, uint32_t out[4]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_links_plan: null argument");
    uint64_t bound = a->links_bound;
    if (!a->links_tab) { const int rc = graph_links_bound(a->graph, &bound); if (rc != BGR_OK) return rc; }
    const bgr::LinksPlan lp = bgr::plan_links(bound, n_reads, (uint32_t)a->num_cus, a->knob_links_form);
    out[0] = lp.form; out[1] = lp.blocks; out[2] = lp.threads; out[3] = lp.lds_bytes;
    return BGR_OK;
}

int bgr_plan_links(uint64_t links_bound, uint64_t n_reads, uint32_t num_cus, uint32_t form_knob, uint32_t out[4]) {
    if (!out || form_knob > 2) return fail(BGR_E_ARG, "bgr_plan_links: null argument or a form beyond 2");
    const bgr::LinksPlan lp = bgr::plan_links(links_bound, n_reads, num_cus, form_knob);
    out[0] = lp.form; out[1] = lp.blocks; out[2] = lp.threads; out[3] = lp.lds_bytes;
    return BGR_OK;
}

int bgr_aligner_reset_links(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_reset_links: null aligner");
    if (!a->links.p) return BGR_OK;
    if (const int rc = sync_all(a); rc != BGR_OK) return rc;   // (the twins add to the same table)
    HIP_TRY(hipMemsetAsync(a->links.p, 0, a->links.cap, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return BGR_OK;
}

// what a whole run calls (run_counts.h, through capi_abundance.hip)
void run_links_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->links.clear();
    g->links_valid = false;
}
int run_links_collect(bgr_graph* g, bgr_aligner* a) {
    std::vector<std::pair<uint64_t, uint64_t>> kv;
    uint64_t tail[bgr::kLinksTailWords];
    const int rc = links_snapshot(a, "bgr_align_all", ~0ull, kv, tail);
    if (rc != BGR_OK) return rc;
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->links.insert(g->links.end(), kv.begin(), kv.end());
    return BGR_OK;
}
void run_links_end(bgr_graph* g, bool ok) {   // the aligners' tables, one behind the other: sorted, equal keys summed
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (!ok) g->links.clear();
    else {
        std::sort(g->links.begin(), g->links.end());
        size_t w = 0;
        for (size_t i = 0; i < g->links.size(); ++i) {
            if (w && g->links[w - 1].first == g->links[i].first) g->links[w - 1].second += g->links[i].second;
            else g->links[w++] = g->links[i];
        }
        g->links.resize(w);
    }
    g->links_valid = ok;
}

int bgr_graph_links_enable(bgr_graph* g, uint32_t on) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_links_enable: null graph");
    if (on && g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_links_enable: the graph has no host blob (the table of links is sized from it)");
    g->links_on = on != 0;
    return BGR_OK;
}

int bgr_graph_links_enabled(const bgr_graph* g) { return g && g->links_on ? 1 : 0; }

int bgr_graph_links(const bgr_graph* g, bgr_link* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!g || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_graph_links: null argument");
    if (!g->links_valid) return fail(BGR_E_ARG, "bgr_graph_links: no totals -- they are those of the last successful bgr_align_all with bgr_graph_links_enable on");
    *n = g->links.size();
    if (g->links.size() > cap) return fail(BGR_E_CAPACITY, "bgr_graph_links: " + std::to_string(g->links.size()) + " links, room for " + std::to_string(cap));
    links_deliver(g->links, out);
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
