// capi_bubbles.hip -- the C-ABI's bubbles (bgr_bubble in include/bgreat_gpu.h has the definition; bubbles_kernels.h the passes): the calls on an
// uploaded list of links and on an aligner's live table, the run's bubbles in the graph object, the writer.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bubbles_kernels.h"
#include "capi_internal.h"
#include "links_kernels.h"

// the four launches over `n_pairs` {key, count} pairs in HBM on the call's stream, then the records' way to the host: into `vec` (as many as there
// are), or into `out` when they are at most `cap`.  *n = their number in any case.  ms: null, or the four launches' milliseconds (the first with the
// memset of the degrees in front of it).  The scratch lives for the call (c.buf[1], c.buf[2]; c.buf[0] is the caller's)
static int bubbles_call(DeviceCall& c, const unsigned long long* pairs, uint64_t n_pairs, uint64_t n_unitigs, uint64_t min_link, const char* who, std::vector<bgr_bubble>* vec, bgr_bubble* out,
                        uint64_t cap, uint64_t* n, double* ms) {
    static_assert(sizeof(bgr_bubble) == 48, "four ids and four 64-bit counts");
    const std::string w = who;
    *n = 0;
    if (ms) for (int i = 0; i < 4; ++i) ms[i] = 0;
    if (vec) vec->clear();
    if (n_unitigs == 0) return BGR_OK;
    DevBuf &scratch = c.buf[1], &outbuf = c.buf[2];
    if (!c.room(scratch, bgr::bubbles_scratch_bytes(n_unitigs), w + ": " + std::to_string(bgr::bubbles_scratch_bytes(n_unitigs)) + " bytes for the adjacency of " + std::to_string(n_unitigs) + " unitigs"))
        return c.rc;
    hipEvent_t* const ev = c.ev;
    if (ms) {
        if (const int rc = c.events(5); rc != BGR_OK) return rc;
        HIP_TRY(hipEventRecord(ev[0], c.s));
    }
    hipError_t e = bgr::launch_bubbles_count(pairs, n_pairs, n_unitigs, min_link, scratch.p, c.s, ms ? ev + 1 : nullptr);
    if (e != hipSuccess) return fail(BGR_E_HIP, w + ": kernel launch (bgr_bubbles_*_kernel): " + hipGetErrorString(e));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, bgr::bubbles_total_word(scratch.p, n_unitigs), 8, hipMemcpyDeviceToHost, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    *n = total;
    if (total > 2 * n_unitigs) return fail(BGR_E_INTERNAL, w + ": more bubbles than oriented ids");
    if (!vec) if (const int rc = rows_refusal(total, cap, n, who, "bubbles"); rc != BGR_OK) return rc;
    if (total) {
        if (!c.room(outbuf, total * sizeof(bgr_bubble), w + ": " + std::to_string(total) + " bubble records on the device")) return c.rc;
        e = bgr::launch_bubbles_emit(n_unitigs, scratch.p, static_cast<bgr_bubble*>(outbuf.p), c.s);
        if (e != hipSuccess) return fail(BGR_E_HIP, w + ": kernel launch (bgr_bubbles_classify_kernel, emit): " + hipGetErrorString(e));
        if (ms) HIP_TRY(hipEventRecord(ev[4], c.s));
        if (vec) { vec->resize(total); out = vec->data(); }
        HIP_TRY(hipMemcpyAsync(out, outbuf.p, total * sizeof(bgr_bubble), hipMemcpyDeviceToHost, c.s));
        HIP_TRY(hipStreamSynchronize(c.s));
    }
    if (ms)
        for (int i = 0; i < (total ? 4 : 3); ++i) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, ev[i], ev[i + 1])); ms[i] = f; }
    return BGR_OK;
}

// a dense list of {key, count} pairs on the host: uploaded to `device` on a stream of its own, called there, everything freed
static int bubbles_of_pairs(int device, const std::array<uint64_t, 2>* kv, uint64_t n_pairs, uint64_t n_unitigs, uint64_t min_link, const char* who, std::vector<bgr_bubble>* vec,
                            bgr_bubble* out, uint64_t cap, uint64_t* n) {
    static_assert(sizeof(std::array<uint64_t, 2>) == 16, "{key, count} as the table holds them");
    HIP_TRY(hipSetDevice(device));
    DeviceCall c;
    if (const int rc = c.own_stream(); rc != BGR_OK) return rc;
    if (!c.room(c.buf[0], n_pairs * 16, std::string(who) + ": " + std::to_string(n_pairs) + " links on the device")) return c.rc;
    HIP_TRY(hipMemcpyAsync(c.buf[0].p, kv, n_pairs * 16, hipMemcpyHostToDevice, c.s));
    return bubbles_call(c, static_cast<const unsigned long long*>(c.buf[0].p), n_pairs, n_unitigs, min_link, who, vec, out, cap, n, nullptr);
}

int bgr_links_bubbles(int device, const bgr_link* links, uint64_t n_links, uint64_t n_unitigs, uint64_t min_link, bgr_bubble* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!n || (n_links && !links) || (cap && !out)) return fail(BGR_E_ARG, "bgr_links_bubbles: null argument");
    if (min_link == 0) return fail(BGR_E_ARG, "bgr_links_bubbles: min_link is at least 1");
    if (n_unitigs >= 0x40000000ull) return fail(BGR_E_ARG, "bgr_links_bubbles: fewer than 2^30 unitigs");
    if (device < 0) return fail(BGR_E_ARG, "bgr_links_bubbles: a negative device");
    std::vector<std::array<uint64_t, 2>> kv(n_links);
    for (uint64_t i = 0; i < n_links; ++i) {
        const bgr_link& l = links[i];
        if (l.from == 0 || l.to == 0 || l.from == INT32_MIN || l.to == INT32_MIN || (uint64_t)std::abs((int64_t)l.from) > n_unitigs || (uint64_t)std::abs((int64_t)l.to) > n_unitigs)
            return fail(BGR_E_ARG, "bgr_links_bubbles: link " + std::to_string(i) + " names a unitig outside 1 .. n_unitigs");
        kv[i] = {bgr::links_pack(l.from, l.to), l.count};
        if (kv[i][0] != bgr::links_canonical(l.from, l.to)) return fail(BGR_E_ARG, "bgr_links_bubbles: link " + std::to_string(i) + " is not canonical (bgr_link_canonical)");
        if (i && kv[i - 1][0] >= kv[i][0]) return fail(BGR_E_ARG, "bgr_links_bubbles: the links are not strictly ascending by key");
    }
    if (n_links == 0) return BGR_OK;   // (no link, no bubble: no device work)
    return bubbles_of_pairs(device, kv.data(), n_links, n_unitigs, min_link, "bgr_links_bubbles", nullptr, out, cap, n);
}

int bgr_aligner_bubbles(bgr_aligner* a, uint64_t min_link, bgr_bubble* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!a || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_aligner_bubbles: null argument");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_bubbles: an internal stream of another aligner");
    if (min_link == 0) return fail(BGR_E_ARG, "bgr_aligner_bubbles: min_link is at least 1");
    uint64_t tail[bgr::kLinksTailWords];
    if (const int rc = links_tail(a, "bgr_aligner_bubbles", tail); rc != BGR_OK) return rc;   // (links never enabled; every stream that adds waited for; the overflow word)
    for (int i = 0; i < 4; ++i) a->bub_ms[i] = 0;
    if (tail[2] == 0) return BGR_OK;   // (an empty table: the passes would read every slot to find nothing)
    DeviceCall c(a->stream);   // (on the aligner's own stream, behind its launches; links_tail has made its device current)
    return bubbles_call(c, a->sh->links.tab, a->sh->links.cap, a->graph->header.n_unitigs, min_link, "bgr_aligner_bubbles", nullptr, out, cap, n, a->sh->knob_no_events ? nullptr : a->bub_ms);
}

int bgr_aligner_bubbles_times(bgr_aligner* a, double ms[4]) {
    if (!a || !ms) return fail(BGR_E_ARG, "bgr_aligner_bubbles_times: null argument");
    for (int i = 0; i < 4; ++i) ms[i] = a->bub_ms[i];
    return BGR_OK;
}

// ---- what a whole run calls (run_counts.h, through capi_abundance.hip) ---------------------------------------------------------------------
void run_bubbles_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->bubbles.forget();
    g->bubbles.device = -1;
}
int run_bubbles_collect(bgr_graph* g, bgr_aligner* a) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (g->bubbles.device < 0) g->bubbles.device = a->device;
    return BGR_OK;
}
int run_bubbles_end(bgr_graph* g, bool ok) {   // behind run_links_end: g->links.rows is merged and sorted, the {key, count} pairs as the kernels read them
    std::lock_guard<std::mutex> l(g->abundance_m);
    return chain_stage_end(g, g->bubbles, ok, g->links.valid, "bubbles without the links they are called from", !g->links.rows.empty(), "links", [&] {
        uint64_t n = 0;
        return bubbles_of_pairs(g->bubbles.device, g->links.rows.data(), g->links.rows.size(), g->header.n_unitigs, run_thresholds(g).link, "bgr_align_all", &g->bubbles.rows, nullptr, 0, &n);
    });
}

int bgr_graph_bubbles_enable(bgr_graph* g, uint32_t on, uint64_t min_link) {
    const ChainMins given = {min_link, 1, 1};
    if (const int rc = chain_refusal(g, "bgr_graph_bubbles_enable", on, given, "the table of links is sized from it",
                                     "bubbles (--bubbles) need a graph of ACGT-only unitigs: on one with other characters a branch read backwards does not spell the reverse complement");
        rc != BGR_OK)
        return rc;
    g->bubbles.set(on, given);
    return BGR_OK;
}

int bgr_graph_bubbles_enabled(const bgr_graph* g) { return g && g->bubbles.on ? 1 : 0; }

int bgr_graph_bubbles(const bgr_graph* g, bgr_bubble* out, uint64_t cap, uint64_t* n) { return graph_rows(g, &bgr_graph::bubbles, out, cap, n, "bgr_graph_bubbles", "bubbles", "totals"); }

int bgr_write_bubbles(const char* path, const bgr_graph* g, const bgr_bubble* bubbles, uint64_t n) {
    if (!path || !g || (n && !bubbles)) return fail(BGR_E_ARG, "bgr_write_bubbles: null argument");
    if (g->ascii_offs.empty()) return fail(BGR_E_ARG, "bgr_write_bubbles: this graph was created from a blob and carries no unitig characters");
    const uint64_t nu = g->header.n_unitigs;
    for (uint64_t i = 0; i < n; ++i) {
        const int32_t ids[4] = {bubbles[i].source, bubbles[i].sink, bubbles[i].branch[0], bubbles[i].branch[1]};
        for (int32_t x : ids)
            if (x == 0 || x == INT32_MIN || (uint64_t)std::abs((int64_t)x) > nu) return fail(BGR_E_ARG, "bgr_write_bubbles: record " + std::to_string(i) + " names a unitig the graph does not have");
    }
    std::string kind, diff;
    auto oriented = [&](int32_t id) {
        const uint64_t u = (uint64_t)std::abs((int64_t)id) - 1, b = g->ascii_offs[u], e = g->ascii_offs[u + 1];
        return bgr::bubbles_oriented(g->ascii.data() + b, e - b, id < 0);
    };
    return write_lines("bgr_write_bubbles", path, "#source\tsink\tbranch1\tbranch2\tlen1\tlen2\tin1\tout1\tin2\tout2\tkind\tdiff\n", n, [&](uint64_t i, std::string* buf) {
        const bgr_bubble& r = bubbles[i];
        const std::string x = oriented(r.branch[0]), y = oriented(r.branch[1]);
        bgr::bubbles_compare(x, y, &kind, &diff);
        *buf += std::to_string(r.source); *buf += '\t'; *buf += std::to_string(r.sink); *buf += '\t';
        *buf += std::to_string(r.branch[0]); *buf += '\t'; *buf += std::to_string(r.branch[1]); *buf += '\t';
        *buf += std::to_string(x.size()); *buf += '\t'; *buf += std::to_string(y.size());
        for (int j = 0; j < 4; ++j) { *buf += '\t'; *buf += std::to_string(r.count[j]); }
        *buf += '\t'; *buf += kind; *buf += '\t'; *buf += diff; *buf += '\n';
    });
}
