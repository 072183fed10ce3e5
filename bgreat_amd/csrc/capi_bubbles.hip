// capi_bubbles.hip -- the C-ABI's bubbles (bgr_bubble in include/bgreat_gpu.h has the definition; bubbles_kernels.h the passes): the calls on an
// uploaded list of links and on an aligner's live table, the run's bubbles in the graph object, the writer.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bubbles_kernels.h"
#include "capi_internal.h"
#include "links_kernels.h"

// the four launches over `n_pairs` {key, count} pairs in HBM on `stream` of the current device, then the records' way to the host: into `vec` (as many
// as there are), or into `out` when they are at most `cap`.  *n = their number in any case.  ms: null, or the four launches' milliseconds (the first
// with the memset of the degrees in front of it).  The scratch lives for the call: whatever happens, nothing stays allocated
static int bubbles_call(const unsigned long long* pairs, uint64_t n_pairs, uint64_t n_unitigs, uint64_t min_link, hipStream_t stream, const char* who, std::vector<bgr_bubble>* vec,
                        bgr_bubble* out, uint64_t cap, uint64_t* n, double* ms) {
    static_assert(sizeof(bgr_bubble) == 48, "four ids and four 64-bit counts");
    *n = 0;
    if (ms) for (int i = 0; i < 4; ++i) ms[i] = 0;
    if (vec) vec->clear();
    if (n_unitigs == 0) return BGR_OK;
    struct Bufs { DevBuf scratch, outbuf; ~Bufs() { scratch.release(); outbuf.release(); } } b;
    hipError_t e = b.scratch.ensure(bgr::bubbles_scratch_bytes(n_unitigs));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": " + std::to_string(bgr::bubbles_scratch_bytes(n_unitigs)) + " bytes for the adjacency of " +
                                                                            std::to_string(n_unitigs) + " unitigs: " + hipGetErrorString(e));
    }
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 5; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } guard{ev};
    if (ms) {
        for (int i = 0; i < 5; ++i) HIP_TRY(hipEventCreate(&ev[i]));
        HIP_TRY(hipEventRecord(ev[0], stream));
    }
    e = bgr::launch_bubbles_count(pairs, n_pairs, n_unitigs, min_link, b.scratch.p, stream, ms ? ev + 1 : nullptr);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_bubbles_*_kernel): " + hipGetErrorString(e));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, bgr::bubbles_total_word(b.scratch.p, n_unitigs), 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *n = total;
    if (total > 2 * n_unitigs) return fail(BGR_E_INTERNAL, std::string(who) + ": more bubbles than oriented ids");
    if (!vec && total > cap) return fail(BGR_E_CAPACITY, std::string(who) + ": " + std::to_string(total) + " bubbles, room for " + std::to_string(cap));
    if (total) {
        e = b.outbuf.ensure(total * sizeof(bgr_bubble));
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": " + std::to_string(total) + " bubble records on the device: " + hipGetErrorString(e)); }
        e = bgr::launch_bubbles_emit(n_unitigs, b.scratch.p, static_cast<bgr_bubble*>(b.outbuf.p), stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_bubbles_classify_kernel, emit): " + hipGetErrorString(e));
        if (ms) HIP_TRY(hipEventRecord(ev[4], stream));
        if (vec) { vec->resize(total); out = vec->data(); }
        HIP_TRY(hipMemcpyAsync(out, b.outbuf.p, total * sizeof(bgr_bubble), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    if (ms)
        for (int i = 0; i < (total ? 4 : 3); ++i) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, ev[i], ev[i + 1])); ms[i] = f; }
    return BGR_OK;
}

// a dense list of pairs on the host: uploaded to `device` on a stream of its own, called there, everything freed
static int bubbles_of_pairs(int device, const std::pair<uint64_t, uint64_t>* kv, uint64_t n_pairs, uint64_t n_unitigs, uint64_t min_link, const char* who, std::vector<bgr_bubble>* vec,
                            bgr_bubble* out, uint64_t cap, uint64_t* n) {
    static_assert(sizeof(std::pair<uint64_t, uint64_t>) == 16, "{key, count} as the table holds them");
    HIP_TRY(hipSetDevice(device));
    struct Res { hipStream_t s = nullptr; DevBuf in; ~Res() { in.release(); if (s) (void)hipStreamDestroy(s); } } r;
    HIP_TRY(hipStreamCreate(&r.s));
    const hipError_t e = r.in.ensure(n_pairs * 16);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": " + std::to_string(n_pairs) + " links on the device: " + hipGetErrorString(e)); }
    HIP_TRY(hipMemcpyAsync(r.in.p, kv, n_pairs * 16, hipMemcpyHostToDevice, r.s));
    return bubbles_call(static_cast<const unsigned long long*>(r.in.p), n_pairs, n_unitigs, min_link, r.s, who, vec, out, cap, n, nullptr);
}

int bgr_links_bubbles(int device, const bgr_link* links, uint64_t n_links, uint64_t n_unitigs, uint64_t min_link, bgr_bubble* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!n || (n_links && !links) || (cap && !out)) return fail(BGR_E_ARG, "bgr_links_bubbles: null argument");
    if (min_link == 0) return fail(BGR_E_ARG, "bgr_links_bubbles: min_link is at least 1");
    if (n_unitigs >= 0x40000000ull) return fail(BGR_E_ARG, "bgr_links_bubbles: fewer than 2^30 unitigs");
    if (device < 0) return fail(BGR_E_ARG, "bgr_links_bubbles: a negative device");
    std::vector<std::pair<uint64_t, uint64_t>> kv(n_links);
    for (uint64_t i = 0; i < n_links; ++i) {
        const bgr_link& l = links[i];
        if (l.from == 0 || l.to == 0 || l.from == INT32_MIN || l.to == INT32_MIN || (uint64_t)std::abs((int64_t)l.from) > n_unitigs || (uint64_t)std::abs((int64_t)l.to) > n_unitigs)
            return fail(BGR_E_ARG, "bgr_links_bubbles: link " + std::to_string(i) + " names a unitig outside 1 .. n_unitigs");
        kv[i] = {bgr::links_pack(l.from, l.to), l.count};
        if (kv[i].first != bgr::links_canonical(l.from, l.to)) return fail(BGR_E_ARG, "bgr_links_bubbles: link " + std::to_string(i) + " is not canonical (bgr_link_canonical)");
        if (i && kv[i - 1].first >= kv[i].first) return fail(BGR_E_ARG, "bgr_links_bubbles: the links are not strictly ascending by key");
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
    return bubbles_call(a->links_tab, a->links_cap, a->graph->header.n_unitigs, min_link, a->stream, "bgr_aligner_bubbles", nullptr, out, cap, n, a->knob_no_events ? nullptr : a->bub_ms);
}

int bgr_aligner_bubbles_times(bgr_aligner* a, double ms[4]) {
    if (!a || !ms) return fail(BGR_E_ARG, "bgr_aligner_bubbles_times: null argument");
    for (int i = 0; i < 4; ++i) ms[i] = a->bub_ms[i];
    return BGR_OK;
}

// ---- what a whole run calls (run_counts.h, through capi_abundance.hip) ---------------------------------------------------------------------
void run_bubbles_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->bubbles.clear();
    g->bubbles_valid = false;
    g->bubbles_device = -1;
}
void run_bubbles_collect(bgr_graph* g, bgr_aligner* a) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (g->bubbles_device < 0) g->bubbles_device = a->device;
}
int run_bubbles_end(bgr_graph* g, bool ok) {   // behind run_links_end: g->links is merged and sorted, the {key, count} pairs as the kernels read them
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->bubbles.clear();
    g->bubbles_valid = false;
    // (a run that only phases calls its bubbles with the phase's threshold, one that only chains blocks with the blocks', one that only spells with the haplotypes')
    const uint64_t min_link = g->bubbles_on ? g->bubbles_min_link : (g->phase_on ? g->phase_min_link : (g->blocks_on ? g->blocks_min_link : (g->haplotypes_on ? g->haplotypes_min_link : g->bubbles_min_link)));
    g->bubbles_called = min_link;
    if (!ok) return BGR_OK;
    int rc = BGR_OK;
    uint64_t n = 0;
    if (!g->links_valid) rc = fail(BGR_E_INTERNAL, "bgr_align_all: bubbles without the links they are called from");
    else if (!g->links.empty()) {
        if (g->bubbles_device < 0) rc = fail(BGR_E_INTERNAL, "bgr_align_all: links, but no aligner of the run was collected");
        else rc = bubbles_of_pairs(g->bubbles_device, g->links.data(), g->links.size(), g->header.n_unitigs, min_link, "bgr_align_all", &g->bubbles, nullptr, 0, &n);
    }
    if (rc != BGR_OK) { g->bubbles.clear(); g->bubbles.shrink_to_fit(); }
    g->bubbles_valid = rc == BGR_OK;
    return rc;
}

int bgr_graph_bubbles_enable(bgr_graph* g, uint32_t on, uint64_t min_link) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_bubbles_enable: null graph");
    if (on) {
        if (min_link == 0) return fail(BGR_E_ARG, "bgr_graph_bubbles_enable: min_link is at least 1");
        if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_bubbles_enable: the graph has no host blob (the table of links is sized from it)");
        if (g->header.has_exc)
            return fail(BGR_E_ARG, "bgr_graph_bubbles_enable: bubbles (--bubbles) need a graph of ACGT-only unitigs: on one with other characters a branch read backwards does not spell the reverse complement");
        g->bubbles_min_link = min_link;
    }
    g->bubbles_on = on != 0;
    return BGR_OK;
}

int bgr_graph_bubbles_enabled(const bgr_graph* g) { return g && g->bubbles_on ? 1 : 0; }

int bgr_graph_bubbles(const bgr_graph* g, bgr_bubble* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!g || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_graph_bubbles: null argument");
    if (!g->bubbles_valid) return fail(BGR_E_ARG, "bgr_graph_bubbles: no totals -- they are those of the last successful bgr_align_all with bgr_graph_bubbles_enable on");
    *n = g->bubbles.size();
    if (g->bubbles.size() > cap) return fail(BGR_E_CAPACITY, "bgr_graph_bubbles: " + std::to_string(g->bubbles.size()) + " bubbles, room for " + std::to_string(cap));
    if (!g->bubbles.empty()) memcpy(out, g->bubbles.data(), g->bubbles.size() * sizeof(bgr_bubble));
    return BGR_OK;
}

int bgr_write_bubbles(const char* path, const bgr_graph* g, const bgr_bubble* bubbles, uint64_t n) {
    if (!path || !g || (n && !bubbles)) return fail(BGR_E_ARG, "bgr_write_bubbles: null argument");
    if (g->ascii_offs.empty()) return fail(BGR_E_ARG, "bgr_write_bubbles: this graph was created from a blob and carries no unitig characters");
    const uint64_t nu = g->header.n_unitigs;
    for (uint64_t i = 0; i < n; ++i) {
        const int32_t ids[4] = {bubbles[i].source, bubbles[i].sink, bubbles[i].branch[0], bubbles[i].branch[1]};
        for (int32_t x : ids)
            if (x == 0 || x == INT32_MIN || (uint64_t)std::abs((int64_t)x) > nu) return fail(BGR_E_ARG, "bgr_write_bubbles: record " + std::to_string(i) + " names a unitig the graph does not have");
    }
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string("bgr_write_bubbles: cannot open ") + path);
    std::string buf = "#source\tsink\tbranch1\tbranch2\tlen1\tlen2\tin1\tout1\tin2\tout2\tkind\tdiff\n", kind, diff;
    bool ok = true;
    auto oriented = [&](int32_t id) {
        const uint64_t u = (uint64_t)std::abs((int64_t)id) - 1, b = g->ascii_offs[u], e = g->ascii_offs[u + 1];
        return bgr::bubbles_oriented(g->ascii.data() + b, e - b, id < 0);
    };
    for (uint64_t i = 0; i < n && ok; ++i) {
        const bgr_bubble& r = bubbles[i];
        const std::string x = oriented(r.branch[0]), y = oriented(r.branch[1]);
        bgr::bubbles_compare(x, y, &kind, &diff);
        buf += std::to_string(r.source); buf += '\t'; buf += std::to_string(r.sink); buf += '\t';
        buf += std::to_string(r.branch[0]); buf += '\t'; buf += std::to_string(r.branch[1]); buf += '\t';
        buf += std::to_string(x.size()); buf += '\t'; buf += std::to_string(y.size());
        for (int j = 0; j < 4; ++j) { buf += '\t'; buf += std::to_string(r.count[j]); }
        buf += '\t'; buf += kind; buf += '\t'; buf += diff; buf += '\n';
        if (buf.size() > (1u << 20)) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); }
    }
    if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string("bgr_write_bubbles: write to ") + path + " failed");
    return BGR_OK;
}
