// capi_inside.hip -- the inside index and the pass that reads it (include/bgreat_gpu.h: bgr_graph_inside_*, bgr_aligner_inside_*): the host table
// (inside_index.cpp) kept in the graph object in a buffer of its own, its copy on each device an enabled aligner lives on, the aligner's switch
// and count, and the graph's sticky switch for whole runs.  The launch itself is queued by align_device_impl (capi.hip), behind the mapping passes.
#include "capi_internal.h"
#include "inside_kernels.h"

int bgr_graph_inside_build(bgr_graph* g) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_inside_build: null graph");
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (g->inside.tab) return BGR_OK;   // (sticky: built once)
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_inside_build: the graph has no host blob (the index is built from the 2-bit store on the host)");
    std::string err;
    const int rc = bgr::build_inside_index(g->host.header(), g->host.base(), bgr::build_threads(), g->inside, err);
    if (rc == 1) return fail(BGR_E_ARG, "bgr_graph_inside_build: " + err);
    if (rc != 0) return fail(BGR_E_NOMEM, "bgr_graph_inside_build: " + err);
    return BGR_OK;
}

int bgr_graph_inside_info(const bgr_graph* g, bgr_inside_info* out) {
    if (!g || !out) return fail(BGR_E_ARG, "bgr_graph_inside_info: null argument");
    memset(out, 0, sizeof(*out));
    out->entries = g->inside.entries;
    out->slots = g->inside.slots;
    out->bytes = g->inside.bytes();
    out->build_seconds = g->inside.build_seconds;
    return BGR_OK;
}

int bgr_graph_inside_lookup(const bgr_graph* g, uint64_t kmer, uint32_t* unitig, uint32_t* offset, uint32_t* forward_canonical, uint32_t* found) {
    if (!g || !found) return fail(BGR_E_ARG, "bgr_graph_inside_lookup: null argument");
    if (!g->inside.tab) return fail(BGR_E_ARG, "bgr_graph_inside_lookup: the graph has no inside index (bgr_graph_inside_build)");
    uint64_t val = 0;
    const bool have = bgr::inside_lookup(g->inside, g->header.k, kmer, &val);
    *found = have ? 1u : 0u;
    if (unitig) *unitig = have ? bgr_inside_id(val) : 0u;
    if (offset) *offset = have ? bgr_inside_off(val) : 0u;
    if (forward_canonical) *forward_canonical = have ? (uint32_t)(val & BGR_INSIDE_FWD_CANON) : 0u;
    return BGR_OK;
}

void inside_free_devices(bgr_graph* g) {
    for (auto& kv : g->inside_dev)
        if (kv.second && hipSetDevice(kv.first) == hipSuccess) (void)hipFree(kv.second);
    g->inside_dev.clear();
}

// the index on `device`, uploaded the first time it is asked for there
static int inside_on_device(bgr_graph* g, int device, const BgrInsideEntry** out) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    auto it = g->inside_dev.find(device);
    if (it == g->inside_dev.end()) {
        HIP_TRY(hipSetDevice(device));
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, g->inside.bytes());
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string("bgr_aligner_inside_enable: the inside index on the device: ") + hipGetErrorString(e));
        }
        const hipError_t c = hipMemcpy(p, g->inside.tab, g->inside.bytes(), hipMemcpyHostToDevice);
        if (c != hipSuccess) { (void)hipFree(p); return fail(BGR_E_HIP, std::string("bgr_aligner_inside_enable: copy of the inside index: ") + hipGetErrorString(c)); }
        it = g->inside_dev.emplace(device, p).first;
    }
    *out = static_cast<const BgrInsideEntry*>(it->second);
    return BGR_OK;
}

int bgr_aligner_inside_enable(bgr_aligner* a, int on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_inside_enable: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_inside_enable: an internal twin (the switch belongs to the aligner it was made for)");
    const BgrInsideEntry* tab = nullptr;
    if (on) {
        if (!a->graph->inside.tab) return fail(BGR_E_ARG, "bgr_aligner_inside_enable: the graph has no inside index (bgr_graph_inside_build)");
        const int rc = inside_on_device(a->graph, a->device, &tab);
        if (rc != BGR_OK) return rc;
    }
    a->sh->inside_tab = tab;   // (read when a launch is queued, on whichever stream)
    a->sh->inside_slots = tab ? a->graph->inside.slots : 0;
    return BGR_OK;
}

int bgr_aligner_inside_count(bgr_aligner* a, uint64_t* n) {
    if (!a || !n) return fail(BGR_E_ARG, "bgr_aligner_inside_count: null argument");
    *n = 0;
    const int rc = sync_all(a);
    if (rc != BGR_OK) return rc;
    for (bgr_aligner* x = a; x; x = x->twin) {   // (the twins map the pieces of overlapped batches and un-waited launches)
        uint64_t c = 0;
        HIP_TRY(hipMemcpy(&c, static_cast<char*>(x->launch.small.p) + bgr::kSmallInside, 8, hipMemcpyDeviceToHost));
        *n += c;
    }
    return BGR_OK;
}

int bgr_graph_inside_enable(bgr_graph* g, int on) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_inside_enable: null graph");
    if (on && !g->inside.tab) return fail(BGR_E_ARG, "bgr_graph_inside_enable: the graph has no inside index (bgr_graph_inside_build)");
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->inside_on = on != 0;
    return BGR_OK;
}
int bgr_graph_inside_enabled(const bgr_graph* g) { return g && g->inside_on ? 1 : 0; }
int bgr_graph_inside_count(const bgr_graph* g, uint64_t* n) {
    if (!g || !n) return fail(BGR_E_ARG, "bgr_graph_inside_count: null argument");
    *n = g->inside_run;
    return BGR_OK;
}

// whole runs (run_counts.h)
void run_inside_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->inside_run = 0;
}
int run_inside_collect(bgr_graph* g, bgr_aligner* a) {
    uint64_t n = 0;
    const int rc = bgr_aligner_inside_count(a, &n);
    if (rc != BGR_OK) return rc;
    std::lock_guard<std::mutex> l(g->abundance_m);   // (the lanes of a split run end side by side)
    g->inside_run += n;
    return BGR_OK;
}
