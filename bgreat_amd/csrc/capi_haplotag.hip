// capi_haplotag.hip -- the C-ABI's haplotags (bgr_read_tag in include/bgreat_gpu.h has the definition; haplotag_host.h the table builders and the
// file parser, haplotag_device.h the per-row function): the two table builders, the aligner's table on the device with the call over the last
// launch's rows, the graph's sticky copy, and the two entries through which a whole run (pipeline.cpp, run_counts.h) reaches them.
#include <cstdio>
#include <new>

#include "capi_internal.h"
#include "haplotag_host.h"
#include "haplotag_kernels.h"

int bgr_blocks_tag_table(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries, uint64_t n_entries, uint64_t n_unitigs, uint64_t min_block,
                         uint32_t* table_out, uint64_t* n_tagged_out) {
    if (n_tagged_out) *n_tagged_out = 0;
    if (!table_out || (n_bubbles && !bubbles) || (n_entries && !entries)) return fail(BGR_E_ARG, "bgr_blocks_tag_table: null argument");
    if (n_unitigs >= 0x40000000ull) return fail(BGR_E_ARG, "bgr_blocks_tag_table: fewer than 2^30 unitigs");
    std::string msg;
    if (!bgr::haplotag_table_of(bubbles, n_bubbles, entries, n_entries, n_unitigs, min_block, table_out, &msg)) return fail(BGR_E_ARG, "bgr_blocks_tag_table: " + msg);
    if (n_tagged_out) *n_tagged_out = bgr::haplotag_count(table_out, n_unitigs);
    return BGR_OK;
}

int bgr_read_blocks_tags(const char* path, uint64_t n_unitigs, uint32_t* table_out, uint64_t* n_tagged_out) {
    if (n_tagged_out) *n_tagged_out = 0;
    if (!path || !table_out) return fail(BGR_E_ARG, "bgr_read_blocks_tags: null argument");
    if (n_unitigs >= 0x40000000ull) return fail(BGR_E_ARG, "bgr_read_blocks_tags: fewer than 2^30 unitigs");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(BGR_E_IO, std::string("bgr_read_blocks_tags: cannot open ") + path);
    std::string data;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) data.append(buf, got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return fail(BGR_E_IO, std::string("bgr_read_blocks_tags: cannot read ") + path);
    std::string msg;
    if (!bgr::haplotag_table_of_text(data.data(), data.size(), n_unitigs, table_out, &msg)) return fail(BGR_E_ARG, std::string("bgr_read_blocks_tags: ") + path + ": " + msg);
    if (n_tagged_out) *n_tagged_out = bgr::haplotag_count(table_out, n_unitigs);
    return BGR_OK;
}

int bgr_aligner_haplotag_enable(bgr_aligner* a, const uint32_t* table, uint64_t n_rows) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_haplotag_enable: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_haplotag_enable: an internal twin (the table belongs to the aligner it was made for)");
    if (table && n_rows != a->graph->header.n_unitigs + 1) return fail(BGR_E_ARG, "bgr_aligner_haplotag_enable: n_rows is not the graph's number of unitigs + 1");
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));   // (a text piece's kernels may still read the table that is about to go)
    if (!table) { a->tag.table.release(); return BGR_OK; }
    const hipError_t e = a->tag.table.ensure(n_rows * sizeof(uint32_t));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        a->tag.table.release();
        return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string("bgr_aligner_haplotag_enable: ") + std::to_string(n_rows * sizeof(uint32_t)) + " bytes on the device: " + hipGetErrorString(e));
    }
    HIP_TRY(hipMemcpyAsync(a->tag.table.p, table, n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));   // (the caller's table may go once this returns)
    return BGR_OK;
}

int bgr_aligner_haplotags(bgr_aligner* a, uint64_t n_reads, bgr_read_tag* out) {
    if (!a || (n_reads && !out)) return fail(BGR_E_ARG, "bgr_aligner_haplotags: null argument");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_haplotags: an internal twin (ask the aligner it was made for)");
    const uint32_t* table = static_cast<const uint32_t*>(a->tag.table.p);
    if (!table) return fail(BGR_E_ARG, "bgr_aligner_haplotags: no tag table on this aligner (bgr_aligner_haplotag_enable)");
    bgr_aligner* h = holder_of(a);   // (the rows of the last launch, on the stream that ran it; the table is the aligner's own)
    if (n_reads != h->last_n) return fail(BGR_E_ARG, "bgr_aligner_haplotags: n_reads differs from the last bgr_align_device call");
    if (h->last_mode == BGR_MODE_EXHAUSTIVE && !h->sh->exhaustive_paths) return fail(BGR_E_ARG, "bgr_aligner_haplotags: the last launch was exhaustive; rows of the greedy modes only");
    if (n_reads == 0) return BGR_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->tag.out.ensure(n_reads * sizeof(bgr_read_tag)));
    const uint2* rows = nullptr;   // (an exhaustive launch, bgr_aligner_exhaustive_paths_enable: settled, and read through its view)
    if (const int rc = last_rows(h, "bgr_aligner_haplotags", &rows); rc != BGR_OK) return rc;
    const hipError_t e = bgr::launch_haplotags(table, a->graph->header.n_unitigs, rows, static_cast<const int32_t*>(h->launch.arena.p), h->last_arena_cap,
                                               (uint32_t)n_reads, static_cast<bgr_read_tag*>(h->tag.out.p), h->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("haplotags launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out, h->tag.out.p, n_reads * sizeof(bgr_read_tag), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(wait_stream(h));
    return BGR_OK;
}

int bgr_graph_haplotag_enable(bgr_graph* g, const uint32_t* table, uint64_t n_rows) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_haplotag_enable: null graph");
    if (table && n_rows != g->header.n_unitigs + 1) return fail(BGR_E_ARG, "bgr_graph_haplotag_enable: n_rows is not the graph's number of unitigs + 1");
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (!table) { std::vector<uint32_t>().swap(g->haplotag); g->haplotag_on = false; return BGR_OK; }
    try { g->haplotag.assign(table, table + n_rows); } catch (const std::bad_alloc&) { return fail(BGR_E_NOMEM, "bgr_graph_haplotag_enable: no memory for the graph's copy of the table"); }
    g->haplotag_on = true;
    return BGR_OK;
}

int bgr_graph_haplotag_enabled(const bgr_graph* g) { return g && g->haplotag_on ? 1 : 0; }

// ---- what a whole run calls (run_counts.h, registered by capi_abundance.hip) ----------------------------------------------------------------
const uint32_t* run_haplotag_table(const bgr_graph* g, uint64_t* n_rows) {
    *n_rows = 0;
    if (!g || !g->haplotag_on) return nullptr;
    *n_rows = g->haplotag.size();
    return g->haplotag.data();
}
