// capi_blocks.hip -- the C-ABI's haplotype blocks (bgr_block_entry in include/bgreat_gpu.h has the definition; blocks_kernels.h the passes): the
// call on two uploaded lists, the run's entries in the graph object, the writer.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_internal.h"
#include "blocks_kernels.h"

static thread_local double tl_blocks_ms[4] = {0, 0, 0, 0};   // bgr_phase_blocks_times: the calling thread's last call

// The two lists checked on the host, uploaded to `device` on a stream of its own, chained there; the entries' way to the host: into `vec`, or into
// `out` when cap has room.  *n = n_bubbles once the lists have passed the host's checks.  The buffers live for the call: whatever happens, nothing
// stays allocated
static int blocks_call(int device, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_phase* phase, uint64_t n_phase, uint64_t n_unitigs, uint64_t min_phase, const char* who,
                       std::vector<bgr_block_entry>* vec, bgr_block_entry* out, uint64_t cap, uint64_t* n) {
    static_assert(sizeof(bgr_block_entry) == 24, "six 32-bit words");
    const std::string w = who;
    *n = 0;
    for (int i = 0; i < 4; ++i) tl_blocks_ms[i] = 0;
    if (vec) vec->clear();
    if (min_phase == 0) return fail(BGR_E_ARG, w + ": min_phase is at least 1");
    if (n_unitigs >= 0x40000000ull) return fail(BGR_E_ARG, w + ": fewer than 2^30 unitigs");
    if (device < 0) return fail(BGR_E_ARG, w + ": a negative device");
    uint64_t bad = 0;
    if (const int what = bgr::blocks_check(bubbles, n_bubbles, phase, n_phase, n_unitigs, &bad)) {
        static const char* const msg[] = {"", "bubble %s names an id that is 0, beyond 2^30 or beyond n_unitigs", "bubble %s does not name four unitigs with its branches in (|id|, id < 0) order",
                                          "bubble %s is not read canonically ((source, sink) against (-sink, -source))", "the bubbles are not strictly ascending by source (bubble %s)",
                                          "phase record %s names an id that is 0, beyond 2^30 or beyond n_unitigs, or a via that is not positive",
                                          "the phase records are not strictly ascending by via (record %s)", "%s bubbles: a node index and a flag share a 32-bit word"};
        std::string m = msg[what];
        m.replace(m.find("%s"), 2, std::to_string(bad));
        return fail(BGR_E_ARG, w + ": " + m);
    }
    *n = n_bubbles;
    if (n_bubbles == 0) return BGR_OK;   // (no bubble, no block: no device work)
    if (!vec) if (const int rc = rows_refusal(n_bubbles, cap, n, who, "entries"); rc != BGR_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(device));
    DeviceCall r;
    if (const int rc = r.own_stream(); rc != BGR_OK) return rc;
    DevBuf &in_b = r.buf[0], &in_p = r.buf[1], &scratch = r.buf[2], &outbuf = r.buf[3];
    const uint64_t bytes[4] = {n_bubbles * sizeof(bgr_bubble), n_phase * sizeof(bgr_phase), bgr::blocks_scratch_bytes(n_bubbles, n_unitigs), n_bubbles * sizeof(bgr_block_entry)};
    for (int i = 0; i < 4; ++i)
        if (bytes[i] && !r.room(r.buf[i], bytes[i], w + ": " + std::to_string(bytes[i]) + " bytes on the device for " + std::to_string(n_bubbles) + " bubbles, " + std::to_string(n_phase) +
                                                        " phase records and " + std::to_string(n_unitigs) + " unitigs"))
            return r.rc;
    if (const int rc = r.events(4); rc != BGR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(in_b.p, bubbles, bytes[0], hipMemcpyHostToDevice, r.s));
    if (n_phase) HIP_TRY(hipMemcpyAsync(in_p.p, phase, bytes[1], hipMemcpyHostToDevice, r.s));
    const bgr::BlocksScratch sc(scratch.p, n_bubbles, n_unitigs);
    const bgr_bubble* db = static_cast<const bgr_bubble*>(in_b.p);
    HIP_TRY(hipEventRecord(r.ev[0], r.s));
    hipError_t e = bgr::launch_blocks_link(db, n_bubbles, static_cast<const bgr_phase*>(in_p.p), n_phase, n_unitigs, min_phase, scratch.p, r.s);
    if (e != hipSuccess) return fail(BGR_E_HIP, w + ": kernel launch (bgr_blocks_index_kernel, bgr_blocks_link_kernel): " + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(r.ev[1], r.s));
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, sc.err, 4, hipMemcpyDeviceToHost, r.s));   // the error word, before anything is chained
    HIP_TRY(hipStreamSynchronize(r.s));
    if (err) {
        const char* m = err & bgr::kBlocksErrId        ? "a record names a unitig outside 1 .. n_unitigs"
                        : err & bgr::kBlocksErrSource  ? "two bubbles, read both ways, leave one oriented unitig: the list of bubbles is malformed"
                        : err & bgr::kBlocksErrMissing ? "a decided phase record's source or via opens no bubble of the list"
                        : err & bgr::kBlocksErrDiffers ? "a decided phase record's in, out or sink are not those of the bubbles it joins"
                                                       : "two decided phase records leave or enter one bubble";
        return fail(BGR_E_ARG, w + ": " + m + " (error word " + std::to_string(err) + ")");
    }
    if ((e = bgr::launch_blocks_rank(n_bubbles, n_unitigs, scratch.p, r.s)) != hipSuccess) return fail(BGR_E_HIP, w + ": kernel launch (bgr_blocks_rank_*_kernel): " + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(r.ev[2], r.s));
    if ((e = bgr::launch_blocks_count(n_bubbles, n_unitigs, scratch.p, r.s)) != hipSuccess) return fail(BGR_E_HIP, w + ": kernel launch (bgr_blocks_heads_kernel): " + hipGetErrorString(e));
    if ((e = bgr::launch_blocks_place(n_bubbles, n_unitigs, scratch.p, static_cast<bgr_block_entry*>(outbuf.p), r.s)) != hipSuccess)
        return fail(BGR_E_HIP, w + ": kernel launch (bgr_blocks_write_kernel): " + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(r.ev[3], r.s));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, sc.offs_s + bgr::blocks_tiles(n_bubbles), 8, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipMemcpyAsync(&err, sc.err, 4, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipStreamSynchronize(r.s));
    if (total != n_bubbles || err) return fail(BGR_E_INTERNAL, w + ": " + std::to_string(total) + " entries placed for " + std::to_string(n_bubbles) + " bubbles (error word " + std::to_string(err) + ")");
    if (vec) { vec->resize(n_bubbles); out = vec->data(); }
    HIP_TRY(hipMemcpyAsync(out, outbuf.p, bytes[3], hipMemcpyDeviceToHost, r.s));   // (only now: a refused list copies nothing)
    HIP_TRY(hipStreamSynchronize(r.s));
    for (int i = 0; i < 3; ++i) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, r.ev[i], r.ev[i + 1])); tl_blocks_ms[i] = f; }
    tl_blocks_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return BGR_OK;
}

int bgr_phase_blocks(int device, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_phase* phase, uint64_t n_phase, uint64_t n_unitigs, uint64_t min_phase, bgr_block_entry* out,
                     uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!n || (n_bubbles && !bubbles) || (n_phase && !phase) || (cap && !out)) return fail(BGR_E_ARG, "bgr_phase_blocks: null argument");
    return blocks_call(device, bubbles, n_bubbles, phase, n_phase, n_unitigs, min_phase, "bgr_phase_blocks", nullptr, out, cap, n);
}

int bgr_phase_blocks_times(double ms[4]) {
    if (!ms) return fail(BGR_E_ARG, "bgr_phase_blocks_times: null argument");
    for (int i = 0; i < 4; ++i) ms[i] = tl_blocks_ms[i];
    return BGR_OK;
}

// ---- what a whole run calls (run_counts.h, through capi_abundance.hip) ---------------------------------------------------------------------
void run_blocks_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->blocks.forget();
}
int run_blocks_end(bgr_graph* g, bool ok) {   // behind run_phase_end: the run's bubbles and phase records uploaded once to the device the bubbles were called on
    std::lock_guard<std::mutex> l(g->abundance_m);
    return chain_stage_end(g, g->blocks, ok, g->bubbles.valid && g->phase.valid, "blocks without the bubbles and the phase records they are chained from", !g->bubbles.rows.empty(), "bubbles", [&] {
        uint64_t n = 0;
        return blocks_call(g->bubbles.device, g->bubbles.rows.data(), g->bubbles.rows.size(), g->phase.rows.data(), g->phase.rows.size(), g->header.n_unitigs, run_thresholds(g).phase, "bgr_align_all",
                           &g->blocks.rows, nullptr, 0, &n);
    });
}

int bgr_graph_blocks_enable(bgr_graph* g, uint32_t on, uint64_t min_link, uint64_t min_phase) {
    const ChainMins given = {min_link, min_phase, 1};
    if (const int rc = chain_refusal(g, "bgr_graph_blocks_enable", on, given, "the tables of links and triples are sized from it",
                                     "blocks (--blocks) chain phased bubbles, which need a graph of ACGT-only unitigs: on one with other characters a branch read backwards does not spell the reverse complement");
        rc != BGR_OK)
        return rc;
    g->blocks.set(on, given);
    return BGR_OK;
}

int bgr_graph_blocks_enabled(const bgr_graph* g) { return g && g->blocks.on ? 1 : 0; }

int bgr_graph_blocks(const bgr_graph* g, bgr_block_entry* out, uint64_t cap, uint64_t* n) { return graph_rows(g, &bgr_graph::blocks, out, cap, n, "bgr_graph_blocks", "entries", "entries"); }

int bgr_write_blocks(const char* path, const bgr_graph* g, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries, uint64_t n) {
    if (!path || !g || (n_bubbles && !bubbles) || (n && !entries)) return fail(BGR_E_ARG, "bgr_write_blocks: null argument");
    const uint64_t nu = g->header.n_unitigs;
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n_bubbles; ++i)
        for (int32_t x : {bubbles[i].source, bubbles[i].sink, bubbles[i].branch[0], bubbles[i].branch[1]})
            if (!bgr::blocks_id_ok(x, nu)) return fail(BGR_E_ARG, "bgr_write_blocks: bubble " + std::to_string(i) + " names a unitig the graph does not have");
    if (!bgr::blocks_entries_ok(entries, n, n_bubbles, &bad)) return fail(BGR_E_ARG, "bgr_write_blocks: entry " + std::to_string(bad) + " names no bubble of the list, or is none that bgr_phase_blocks makes");
    return write_lines("bgr_write_blocks", path, bgr::blocks_header(), n, [&](uint64_t i, std::string* buf) { bgr::blocks_line(entries[i], bubbles[entries[i].bubble], buf); });
}
