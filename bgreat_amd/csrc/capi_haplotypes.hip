// capi_haplotypes.hip -- the C-ABI's haplotype sequences (bgr_haplotype in include/bgreat_gpu.h has the definition; haplotypes_kernels.h the passes):
// the call on two uploaded lists over the resident graph, the run's records and bytes in the graph object, the writer.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_internal.h"
#include "haplotypes_kernels.h"

static thread_local double tl_hap_ms[4] = {0, 0, 0, 0};   // bgr_blocks_haplotypes_times: the calling thread's last call

// The two lists checked on the host, uploaded to `device` on a stream of its own, spelled there from the graph's blob; the records' and bytes' way to
// the host: into the vectors, or into `out` and `seq` when both capacities have room.  *n, *seq_bytes and *bad_junctions are set once the first two
// passes have run.  The buffers live for the call: whatever happens, nothing stays allocated
static int haplotypes_call(const bgr_graph* g, int device, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries, uint64_t n_entries, uint64_t min_block, const char* who,
                           std::vector<bgr_haplotype>* vec, std::vector<char>* vseq, bgr_haplotype* out, uint64_t cap, uint64_t* n, char* seq, uint64_t seq_cap, uint64_t* seq_bytes,
                           uint64_t* bad_junctions) {
    static_assert(sizeof(bgr_haplotype) == 32, "four 32-bit words and two 64-bit ones");
    const std::string w = who;
    *n = *seq_bytes = *bad_junctions = 0;
    for (int i = 0; i < 4; ++i) tl_hap_ms[i] = 0;
    if (vec) { vec->clear(); vseq->clear(); }
    if (min_block == 0) return fail(BGR_E_ARG, w + ": min_block is at least 1");
    if (device < 0) return fail(BGR_E_ARG, w + ": a negative device");
    const auto it = g->dev.find(device);
    if (it == g->dev.end() || !it->second.ptr) return fail(BGR_E_ARG, w + ": the graph is not resident on device " + std::to_string(device) + " (bgr_graph_upload, bgr_devices_init)");
    if (g->header.has_exc)
        return fail(BGR_E_ARG, w + ": the haplotypes (--haplotypes) are spelled from the 2-bit store, which needs a graph of ACGT-only unitigs: on one with other characters it does not hold the unitigs' characters");
    const uint64_t nu = g->header.n_unitigs;
    if (nu >= 0x40000000ull) return fail(BGR_E_ARG, w + ": fewer than 2^30 unitigs");
    uint64_t bad = 0;
    if (const int what = bgr::haplotypes_check(bubbles, n_bubbles, entries, n_entries, nu, &bad)) {
        static const char* const msg[] = {"", "bubble %s names an id that is 0, beyond 2^30 or beyond the graph's unitigs", "entry %s names no bubble of the list, or is none that bgr_phase_blocks makes",
                                          "the entries do not come block after block in chain order (entry %s)",
                                          "entry %s does not begin where the entry before it ends (its source is not that one's sink): no decided link joins the two", "%s entries: 2^30 - 1 at the most"};
        std::string m = msg[what];
        m.replace(m.find("%s"), 2, std::to_string(bad));
        return fail(BGR_E_ARG, w + ": " + m);
    }
    if (n_entries == 0) return BGR_OK;   // (no entry, no sequence: no device work)
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(device));
    BgrDeviceGraph dg;
    bgr::resolve_device_graph(&g->header, it->second.ptr, dg);
    DeviceCall r;   // r.ev: around items + scan; before the spell launch (behind the allocations), behind it, behind the records
    if (const int rc = r.own_stream(); rc != BGR_OK) return rc;
    DevBuf &in_b = r.buf[0], &in_e = r.buf[1], &scratch = r.buf[2], &recs = r.buf[3], &bytes = r.buf[4];
    auto room = [&](DevBuf& b, uint64_t want) {   // -> whether the device has `want` more bytes
        return r.room(b, want, w + ": " + std::to_string(want) + " bytes on the device for " + std::to_string(n_bubbles) + " bubbles and " + std::to_string(n_entries) + " entries");
    };
    const uint64_t in_bytes[2] = {n_bubbles * sizeof(bgr_bubble), n_entries * sizeof(bgr_block_entry)};
    if (!room(in_b, in_bytes[0]) || !room(in_e, in_bytes[1]) || !room(scratch, bgr::hap_scratch_bytes(n_entries))) return r.rc;
    if (const int rc = r.events(5); rc != BGR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(in_b.p, bubbles, in_bytes[0], hipMemcpyHostToDevice, r.s));
    HIP_TRY(hipMemcpyAsync(in_e.p, entries, in_bytes[1], hipMemcpyHostToDevice, r.s));
    const bgr::HapScratch sc(scratch.p, n_entries);
    const bgr_bubble* db = static_cast<const bgr_bubble*>(in_b.p);
    const bgr_block_entry* de = static_cast<const bgr_block_entry*>(in_e.p);
    HIP_TRY(hipEventRecord(r.ev[0], r.s));
    hipError_t e = bgr::launch_hap_items(dg, nu, g->header.total_bases, db, n_bubbles, de, n_entries, min_block, scratch.p, r.s);
    if (e != hipSuccess) return fail(BGR_E_HIP, w + ": kernel launch (bgr_hap_items_kernel, bgr_hap_tiles_kernel, bgr_hap_tile_scan_kernel): " + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(r.ev[1], r.s));
    uint64_t total = 0, blocks = 0, words[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&total, sc.ioff + 2 * n_entries, 8, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipMemcpyAsync(&blocks, sc.iord + 2 * n_entries, 8, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipMemcpyAsync(words, sc.words, 16, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipStreamSynchronize(r.s));
    if (const uint32_t err = (uint32_t)words[1]) {
        const char* m = err & bgr::kHapErrId ? "an entry's bubble names a unitig outside the graph" : err & bgr::kHapErrEntry ? "an entry lies outside its block or names no bubble of the list"
                                                                                                                                : "a unitig does not lie inside the graph's sequence store";
        return fail(err & bgr::kHapErrSeq ? BGR_E_INTERNAL : BGR_E_ARG, w + ": " + m + " (error word " + std::to_string(err) + ")");
    }
    *n = 2 * blocks;
    *seq_bytes = total;
    *bad_junctions = words[0];
    { float f = 0; HIP_TRY(hipEventElapsedTime(&f, r.ev[0], r.ev[1])); tl_hap_ms[0] = f; }
    if (!vec && (2 * blocks > cap || total > seq_cap)) {
        tl_hap_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return fail(BGR_E_CAPACITY, w + ": " + std::to_string(2 * blocks) + " sequences of " + std::to_string(total) + " bytes, room for " + std::to_string(cap) + " and " + std::to_string(seq_cap));
    }
    if (blocks) {   // (every kept block has two sequences of at least k characters)
        if (!room(recs, 2 * blocks * sizeof(bgr_haplotype)) || !room(bytes, total)) return r.rc;
        HIP_TRY(hipEventRecord(r.ev[2], r.s));   // (only here: the sizing copies, the wait and the two allocations above are no part of the spell stage)
        if ((e = bgr::launch_hap_spell(dg, n_entries, total, scratch.p, static_cast<char*>(bytes.p), r.s)) != hipSuccess)
            return fail(BGR_E_HIP, w + ": kernel launch (bgr_hap_spell_kernel): " + hipGetErrorString(e));
        HIP_TRY(hipEventRecord(r.ev[3], r.s));
        if ((e = bgr::launch_hap_records(de, n_entries, min_block, scratch.p, static_cast<bgr_haplotype*>(recs.p), 2 * blocks, r.s)) != hipSuccess)
            return fail(BGR_E_HIP, w + ": kernel launch (bgr_hap_records_kernel): " + hipGetErrorString(e));
        HIP_TRY(hipEventRecord(r.ev[4], r.s));
        HIP_TRY(hipMemcpyAsync(words, sc.words, 16, hipMemcpyDeviceToHost, r.s));
        HIP_TRY(hipStreamSynchronize(r.s));
        if ((uint32_t)words[1]) return fail(BGR_E_INTERNAL, w + ": a record beyond the " + std::to_string(2 * blocks) + " the scan counted (error word " + std::to_string((uint32_t)words[1]) + ")");
        if (vec) { vec->resize(2 * blocks); vseq->resize(total); out = vec->data(); seq = vseq->data(); }
        HIP_TRY(hipMemcpyAsync(out, recs.p, 2 * blocks * sizeof(bgr_haplotype), hipMemcpyDeviceToHost, r.s));   // (only now: a refused call copies nothing)
        HIP_TRY(hipMemcpyAsync(seq, bytes.p, total, hipMemcpyDeviceToHost, r.s));
        HIP_TRY(hipStreamSynchronize(r.s));
        for (int i = 1; i < 3; ++i) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, r.ev[i + 1], r.ev[i + 2])); tl_hap_ms[i] = f; }
    }
    tl_hap_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return BGR_OK;
}

int bgr_blocks_haplotypes(const bgr_graph* g, int device, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries, uint64_t n_entries, uint64_t min_block,
                          bgr_haplotype* out, uint64_t cap, uint64_t* n, char* seq, uint64_t seq_cap, uint64_t* seq_bytes, uint64_t* bad_junctions) {
    if (n) *n = 0;
    if (seq_bytes) *seq_bytes = 0;
    if (bad_junctions) *bad_junctions = 0;
    if (!g || !n || !seq_bytes || !bad_junctions || (n_bubbles && !bubbles) || (n_entries && !entries) || (cap && !out) || (seq_cap && !seq)) return fail(BGR_E_ARG, "bgr_blocks_haplotypes: null argument");
    return haplotypes_call(g, device, bubbles, n_bubbles, entries, n_entries, min_block, "bgr_blocks_haplotypes", nullptr, nullptr, out, cap, n, seq, seq_cap, seq_bytes, bad_junctions);
}

int bgr_blocks_haplotypes_times(double ms[4]) {
    if (!ms) return fail(BGR_E_ARG, "bgr_blocks_haplotypes_times: null argument");
    for (int i = 0; i < 4; ++i) ms[i] = tl_hap_ms[i];
    return BGR_OK;
}

// ---- what a whole run calls (run_counts.h, through capi_abundance.hip) ---------------------------------------------------------------------
void run_haplotypes_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->haplotypes.forget();
}
int run_haplotypes_end(bgr_graph* g, bool ok) {   // behind run_blocks_end: the run's bubbles and entries uploaded once to the device the bubbles were called on
    std::lock_guard<std::mutex> l(g->abundance_m);
    return chain_stage_end(g, g->haplotypes, ok, g->bubbles.valid && g->blocks.valid, "haplotypes without the bubbles and the block entries they are spelled from", !g->blocks.rows.empty(),
                           "block entries", [&] {
        uint64_t n = 0, bytes = 0, bad = 0;
        const int rc = haplotypes_call(g, g->bubbles.device, g->bubbles.rows.data(), g->bubbles.rows.size(), g->blocks.rows.data(), g->blocks.rows.size(), run_thresholds(g).block, "bgr_align_all",
                                       &g->haplotypes.rows, &g->haplotypes.seq, nullptr, 0, &n, nullptr, 0, &bytes, &bad);
        if (rc != BGR_OK || !bad) return rc;
        return fail(BGR_E_INTERNAL, "bgr_align_all: " + std::to_string(bad) + " junctions of the run's haplotype walks do not overlap in k - 1 characters: the bubbles' links are none of this graph");
    });
}

int bgr_graph_haplotypes_enable(bgr_graph* g, uint32_t on, uint64_t min_link, uint64_t min_phase, uint64_t min_block) {
    const ChainMins given = {min_link, min_phase, min_block};
    if (const int rc = chain_refusal(g, "bgr_graph_haplotypes_enable", on, given, "the tables of links and triples are sized from it",
                                     "the haplotypes (--haplotypes) are spelled from the 2-bit store along phased bubbles, which needs a graph of ACGT-only unitigs");
        rc != BGR_OK)
        return rc;
    g->haplotypes.set(on, given);
    return BGR_OK;
}

int bgr_graph_haplotypes_enabled(const bgr_graph* g) { return g && g->haplotypes.on ? 1 : 0; }

// (two vectors with one refusal for both: the one getter that is not graph_rows)
int bgr_graph_haplotypes(const bgr_graph* g, bgr_haplotype* out, uint64_t cap, uint64_t* n, char* seq, uint64_t seq_cap, uint64_t* seq_bytes) {
    if (n) *n = 0;
    if (seq_bytes) *seq_bytes = 0;
    if (!g || !n || !seq_bytes || (cap && !out) || (seq_cap && !seq)) return fail(BGR_E_ARG, "bgr_graph_haplotypes: null argument");
    const bgr_graph::Haplotypes& h = g->haplotypes;
    if (!h.valid) return fail(BGR_E_ARG, "bgr_graph_haplotypes: no sequences -- they are those of the last successful bgr_align_all with bgr_graph_haplotypes_enable on");
    *n = h.rows.size();
    *seq_bytes = h.seq.size();
    if (h.rows.size() > cap || h.seq.size() > seq_cap)
        return fail(BGR_E_CAPACITY, "bgr_graph_haplotypes: " + std::to_string(h.rows.size()) + " sequences of " + std::to_string(h.seq.size()) + " bytes, room for " + std::to_string(cap) + " and " +
                                        std::to_string(seq_cap));
    if (!h.rows.empty()) memcpy(out, h.rows.data(), h.rows.size() * sizeof(bgr_haplotype));
    if (!h.seq.empty()) memcpy(seq, h.seq.data(), h.seq.size());
    return BGR_OK;
}

int bgr_write_haplotypes(const char* path, const bgr_graph* g, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries, uint64_t n_entries, const bgr_haplotype* haps,
                         uint64_t n, const char* seq, uint64_t seq_bytes) {
    if (!path || !g || (n_bubbles && !bubbles) || (n_entries && !entries) || (n && !haps) || (seq_bytes && !seq)) return fail(BGR_E_ARG, "bgr_write_haplotypes: null argument");
    uint64_t bad = 0;
    if (const int what = bgr::haplotypes_check(bubbles, n_bubbles, entries, n_entries, g->header.n_unitigs, &bad))
        return fail(BGR_E_ARG, "bgr_write_haplotypes: the bubbles and entries are none that bgr_blocks_haplotypes takes (check " + std::to_string(what) + ", record " + std::to_string(bad) + ")");
    std::vector<uint64_t> first(n);
    if (!bgr::hap_records_ok(haps, n, entries, n_entries, seq_bytes, first.data(), &bad))
        return fail(BGR_E_ARG, "bgr_write_haplotypes: record " + std::to_string(bad) + " is not one of the entries' blocks, or the sequences do not lie back to back in " + std::to_string(seq_bytes) + " bytes");
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string("bgr_write_haplotypes: cannot open ") + path);
    std::string buf;
    bool ok = true;
    for (uint64_t i = 0; i < n && ok; ++i) {
        bgr::hap_header(haps[i], entries + first[i], bubbles, &buf);
        ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
        buf.clear();
        if (ok && haps[i].length) ok = fwrite(seq + haps[i].offset, 1, haps[i].length, f) == haps[i].length;
        if (ok) ok = fputc('\n', f) != EOF;
    }
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string("bgr_write_haplotypes: write to ") + path + " failed");
    return BGR_OK;
}
