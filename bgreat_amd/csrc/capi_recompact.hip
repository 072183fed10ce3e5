// capi_recompact.hip -- the C-ABI's re-compaction (bgr_chain in include/bgreat_gpu.h has the definition; recompact_kernels.h the passes): the call on
// keep bytes over the resident graph, the run's chains in the graph object, the writer.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_internal.h"
#include "recompact_host.h"
#include "recompact_kernels.h"

static thread_local double tl_recompact_ms[5] = {0, 0, 0, 0, 0};   // bgr_graph_recompact_times: the calling thread's last call

// The keep bytes uploaded to `device` on a stream of its own into the call's one scratch allocation, compacted there from the graph's blob; the result's
// way to the host: into the vectors, or into the caller's buffers when all three capacities have room.  *n, *walk_n and *seq_bytes are set once the
// sizing passes have run.  The buffers live for the call: whatever happens, nothing stays allocated
static int recompact_call(const bgr_graph* g, int device, const uint8_t* keep, uint64_t n_keep, const char* who, std::vector<bgr_chain>* vec, std::vector<int32_t>* vwalk, std::vector<char>* vseq,
                          bgr_chain* out, uint64_t cap, uint64_t* n, int32_t* walk, uint64_t walk_cap, uint64_t* walk_n, char* seq, uint64_t seq_cap, uint64_t* seq_bytes) {
    static_assert(sizeof(bgr_chain) == 32, "three 64-bit words and two 32-bit ones");
    const std::string w = who;
    *n = *walk_n = *seq_bytes = 0;
    for (double& m : tl_recompact_ms) m = 0;
    if (vec) { vec->clear(); vwalk->clear(); vseq->clear(); }
    if (device < 0) return fail(BGR_E_ARG, w + ": a negative device");
    const auto it = g->dev.find(device);
    if (it == g->dev.end() || !it->second.ptr) return fail(BGR_E_ARG, w + ": the graph is not resident on device " + std::to_string(device) + " (bgr_graph_upload, bgr_devices_init)");
    if (g->header.has_exc)
        return fail(BGR_E_ARG, w + ": the chains (--recompact) are spelled from the 2-bit store, which needs a graph of ACGT-only unitigs: on one with other characters it does not hold the unitigs' characters");
    const uint64_t nu = g->header.n_unitigs, nk = g->header.n_keys;
    if (n_keep != nu) return fail(BGR_E_ARG, w + ": n_keep is not the graph's number of unitigs");
    if (nu >= 0x40000000ull || nk >= 0x7FFFFFFFull) return fail(BGR_E_ARG, w + ": fewer than 2^30 unitigs and 2^31 - 1 key indices");
    if (nu == 0) return BGR_OK;   // (no unitig, no chain: no device work)
    HIP_TRY(hipSetDevice(device));
    BgrDeviceGraph dg;
    bgr::resolve_device_graph(&g->header, it->second.ptr, dg);
    DeviceCall r;
    if (const int rc = r.own_stream(); rc != BGR_OK) return rc;
    DevBuf &scratch = r.buf[0], &recs = r.buf[1], &bytes = r.buf[2];
    auto room = [&](DevBuf& b, uint64_t want) {   // -> whether the device has `want` more bytes
        return r.room(b, want, w + ": " + std::to_string(want) + " bytes on the device for " + std::to_string(nu) + " unitigs and " + std::to_string(nk) + " key indices");
    };
    if (!room(scratch, bgr::recompact_scratch_bytes(nu, nk))) return r.rc;
    if (const int rc = r.events(5); rc != BGR_OK) return rc;
    const bgr::RecompactScratch sc(scratch.p, nu, nk);
    HIP_TRY(hipMemcpyAsync(sc.keep, keep, nu, hipMemcpyHostToDevice, r.s));
    HIP_TRY(hipEventRecord(r.ev[0], r.s));
    hipError_t e = bgr::launch_recompact_links(dg, nu, nk, scratch.p, r.s);
    if (e != hipSuccess) return fail(BGR_E_HIP, w + ": kernel launch (bgr_recompact_ends_kernel, bgr_recompact_succ_kernel): " + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(r.ev[1], r.s));
    if ((e = bgr::launch_recompact_rank(nu, nk, scratch.p, r.s)) != hipSuccess) return fail(BGR_E_HIP, w + ": kernel launch (bgr_recompact_rank_*_kernel, bgr_recompact_open_kernel): " + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(r.ev[2], r.s));
    if ((e = bgr::launch_recompact_place(dg, nu, nk, g->header.total_bases, scratch.p, r.s)) != hipSuccess)
        return fail(BGR_E_HIP, w + ": kernel launch (bgr_recompact_tail_kernel ... bgr_recompact_place_kernel): " + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(r.ev[3], r.s));
    uint64_t chains = 0, ints = 0, total = 0, words[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&chains, sc.hord + 2 * nu, 8, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipMemcpyAsync(&ints, sc.hoff + 2 * nu, 8, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipMemcpyAsync(&total, sc.ioff + nu, 8, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipMemcpyAsync(words, sc.words, 16, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipStreamSynchronize(r.s));
    if (const uint32_t err = (uint32_t)words[1]) {
        const char* m = err & bgr::kRecompactErrKey ? "a unitig's end names a key index beyond the graph's" : err & bgr::kRecompactErrId ? "the table of ends names a unitig outside the graph"
                        : err & bgr::kRecompactErrSeq ? "a unitig does not lie inside the graph's sequence store" : err & bgr::kRecompactErrLen ? "a unitig is shorter than k" : "a place beyond the walk";
        return fail(BGR_E_INTERNAL, w + ": " + m + " (error word " + std::to_string(err) + ")");
    }
    if (ints > nu || chains > ints) return fail(BGR_E_INTERNAL, w + ": " + std::to_string(chains) + " chains of " + std::to_string(ints) + " unitigs out of " + std::to_string(nu));
    *n = chains;
    *walk_n = ints;
    *seq_bytes = total;
    for (int i = 0; i < 3; ++i) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, r.ev[i], r.ev[i + 1])); tl_recompact_ms[i] = f; }
    if (!vec && (chains > cap || ints > walk_cap || total > seq_cap))
        return fail(BGR_E_CAPACITY, w + ": " + std::to_string(chains) + " chains of " + std::to_string(ints) + " unitigs and " + std::to_string(total) + " bytes, room for " + std::to_string(cap) + ", " +
                                        std::to_string(walk_cap) + " and " + std::to_string(seq_cap));
    if (chains) {   // (every chain has a unitig of at least k characters)
        if (!room(recs, chains * sizeof(bgr_chain)) || !room(bytes, total)) return r.rc;
        HIP_TRY(hipEventRecord(r.ev[0], r.s));   // (only here: the sizing copies, the wait and the two allocations above are no part of the spell stage)
        if ((e = bgr::launch_recompact_spell(dg, nu, nk, ints, total, scratch.p, static_cast<char*>(bytes.p), r.s)) != hipSuccess)
            return fail(BGR_E_HIP, w + ": kernel launch (bgr_recompact_spell_kernel): " + hipGetErrorString(e));
        HIP_TRY(hipEventRecord(r.ev[1], r.s));
        if ((e = bgr::launch_recompact_records(nu, nk, scratch.p, static_cast<bgr_chain*>(recs.p), chains, r.s)) != hipSuccess)
            return fail(BGR_E_HIP, w + ": kernel launch (bgr_recompact_records_kernel): " + hipGetErrorString(e));
        HIP_TRY(hipEventRecord(r.ev[2], r.s));
        HIP_TRY(hipMemcpyAsync(words, sc.words, 16, hipMemcpyDeviceToHost, r.s));
        HIP_TRY(hipStreamSynchronize(r.s));
        if ((uint32_t)words[1]) return fail(BGR_E_INTERNAL, w + ": a record beyond the " + std::to_string(chains) + " the scan counted (error word " + std::to_string((uint32_t)words[1]) + ")");
        if (vec) { vec->resize(chains); vwalk->resize(ints); vseq->resize(total); out = vec->data(); walk = vwalk->data(); seq = vseq->data(); }
        HIP_TRY(hipMemcpyAsync(out, recs.p, chains * sizeof(bgr_chain), hipMemcpyDeviceToHost, r.s));   // (only now: a refused call copies nothing)
        HIP_TRY(hipMemcpyAsync(walk, sc.walk, ints * sizeof(int32_t), hipMemcpyDeviceToHost, r.s));
        HIP_TRY(hipMemcpyAsync(seq, bytes.p, total, hipMemcpyDeviceToHost, r.s));
        HIP_TRY(hipStreamSynchronize(r.s));
        for (int i = 0; i < 2; ++i) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, r.ev[i], r.ev[i + 1])); tl_recompact_ms[3 + i] = f; }
    }
    return BGR_OK;
}

int bgr_graph_recompact(const bgr_graph* g, int device, const uint8_t* keep, uint64_t n_keep, bgr_chain* out, uint64_t cap, uint64_t* n, int32_t* walk, uint64_t walk_cap, uint64_t* walk_n,
                        char* seq, uint64_t seq_cap, uint64_t* seq_bytes) {
    if (n) *n = 0;
    if (walk_n) *walk_n = 0;
    if (seq_bytes) *seq_bytes = 0;
    if (!g || !n || !walk_n || !seq_bytes || (n_keep && !keep) || (cap && !out) || (walk_cap && !walk) || (seq_cap && !seq)) return fail(BGR_E_ARG, "bgr_graph_recompact: null argument");
    return recompact_call(g, device, keep, n_keep, "bgr_graph_recompact", nullptr, nullptr, nullptr, out, cap, n, walk, walk_cap, walk_n, seq, seq_cap, seq_bytes);
}

int bgr_graph_recompact_times(double ms[5]) {
    if (!ms) return fail(BGR_E_ARG, "bgr_graph_recompact_times: null argument");
    for (int i = 0; i < 5; ++i) ms[i] = tl_recompact_ms[i];
    return BGR_OK;
}

// ---- what a whole run calls (run_counts.h, through capi_abundance.hip) ---------------------------------------------------------------------
void run_recompact_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->recompact.forget();
    g->recompact.device = -1;
}
int run_recompact_collect(bgr_graph* g, bgr_aligner* a) {   // nothing of an aligner's joins the run's: the first one's device is where the run's chains will be made
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (g->recompact.device < 0) g->recompact.device = a->device;
    return BGR_OK;
}
int run_recompact_end(bgr_graph* g, bool ok) {   // behind the abundance's end: the keep bytes from the run's summed reads column, uploaded once
    std::lock_guard<std::mutex> l(g->abundance_m);
    bgr_graph::Recompact& rc = g->recompact;
    rc.forget();
    if (!ok) return BGR_OK;
    const uint64_t nu = g->header.n_unitigs;
    int rv = BGR_OK;
    if (!g->abundance_valid || g->abundance.size() != nu) rv = fail(BGR_E_INTERNAL, "bgr_align_all: the re-compaction without the run's abundance totals it keeps unitigs by");
    else if (nu && rc.device < 0) rv = fail(BGR_E_INTERNAL, "bgr_align_all: unitigs to re-compact, but no aligner of the run was collected");
    else if (nu) {
        std::vector<uint8_t> keep(nu);
        bgr::recompact_keep(g->abundance.data(), nu, rc.min_reads, keep.data());
        uint64_t n = 0, wn = 0, sb = 0;
        rv = recompact_call(g, rc.device, keep.data(), nu, "bgr_align_all", &rc.rows, &rc.walk, &rc.seq, nullptr, 0, &n, nullptr, 0, &wn, nullptr, 0, &sb);
    }
    if (rv != BGR_OK) rc.forget();
    rc.valid = rv == BGR_OK;
    return rv;
}

int bgr_graph_recompact_enable(bgr_graph* g, uint32_t on, uint64_t min_reads) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_recompact_enable: null graph");
    if (on && g->header.has_exc)
        return fail(BGR_E_ARG, "bgr_graph_recompact_enable: the chains (--recompact) are spelled from the 2-bit store, which needs a graph of ACGT-only unitigs");
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (on) g->recompact.min_reads = min_reads;
    g->recompact.on = on != 0;
    return BGR_OK;
}

int bgr_graph_recompact_enabled(const bgr_graph* g) { return g && g->recompact.on ? 1 : 0; }

int bgr_graph_recompact_result(const bgr_graph* g, bgr_chain* out, uint64_t cap, uint64_t* n, int32_t* walk, uint64_t walk_cap, uint64_t* walk_n, char* seq, uint64_t seq_cap,
                               uint64_t* seq_bytes) {
    if (n) *n = 0;
    if (walk_n) *walk_n = 0;
    if (seq_bytes) *seq_bytes = 0;
    if (!g || !n || !walk_n || !seq_bytes || (cap && !out) || (walk_cap && !walk) || (seq_cap && !seq)) return fail(BGR_E_ARG, "bgr_graph_recompact_result: null argument");
    const bgr_graph::Recompact& r = g->recompact;
    if (!r.valid) return fail(BGR_E_ARG, "bgr_graph_recompact_result: no chains -- they are those of the last successful bgr_align_all with bgr_graph_recompact_enable on");
    *n = r.rows.size();
    *walk_n = r.walk.size();
    *seq_bytes = r.seq.size();
    if (r.rows.size() > cap || r.walk.size() > walk_cap || r.seq.size() > seq_cap)
        return fail(BGR_E_CAPACITY, "bgr_graph_recompact_result: " + std::to_string(r.rows.size()) + " chains of " + std::to_string(r.walk.size()) + " unitigs and " + std::to_string(r.seq.size()) +
                                        " bytes, room for " + std::to_string(cap) + ", " + std::to_string(walk_cap) + " and " + std::to_string(seq_cap));
    if (!r.rows.empty()) memcpy(out, r.rows.data(), r.rows.size() * sizeof(bgr_chain));
    if (!r.walk.empty()) memcpy(walk, r.walk.data(), r.walk.size() * sizeof(int32_t));
    if (!r.seq.empty()) memcpy(seq, r.seq.data(), r.seq.size());
    return BGR_OK;
}

int bgr_write_recompact(const char* path, const bgr_graph* g, const bgr_chain* chains, uint64_t n, const int32_t* walk, uint64_t walk_n, const char* seq, uint64_t seq_bytes) {
    if (!path || !g || (n && !chains) || (walk_n && !walk) || (seq_bytes && !seq)) return fail(BGR_E_ARG, "bgr_write_recompact: null argument");
    uint64_t bad = 0;
    if (!bgr::recompact_records_ok(chains, n, walk, walk_n, seq_bytes, g->header.n_unitigs, g->header.k, &bad))
        return fail(BGR_E_ARG, "bgr_write_recompact: record " + std::to_string(bad) + " does not lie back to back with the one before it in " + std::to_string(walk_n) + " walk ids and " +
                                   std::to_string(seq_bytes) + " bytes, is shorter than k, or names a unitig outside the graph");
    return write_lines("bgr_write_recompact", path, "", n, [&](uint64_t i, std::string* buf) {
        bgr::recompact_header(i + 1, chains[i], walk + chains[i].walk_off, buf);
        buf->append(seq + chains[i].seq_off, chains[i].seq_len);
        *buf += '\n';
    });
}
