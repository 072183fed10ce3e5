// capi.hip -- implementation of the C-ABI declared in include/bgreat_gpu.h.  Thin: argument checks, HIP memory
// and stream management, launch geometry; the algorithm lives in graph_build.cpp (index) and
// the *_kernels.hip files (mapping; launch interface align_kernels.h).  There is no CPU mapping path in this library.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bgreat_gpu.h"
#include "abundance_kernels.h"
#include "align_kernels.h"
#include "fanout.h"
#include "fastx.h"
#include "anchor_index.h"
#include "graph_build.h"
#include "launch_plan.h"
#include "links_kernels.h"
#include "pileup_kernels.h"
#include "read_pack.h"
#include "run_abundance.h"
#include "run_links.h"
#include "run_pileup.h"
#include "text_kernels.h"
#include "variants_kernels.h"
#include "options.h"

namespace {

thread_local std::string tl_err;
int fail(int code, const std::string& msg) { tl_err = msg; return code; }
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(BGR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

const int kTimerRing = 64;   // launches between two drains of the timers
const int kTimerSlots = 8;   // kernels of one launch timed separately (pre-pass, passes)

}  // namespace

namespace bgr {
int set_error(int code, const std::string& msg) { return fail(code, msg); }  // for pipeline.cpp
}

struct bgr_graph {
    bgr::HostGraph host;  // empty when adopted from a device blob
    std::vector<char> ascii;            // the unitig characters as given (only graphs built from sequences have them):
    std::vector<uint64_t> ascii_offs;   // correction mode spells reads from these, like the reference's vector<string>
    BgrBlobHeader header;
    struct Dev { void* ptr; bool owned; };
    std::map<int, Dev> dev;
    uint32_t fanout_method = 0;  // how bgr_devices_init moved the blob between devices last time
    // per-unitig totals of the last bgr_align_all with bgr_run_options.abundance (row i = unitig id i + 1); the run's aligners add theirs as they finish
    std::vector<bgr_unitig_abundance> abundance;
    bool abundance_valid = false;
    std::mutex abundance_m;   // (the lanes of a split run end side by side)
    // links (bgr_graph_links_enable): the sticky switch, the bound of distinct links (computed from the host blob the first time it is asked for),
    // and the totals of the last bgr_align_all with the switch on: {key, count} as the aligners delivered them until the run ends, then merged and sorted
    bool links_on = false, links_valid = false, links_bound_known = false;
    uint64_t links_bound = 0;
    std::vector<std::pair<uint64_t, uint64_t>> links;
    // pileup (bgr_graph_pileup_enable): the sticky switch, where every unitig's bases start in a table (prefix sums of the lengths, from the host blob
    // the first time they are asked for), and the totals of the last bgr_align_all with the switch on: the aligners' tables summed mod 2^32
    bool pileup_on = false, pileup_valid = false;
    std::vector<uint64_t> base_offs;          // [n_unitigs + 2]: base_offs[id] = sum of len of the unitigs 1 .. id - 1
    std::vector<uint32_t> pileup_words;       // alt[4 T] then delta[T + n] (pileup_kernels.h)
    uint64_t pileup_skipped = 0;
    // SNV sites (bgr_graph_variants_enable): the sticky switch and its thresholds; while a run collects its aligners, the run's pileup table on a device
    // (the first aligner's, adopted; the others' added into it); then the sites of the last successful run and the thresholds they were called with
    bool variants_on = false, variants_valid = false;
    bgr_variant_params variants_prm = {2, 2, 200000}, variants_called = {0, 0, 0};
    struct VariantsRun* variants_run = nullptr;
    std::vector<bgr_variant_site> variants_sites;
    // strands (bgr_graph_pileup_strands_enable, bgr_graph_variants_strands_enable): the run's aligners also count the forward table; with the pileup
    // switch its totals are gathered next to pileup_words, with the variants switch it travels with the run's table and the records are 64 bytes
    bool pileup_strands_on = false, pileup_fwd_valid = false, variants_strands_on = false, variants_strands_valid = false;
    uint32_t variants_min_alt_strand = 0, variants_called_strand = 0;
    std::vector<uint32_t> pileup_fwd_words;
    std::vector<bgr_variant_strand_site> variants_strand_sites;
};

namespace {  // for pipeline.cpp (run_abundance.h): the totals of a run with bgr_run_options.abundance
void graph_abundance_begin(bgr_graph* g) {  // a new run: the totals of the one before are gone, whatever becomes of this one
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->abundance.assign(g->header.n_unitigs, bgr_unitig_abundance{0, 0, 0});
    g->abundance_valid = false;
}
void graph_abundance_add(bgr_graph* g, const bgr_unitig_abundance* rows, uint64_t n) {  // one aligner's table
    std::lock_guard<std::mutex> l(g->abundance_m);
    for (uint64_t i = 0; i < n && i < g->abundance.size(); ++i) { g->abundance[i].reads += rows[i].reads; g->abundance[i].bases += rows[i].bases; g->abundance[i].kmers += rows[i].kmers; }
}
void graph_abundance_end(bgr_graph* g, bool ok) {  // totals only of a run that ended well
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (!ok) g->abundance.clear();
    g->abundance_valid = ok;
}
}  // namespace

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        // diagnostic (bgr_set_option("poison_device_buffers", 1); tools/fuzz_*.py, the GPU suite): fresh device memory usually reads as zeroes, recycled memory of
        // a long-lived process does not -- fill every new buffer with a pattern so that a kernel that reads what nothing has written shows in ANY run
        const bool poison = bgr::opt("poison_device_buffers") != 0;
        if (e == hipSuccess && poison) { e = hipMemset(p, 0xA5, want); if (e == hipSuccess) e = hipDeviceSynchronize(); }  // (the fill runs on the null stream: the aligner's streams do not wait for it)
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct VariantsRun {   // the pileup table of a run with bgr_graph_variants_enable while its aligners are collected (bgr_graph has the rest)
    int device = 0, num_cus = 0;
    hipStream_t stream = nullptr;
    BgrDeviceGraph dg;
    DevBuf table, offs, stage, table_fwd;   // (table_fwd: only in a run that counts strands)
};
static void variants_run_free(bgr_graph* g) {
    if (!g->variants_run) return;
    if (hipSetDevice(g->variants_run->device) == hipSuccess) {
        if (g->variants_run->stream) (void)hipStreamDestroy(g->variants_run->stream);
        g->variants_run->table.release(); g->variants_run->offs.release(); g->variants_run->stage.release(); g->variants_run->table_fwd.release();
    }
    delete g->variants_run;
    g->variants_run = nullptr;
}

struct bgr_text_stage {  // one piece of text on its way to / resident in a device: buffer, copy stream, "it has arrived" event
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev = nullptr, ev0 = nullptr;  // ev0: BGREAT_TIMING only, start of the copy
    DevBuf buf;
    uint64_t bytes = 0;
    bool timing = false, pending = false;
    double copy_ms = 0, copy_bytes = 0;
    void settle() {  // BGREAT_TIMING: duration of the last copy (it has completed)
        if (!timing || !pending) return;
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev0, ev) == hipSuccess) { copy_ms += ms; copy_bytes += (double)bytes; }
        pending = false;
    }
};

struct bgr_aligner {
    bgr_graph* graph = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    BgrDeviceGraph dg;
    // the text route (bgr_align_fasta_text): the piece, its records, the formatted streams
    DevBuf tx_in, tx_sums, tx_state, tx_rec, tx_idx, tx_accrec, tx_accsrc, tx_offs, tx_psz, tx_nsz, tx_poff, tx_noff, tx_pout, tx_nout, tx_info, tx_gaf, path_stats;
    uint64_t tx_n_acc = 0, tx_pbytes = 0, tx_nbytes = 0;
    bool blocking_sync = bgr::opt("blocking_sync") != 0;
    hipEvent_t ev_wait = nullptr;
    const uint8_t* tx_text = nullptr;  // where the last call's piece lies in HBM (tx_in, or the caller's stage)
    uint32_t tx_flip = 0;              // which of the two info blocks the current piece uses
    uint32_t tx_epoch = 0, tx_ticket[2] = {0, 0};   // the one-launch kernels' chains: epoch of the last launch; tickets earlier launches took (parse, format)
    bool tx_written = false;           // the streams lie in tx_pout / tx_nout (the format launch wrote them: every stretch ended below the capacities)
    uint32_t tx_want = 0;              // its want_output (2 = correction mode: mapped reads as spelled by their paths, 3 = GAF lines)
    double tx_phase_s[5] = {0, 0, 0, 0, 0};  // BGREAT_TIMING: host wall seconds to the call's four waits (mark, records, mapping + sizes, streams) + calls

    DevBuf in_reads, in_offs, pk_fw3, pk_nm, pk_hasn, results, arena, ovf, ovf2, lst, deepbuf, retry, retry2, small, csr_sums, csr_poffs, csr_status, csr_paths;  // small: kSmall* (align_kernels.h)
    struct DeepRun {  // the last pass of the exhaustive launch in flight, as enqueued: settle_launch runs it again for reads whose table filled up
        bool open = false;
        bgr::Pass pass;
        bgr::BatchIO io;
        bgr::KernelParams kp;
        BgrDeviceGraph dg;
        uint32_t per_wave_lds = 0, path_cap = 0, memo_cap = 0, runs = 0;
    } deep;
    bgr::PlanDevice plan_dev;     // CUs, LDS, resident waves per kernel: asked once
    bool plan_dev_known = false;
    uint64_t last_n = 0;
    uint32_t last_mode = 0;       // mode of the last mapping launch (bgr_aligner_path_stats)
    DevBuf wave_times;            // diagnostic builds only (-DBGR_PHASE_TIMING)
    uint64_t wave_times_n = 0;
    uint64_t ticket_serial = 0;       // bgr_align_batch_begin: tickets handed out; the batch of the last one is in flight until its wait
    bool ticket_open = false;
    std::vector<uint64_t> ticket_offs;  // that batch's offsets made relative (kept alive for the asynchronous copy)
    uint32_t last_launch[4] = {0, 0, 0, 0};
    uint32_t cfg_waves = 0, cfg_blocks_per_cu = 0, cfg_lds_mphf = 0;
    bool exh_filter = bgr::opt("exh_filter") != 0;  // exhaustive mode through the minimizer filter too (option exh_filter = 0: without)
    // bgr_aligner_set_knob (test / diagnostic hooks, read here instead of from the environment on every launch)
    uint32_t knob_frame_cap = 0, knob_search = 0, knob_debug_stop = 0, knob_greedy_fast = 0, knob_exh_fast = 0, knob_anc_fast = 0, knob_memo_cap = 0, knob_prepass = 0, knob_no_events = 0;
    uint64_t knob_split_limit = 0;
    uint32_t knob_overlap = 0;      // BGR_KNOB_BATCH_OVERLAP
    uint32_t knob_abundance_form = 0;  // BGR_KNOB_ABUNDANCE_FORM
    bool abundance_on = false;      // bgr_aligner_abundance_enable: every greedy / anchors launch is followed by the abundance kernel
    DevBuf abundance;               // u64[n_unitigs + 1][3], allocated and zeroed on the first enable
    uint32_t knob_links_form = 0;   // BGR_KNOB_LINKS_FORM
    bool links_on = false;          // bgr_aligner_links_enable: every greedy / anchors launch is followed by the links kernel
    DevBuf links;                   // {u64 key, u64 count}[links_cap] + the tail words (links_kernels.h), allocated and zeroed on the first enable
    unsigned long long* links_tab = nullptr;   // the table this aligner's launches add to: its own, or (a twin) the one of the aligner it belongs to
    uint64_t links_cap = 0, links_bound = 0;
    bool pileup_on = false;         // bgr_aligner_pileup_enable: every greedy / anchors launch is followed by the pileup kernel
    DevBuf pileup, pileup_offs;     // the table (pileup_kernels.h) and base_offs, allocated, zeroed / uploaded on the first enable
    uint32_t* pileup_tab = nullptr;             // the table this aligner's launches add to: its own, or (a twin) the one of the aligner it belongs to
    const uint64_t* pileup_base_offs = nullptr;
    bool strands_on = false;        // bgr_aligner_pileup_strands_enable: the pileup kernel also adds the forward observations to a second table
    DevBuf pileup_fwd;              // that table: the layout of `pileup`, its tail stays 0
    uint32_t* pileup_fwd_tab = nullptr;   // as pileup_tab: its own, or (a twin) the one of the aligner it belongs to
    DevBuf var_scratch, var_out, var_stage;   // bgr_aligner_pileup_sites: the passes' tile arrays and the records; bgr_aligner_pileup_add: the staging piece
    double var_ms[5] = {0, 0, 0, 0, 0};       // the last call's five launches
    bgr_aligner* twin = nullptr;    // second stream + buffers for the overlapped form of bgr_align_batch (created on first use)
    bool is_twin = false;
    int num_cus = 0;
    size_t lds_per_cu = 0;
    hipEvent_t ev[kTimerRing][kTimerSlots + 1];  // ev[i][0] = start of launch i, ev[i][j] = behind its j-th kernel
    int ev_marks[kTimerRing];                    // kernels timed in launch i
    int ev_used = 0;
    uint64_t t_launches = 0;
    double t_ms = 0, t_slot_ms[kTimerSlots] = {0, 0, 0, 0, 0, 0, 0, 0};
    const char* t_slot_name[kTimerSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

namespace {

// Wait for the aligner's stream.  By default hipStreamSynchronize (the runtime spins: lowest latency, one busy CPU per waiting thread);
// with BGREAT_BLOCKING_SYNC=1 an event made with hipEventBlockingSync is recorded and waited for instead: the thread sleeps until the
// interrupt, so more stream workers per device than CPUs to spare can overlap their calls (bgr_align_all's text route).
hipError_t wait_stream(bgr_aligner* a) {
    if (!a->blocking_sync) return hipStreamSynchronize(a->stream);
    hipError_t e = hipEventRecord(a->ev_wait, a->stream);
    return e == hipSuccess ? hipEventSynchronize(a->ev_wait) : e;
}

int drain_timers(bgr_aligner* a) {
    if (a->ev_used == 0) return BGR_OK;
    HIP_TRY(hipStreamSynchronize(a->stream));
    for (int i = 0; i < a->ev_used; ++i) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, a->ev[i][0], a->ev[i][a->ev_marks[i]]));
        a->t_ms += ms;
        for (int j = 0; j < a->ev_marks[i]; ++j) {
            HIP_TRY(hipEventElapsedTime(&ms, a->ev[i][j], a->ev[i][j + 1]));
            a->t_slot_ms[j] += ms;
        }
        ++a->t_launches;
    }
    a->ev_used = 0;
    return BGR_OK;
}

}  // namespace

extern "C" {

const char* bgr_last_error(void) { return tl_err.c_str(); }

int bgr_set_option(const char* name, int64_t value) {
    bgr::Option* o = name ? bgr::find_option(name) : nullptr;
    if (!o) return fail(BGR_E_ARG, std::string("bgr_set_option: unknown option '") + (name ? name : "") + "'");
    if (value < o->lo || value > o->hi) return fail(BGR_E_ARG, std::string("bgr_set_option: value out of range for '") + name + "'");
    o->value.store(value, std::memory_order_relaxed);
    return BGR_OK;
}
int bgr_get_option(const char* name, int64_t* value) {
    bgr::Option* o = name ? bgr::find_option(name) : nullptr;
    if (!o || !value) return fail(BGR_E_ARG, std::string("bgr_get_option: unknown option '") + (name ? name : "") + "'");
    *value = o->value.load(std::memory_order_relaxed);
    return BGR_OK;
}
const char* bgr_option_name(uint32_t index, const char** what) {
    size_t n;
    bgr::Option* t = bgr::option_table(&n);
    if (index >= n) return nullptr;
    if (what) *what = t[index].what;
    return t[index].name;
}
void bgr_set_build_threads(uint32_t threads) { bgr::set_build_threads(threads); }

int bgr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- index ------------------------------------------------------------------------------------------
int bgr_graph_build(uint32_t k, uint64_t n_unitigs, const char* seqs, const uint64_t* offsets, double gamma, bgr_graph** out) {
    return bgr_graph_build_ex(k, n_unitigs, seqs, offsets, gamma, 0, out);
}

int bgr_graph_build_ex(uint32_t k, uint64_t n_unitigs, const char* seqs, const uint64_t* offsets, double gamma, uint32_t flags, bgr_graph** out) {
    if (!out || (n_unitigs && (!seqs || !offsets))) return fail(BGR_E_ARG, "bgr_graph_build: null argument");
    if (flags & ~(uint32_t)(BGR_BUILD_ANCHORS | BGR_BUILD_NO_EVICTIONS)) return fail(BGR_E_ARG, "bgr_graph_build: unknown flag");
    bgr_graph* g = new bgr_graph();
    std::string err;
    uint64_t zero[1] = {0};
    if (!bgr::build_graph(k, n_unitigs, seqs, n_unitigs ? offsets : zero, gamma > 0 ? gamma : 0.0, flags, g->host, err)) {
        delete g;
        return fail(BGR_E_ARG, err);
    }
    g->header = *g->host.header();
    const uint64_t nu = g->header.n_unitigs;  // loading stopped at the first short sequence
    g->ascii.assign(seqs + (nu ? offsets[0] : 0), seqs + (nu ? offsets[nu] : 0));
    g->ascii_offs.resize(nu + 1);
    for (uint64_t i = 0; i <= nu; ++i) g->ascii_offs[i] = nu ? offsets[i] - offsets[0] : 0;
    *out = g;
    return BGR_OK;
}

int bgr_graph_unitigs(const bgr_graph* g, const char** seqs, const uint64_t** offsets, uint64_t* n) {
    if (!g || !seqs || !offsets || !n) return fail(BGR_E_ARG, "bgr_graph_unitigs: null argument");
    if (g->ascii_offs.empty()) return fail(BGR_E_ARG, "bgr_graph_unitigs: this graph was created from a blob and carries no unitig characters");
    *seqs = g->ascii.data();
    *offsets = g->ascii_offs.data();
    *n = g->ascii_offs.size() - 1;
    return BGR_OK;
}

int bgr_graph_build_from_fasta(const char* path, uint32_t k, double gamma, bgr_graph** out) {
    return bgr_graph_build_from_fasta_ex(path, k, gamma, 0, out);
}

int bgr_graph_build_from_fasta_ex(const char* path, uint32_t k, double gamma, uint32_t flags, bgr_graph** out) {
    if (!path || !out) return fail(BGR_E_ARG, "bgr_graph_build_from_fasta: null argument");
    std::vector<char> seqs;
    std::vector<uint64_t> offs;
    std::string err;
    if (!bgr::read_unitig_fasta(path, k, seqs, offs, err)) return fail(BGR_E_IO, err);
    return bgr_graph_build_ex(k, offs.size() - 1, seqs.data(), offs.data(), gamma, flags, out);
}

int bgr_graph_anchor_lookup(const bgr_graph* g, uint64_t kmer, uint64_t* index_out, uint64_t* position_out) {
    if (!g || !index_out) return fail(BGR_E_ARG, "bgr_graph_anchor_lookup: null argument");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_anchor_lookup: graph has no host blob");
    if (!g->header.anc_n) return fail(BGR_E_ARG, "bgr_graph_anchor_lookup: the graph was built without BGR_BUILD_ANCHORS");
    const uint64_t idx = bgr::anchor_lookup(g->host.header(), g->host.base(), kmer);
    *index_out = idx;
    if (position_out) *position_out = idx == ~0ULL ? 0 : reinterpret_cast<const uint64_t*>(g->host.base() + g->header.off_anc_pos)[idx];
    return BGR_OK;
}

int bgr_graph_key_lookup(const bgr_graph* g, uint64_t key, uint32_t* slot_out) {
    if (!g || !slot_out) return fail(BGR_E_ARG, "bgr_graph_key_lookup: null argument");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_key_lookup: graph has no host blob");
    if (g->header.wide_keys) return fail(BGR_E_ARG, "bgr_graph_key_lookup: the graph has two-word keys (k > 32): use bgr_graph_key_lookup_wide");
    *slot_out = bgr::host_lookup(g->host.header(), g->host.base(), key);
    return BGR_OK;
}

int bgr_graph_key_lookup_wide(const bgr_graph* g, uint64_t key_hi, uint64_t key_lo, uint32_t* slot_out) {
    if (!g || !slot_out) return fail(BGR_E_ARG, "bgr_graph_key_lookup_wide: null argument");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_key_lookup_wide: graph has no host blob");
    *slot_out = bgr::host_lookup_wide(g->host.header(), g->host.base(), key_hi, key_lo);
    return BGR_OK;
}

const void* bgr_graph_blob(const bgr_graph* g, uint64_t* bytes) {
    if (!g || g->host.blob.empty()) { if (bytes) *bytes = 0; return nullptr; }
    if (bytes) *bytes = g->header.blob_bytes;
    return g->host.blob.data();
}

int bgr_graph_from_blob(const void* blob, uint64_t bytes, bgr_graph** out) {
    if (!blob || !out) return fail(BGR_E_ARG, "bgr_graph_from_blob: null argument");
    std::string err;
    if (!bgr::validate_blob(blob, bytes, err)) return fail(BGR_E_ARG, err);
    bgr_graph* g = new bgr_graph();
    if (!g->host.blob.reset((bytes + 7) / 8)) { delete g; return fail(BGR_E_ARG, "bgr_graph_from_blob: out of memory"); }
    memcpy(g->host.blob.data(), blob, bytes);
    g->header = *g->host.header();
    *out = g;
    return BGR_OK;
}

int bgr_graph_info(const bgr_graph* g, bgr_graph_info_t* o) {
    if (!g || !o) return fail(BGR_E_ARG, "bgr_graph_info: null argument");
    const BgrBlobHeader& h = g->header;
    memset(o, 0, sizeof(*o));
    o->k = h.k; o->n_levels = 2; o->n_unitigs = h.n_unitigs; o->n_keys = h.n_placed + h.n_fallback;
    o->n_left_keys = h.n_left_keys; o->n_right_keys = h.n_right_keys; o->n_fallback = h.n_fallback;
    o->total_bases = h.total_bases; o->blob_bytes = h.blob_bytes; o->mphf_bytes = h.n_buckets * 4;
    o->max_unitig_len = h.max_unitig_len; o->has_exceptions = h.has_exc; o->has_anchors = h.anc_n ? 1 : 0; o->gamma = h.gamma;
    return BGR_OK;
}

void bgr_graph_destroy(bgr_graph* g) {
    if (!g) return;
    for (auto& kv : g->dev) {
        if (kv.second.owned && kv.second.ptr) {
            if (hipSetDevice(kv.first) == hipSuccess) (void)hipFree(kv.second.ptr);
        }
    }
    variants_run_free(g);
    delete g;
}

int bgr_graph_upload(bgr_graph* g, int device) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_upload: null graph");
    if (g->dev.count(device)) return BGR_OK;
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_upload: graph has no host blob (adopted graphs live on one device)");
    HIP_TRY(hipSetDevice(device));
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, g->header.blob_bytes));
    hipError_t e = hipMemcpy(p, g->host.blob.data(), g->header.blob_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (from pageable memory on the null stream; the aligners' streams are non-blocking: the blob is there before any of them starts)
    if (e != hipSuccess) { (void)hipFree(p); return fail(BGR_E_HIP, std::string("blob H2D: ") + hipGetErrorString(e)); }
    g->dev[device] = {p, true};
    return BGR_OK;
}

// ---- one-off distribution of the graph over the GPUs of one process -------------------------------------------------------
// The blob goes from the host to the first device once and from there device to device over xGMI: as ONE RCCL broadcast
// (a communicator per device from ncclCommInitAll; librccl is looked up at run time, so the library has no link-time
// dependency on it), or, when RCCL is not available or refuses, as peer copies in a doubling schedule (1 -> 2 -> 4 -> 8
// holders: every round uses disjoint point-to-point links).
namespace {

struct Rccl {
    typedef int (*CommInitAll_t)(void** comms, int n, const int* devs);
    typedef int (*Group_t)(void);
    typedef int (*Broadcast_t)(const void* send, void* recv, size_t count, int dtype, int root, void* comm, hipStream_t stream);
    typedef int (*CommDestroy_t)(void* comm);
    void* lib = nullptr;
    CommInitAll_t CommInitAll = nullptr;
    Group_t GroupStart = nullptr, GroupEnd = nullptr;
    Broadcast_t Broadcast = nullptr;
    CommDestroy_t CommDestroy = nullptr;
    bool load() {
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) return false;
        CommInitAll = reinterpret_cast<CommInitAll_t>(dlsym(lib, "ncclCommInitAll"));
        GroupStart = reinterpret_cast<Group_t>(dlsym(lib, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<Group_t>(dlsym(lib, "ncclGroupEnd"));
        Broadcast = reinterpret_cast<Broadcast_t>(dlsym(lib, "ncclBroadcast"));
        CommDestroy = reinterpret_cast<CommDestroy_t>(dlsym(lib, "ncclCommDestroy"));
        return CommInitAll && GroupStart && GroupEnd && Broadcast && CommDestroy;
    }
};

// ptr[i] on device devs[i]; ptr[0] holds the blob.  false = RCCL not usable here (nothing has been copied, or partly:
// the caller then overwrites with peer copies).
bool fanout_rccl(const std::vector<int>& devs, const std::vector<void*>& ptr, uint64_t bytes, std::string& why) {
    Rccl r;
    if (!r.load()) { why = "librccl not loadable"; return false; }
    const int n = (int)devs.size();
    std::vector<void*> comms(n, nullptr);
    if (r.CommInitAll(comms.data(), n, devs.data()) != 0) { why = "ncclCommInitAll failed"; return false; }
    std::vector<hipStream_t> streams(n, nullptr);
    bool ok = true;
    for (int i = 0; i < n && ok; ++i) ok = hipSetDevice(devs[i]) == hipSuccess && hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking) == hipSuccess;
    if (ok) {
        ok = r.GroupStart() == 0;
        for (int i = 0; i < n && ok; ++i) {
            ok = hipSetDevice(devs[i]) == hipSuccess &&
                 r.Broadcast(ptr[i], ptr[i], (size_t)bytes, /*ncclChar*/ 0, /*root rank*/ 0, comms[i], streams[i]) == 0;
        }
        ok = r.GroupEnd() == 0 && ok;
    }
    for (int i = 0; i < n; ++i) {
        if (streams[i]) { if (hipSetDevice(devs[i]) == hipSuccess) { ok = hipStreamSynchronize(streams[i]) == hipSuccess && ok; (void)hipStreamDestroy(streams[i]); } }
    }
    for (void* c : comms) if (c) (void)r.CommDestroy(c);
    if (!ok) why = "RCCL broadcast failed";
    return ok;
}

// one round of the doubling schedule: concurrent peer copies over disjoint links, complete on return
bool peer_round(const std::vector<bgr::FanoutCopy>& round, uint64_t bytes, std::string& why) {
    std::vector<hipStream_t> streams;
    std::vector<int> sdev;
    bool ok = true;
    for (const bgr::FanoutCopy& c : round) {
        if (hipSetDevice(c.src_dev) != hipSuccess) { ok = false; why = "hipSetDevice failed"; break; }
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, c.src_dev, c.dst_dev) == hipSuccess && can) {
            hipError_t pe = hipDeviceEnablePeerAccess(c.dst_dev, 0);  // direct xGMI path; without it the runtime stages through the host
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        }
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { ok = false; why = "hipStreamCreate failed"; break; }
        streams.push_back(st);
        sdev.push_back(c.src_dev);
        hipError_t e = hipMemcpyPeerAsync(c.dst, c.dst_dev, c.src, c.src_dev, bytes, st);
        if (e != hipSuccess) { ok = false; why = std::string("hipMemcpyPeerAsync: ") + hipGetErrorString(e); break; }
    }
    for (size_t j = 0; j < streams.size(); ++j) {  // (also after a failure: nothing may still be writing when the buffers are released)
        if (hipSetDevice(sdev[j]) == hipSuccess) {
            hipError_t e = hipStreamSynchronize(streams[j]);
            if (e != hipSuccess && ok) { ok = false; why = std::string("peer copy: ") + hipGetErrorString(e); }
            (void)hipStreamDestroy(streams[j]);
        }
    }
    return ok;
}

}  // namespace

int bgr_devices_init(bgr_graph* g, int first_device, uint32_t n_devices, uint32_t how) {
    if (!g) return fail(BGR_E_ARG, "bgr_devices_init: null graph");
    if (n_devices == 0) n_devices = 1;
    if (how > BGR_FANOUT_PEER) return fail(BGR_E_ARG, "bgr_devices_init: unknown distribution method");
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return fail(BGR_E_HIP, "no HIP device available");
    if (first_device < 0 || (uint64_t)first_device + n_devices > (uint64_t)nd) return fail(BGR_E_ARG, "bgr_devices_init: device range outside the visible devices");
    int rc = bgr_graph_upload(g, first_device);  // host -> first device (idempotent)
    if (rc != BGR_OK) return rc;
    const uint64_t bytes = g->header.blob_bytes;
    bgr::FanoutOps ops;
    ops.alloc = [bytes](int dev, void** out) { return hipSetDevice(dev) == hipSuccess && hipMalloc(out, bytes) == hipSuccess; };
    ops.release = [](int dev, void* p) { if (p && hipSetDevice(dev) == hipSuccess) (void)hipFree(p); };
    ops.broadcast = [bytes](const std::vector<int>& devs, const std::vector<void*>& ptr, std::string& why) { return fanout_rccl(devs, ptr, bytes, why); };
    ops.peer_round = [bytes](const std::vector<bgr::FanoutCopy>& round, std::string& why) { return peer_round(round, bytes, why); };
    // (bookkeeping in fanout.h: new buffers are registered only once they hold the blob; after a failure they are released and
    // g->dev is unchanged, so bgr_graph_upload / bgr_aligner_create can still bring the blob to a device on their own)
    std::map<int, void*> resident;
    for (auto& kv : g->dev) resident[kv.first] = kv.second.ptr;
    g->fanout_method = 0;
    const bgr::FanoutResult r = bgr::fanout_blob(first_device, n_devices, how, resident, ops);
    if (!r.error.empty()) return fail(r.hip_error ? BGR_E_HIP : BGR_E_ARG, "bgr_devices_init: " + r.error);
    for (auto& kv : resident) if (!g->dev.count(kv.first)) g->dev[kv.first] = {kv.second, true};
    g->fanout_method = (uint32_t)r.method;
    return BGR_OK;
}

uint32_t bgr_devices_method(const bgr_graph* g) { return g ? g->fanout_method : 0; }

const void* bgr_graph_device_blob(const bgr_graph* g, int device) {
    if (!g) return nullptr;
    auto it = g->dev.find(device);
    return it == g->dev.end() ? nullptr : it->second.ptr;
}

int bgr_graph_adopt_device_blob(int device, const void* dev_blob, uint64_t bytes, bgr_graph** out) {
    if (!dev_blob || !out || bytes < sizeof(BgrBlobHeader)) return fail(BGR_E_ARG, "bgr_graph_adopt_device_blob: bad argument");
    HIP_TRY(hipSetDevice(device));
    bgr_graph* g = new bgr_graph();
    hipError_t e = hipMemcpy(&g->header, dev_blob, sizeof(BgrBlobHeader), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { delete g; return fail(BGR_E_HIP, std::string("header D2H: ") + hipGetErrorString(e)); }
    std::string verr;  // the same checks as for a host blob: the kernels index HBM with these numbers
    if (!bgr::validate_blob_header(&g->header, bytes, verr)) {
        delete g;
        return fail(BGR_E_ARG, "bgr_graph_adopt_device_blob: " + verr);
    }
    g->dev[device] = {const_cast<void*>(dev_blob), false};
    *out = g;
    return BGR_OK;
}

// ---- mapping ----------------------------------------------------------------------------------------
int bgr_aligner_create(bgr_graph* g, int device, bgr_aligner** out) {
    if (!g || !out) return fail(BGR_E_ARG, "bgr_aligner_create: null argument");
    int nd = 0;
    hipError_t e0 = hipGetDeviceCount(&nd);
    if (e0 != hipSuccess || nd == 0) return fail(BGR_E_HIP, "no HIP device available (this library has no CPU mapping path)");
    if (device < 0 || device >= nd) return fail(BGR_E_ARG, "bgr_aligner_create: device index out of range");
    int rc = bgr_graph_upload(g, device);
    if (rc != BGR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    bgr_aligner* a = new bgr_aligner();
    a->graph = g;
    a->device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) { delete a; return fail(BGR_E_HIP, hipGetErrorString(e)); }
    a->num_cus = prop.multiProcessorCount;
    a->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 65536;
    e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete a; return fail(BGR_E_HIP, hipGetErrorString(e)); }
    for (int i = 0; i < kTimerRing; ++i) {
        for (int j = 0; j <= kTimerSlots; ++j) {
            if (hipEventCreate(&a->ev[i][j]) != hipSuccess) {
                delete a;
                return fail(BGR_E_HIP, "hipEventCreate failed");
            }
        }
    }
    if (a->blocking_sync && hipEventCreateWithFlags(&a->ev_wait, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) a->blocking_sync = false;
    bgr::resolve_device_graph(&g->header, g->dev[device].ptr, a->dg);
    e = a->small.ensure(bgr::kSmallBytes);
    if (e == hipSuccess) e = hipMemset(a->small.p, 0, a->small.cap);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (the fill runs on the null stream, which the aligner's non-blocking stream does not wait for)
    if (e != hipSuccess) { delete a; return fail(BGR_E_HIP, hipGetErrorString(e)); }
    *out = a;
    return BGR_OK;
}

void bgr_aligner_destroy(bgr_aligner* a) {
    if (!a) return;
    if (a->tx_phase_s[4] > 0 && bgr::opt("timing"))
        fprintf(stderr, "bgreat: text calls %.0f on device %d: to record count %.3f s, records %.3f s, mapping + sizes %.3f s, streams out %.3f s\n", a->tx_phase_s[4], a->device,
                a->tx_phase_s[0], a->tx_phase_s[1], a->tx_phase_s[2], a->tx_phase_s[3]);
    if (a->twin) { bgr_aligner_destroy(a->twin); a->twin = nullptr; }
    if (hipSetDevice(a->device) == hipSuccess) {
        if (a->stream) (void)hipStreamSynchronize(a->stream);
        a->in_reads.release(); a->in_offs.release(); a->pk_fw3.release(); a->pk_nm.release(); a->pk_hasn.release(); a->results.release(); a->arena.release(); a->ovf.release(); a->ovf2.release(); a->lst.release(); a->deepbuf.release(); a->retry.release(); a->retry2.release(); a->small.release();
        a->csr_sums.release(); a->csr_poffs.release(); a->csr_status.release(); a->csr_paths.release(); a->wave_times.release(); a->abundance.release(); a->links.release(); a->pileup.release(); a->pileup_offs.release(); a->pileup_fwd.release(); a->var_scratch.release(); a->var_out.release(); a->var_stage.release();
        for (DevBuf* b : {&a->tx_in, &a->tx_sums, &a->tx_state, &a->tx_rec, &a->tx_idx, &a->tx_accrec, &a->tx_accsrc, &a->tx_offs,
                          &a->tx_psz, &a->tx_nsz, &a->tx_poff, &a->tx_noff, &a->tx_pout, &a->tx_nout, &a->tx_info, &a->tx_gaf, &a->path_stats}) b->release();
        for (int i = 0; i < kTimerRing; ++i) for (int j = 0; j <= kTimerSlots; ++j) (void)hipEventDestroy(a->ev[i][j]);
        if (a->ev_wait) (void)hipEventDestroy(a->ev_wait);
        if (a->stream) (void)hipStreamDestroy(a->stream);
    }
    delete a;
}

int bgr_aligner_configure(bgr_aligner* a, uint32_t waves_per_block, uint32_t blocks_per_cu, uint32_t lds_mphf) {
    if (!a || waves_per_block > 16 || lds_mphf > 2) return fail(BGR_E_ARG, "bgr_aligner_configure: bad argument");
    a->cfg_waves = waves_per_block;
    a->cfg_blocks_per_cu = blocks_per_cu;
    a->cfg_lds_mphf = lds_mphf;
    return BGR_OK;
}

int bgr_aligner_set_knob(bgr_aligner* a, uint32_t knob, uint64_t value) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_set_knob: null aligner");
    switch (knob) {
        case BGR_KNOB_EXH_FRAME_CAP: a->knob_frame_cap = (uint32_t)std::min<uint64_t>(value, 1u << 20); return BGR_OK;
        case BGR_KNOB_EXH_SEARCH: if (value > 2) break; a->knob_search = (uint32_t)value; return BGR_OK;
        case BGR_KNOB_BATCH_SPLIT_LIMIT: a->knob_split_limit = value; return BGR_OK;
        case BGR_KNOB_DEBUG_STOP: a->knob_debug_stop = (uint32_t)value; return BGR_OK;
        case BGR_KNOB_BATCH_OVERLAP: a->knob_overlap = (uint32_t)value; return BGR_OK;
        case BGR_KNOB_GREEDY_FAST: if (value > 1) break; a->knob_greedy_fast = (uint32_t)value; return BGR_OK;
        case BGR_KNOB_EXH_FAST: if (value > 1) break; a->knob_exh_fast = (uint32_t)value; return BGR_OK;
        case BGR_KNOB_ANCHORS_FAST: if (value > 1) break; a->knob_anc_fast = (uint32_t)value; return BGR_OK;
        case BGR_KNOB_GREEDY_PREPASS: if (value > 1) break; a->knob_prepass = (uint32_t)value; return BGR_OK;
        case BGR_KNOB_KERNEL_EVENTS: if (value > 1) break; a->knob_no_events = value ? 0u : 1u; return BGR_OK;
        case BGR_KNOB_ABUNDANCE_FORM: if (value > 2) break; a->knob_abundance_form = (uint32_t)value; for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) tw->knob_abundance_form = (uint32_t)value; return BGR_OK;
        case BGR_KNOB_LINKS_FORM: if (value > 2) break; a->knob_links_form = (uint32_t)value; for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) tw->knob_links_form = (uint32_t)value; return BGR_OK;
        case BGR_KNOB_EXH_MEMO_CAP: a->knob_memo_cap = (uint32_t)std::min<uint64_t>(value, 1u << 24); return BGR_OK;
        default: break;
    }
    return fail(BGR_E_ARG, "bgr_aligner_set_knob: unknown knob or value out of range");
}

// What the planner needs of the graph / device / caller's tuning (launch_plan.h)
static bgr::PlanGraph plan_graph_of(const BgrBlobHeader& h) {
    bgr::PlanGraph g;
    g.k = h.k; g.slot_fill_x100 = h.slot_fill_x100; g.table_bytes = (uint32_t)std::min<uint64_t>((uint64_t)h.n_buckets * 4, 0xFFFFFFFFull);
    g.total_bases = h.total_bases; g.n_unitigs = h.n_unitigs; g.n_buckets = h.n_buckets; g.max_unitig_len = h.max_unitig_len;
    g.anc_n = h.anc_n; g.anc_active_levels = h.anc_active_levels; g.has_exc = h.has_exc != 0; g.wide_keys = h.wide_keys != 0;
    return g;
}
static bgr::PlanTuning plan_tuning_of(const bgr_aligner* a) {
    bgr::PlanTuning t;
    t.cfg_waves = a->cfg_waves; t.cfg_blocks_per_cu = a->cfg_blocks_per_cu; t.cfg_lds_mphf = a->cfg_lds_mphf;
    t.frame_cap = a->knob_frame_cap; t.search = a->knob_search; t.memo_cap = a->knob_memo_cap;
    t.no_greedy_fast = a->knob_greedy_fast != 0; t.no_exh_fast = a->knob_exh_fast != 0; t.no_anc_fast = a->knob_anc_fast != 0;
    return t;
}

// The planner by itself, on numbers (no device, no graph object): what tests/test_launch_plan.py sweeps on the CPU.
extern "C" int bgr_plan_launch(const bgr_plan_input* in, bgr_plan_output* out) {
    if (!in || !out) return fail(BGR_E_ARG, "bgr_plan_launch: null argument");
    bgr::PlanGraph g;
    g.k = in->k; g.slot_fill_x100 = in->slot_fill_x100; g.table_bytes = in->table_bytes; g.total_bases = in->graph_bases; g.n_unitigs = in->n_unitigs;
    g.n_buckets = in->table_bytes / 4; g.max_unitig_len = in->max_unitig_len; g.anc_n = in->anchors ? 1 : 0; g.anc_active_levels = in->anchor_levels; g.has_exc = in->has_exceptions != 0;
    g.wide_keys = in->wide_keys != 0;
    bgr::PlanDevice d;
    if (in->num_cus) d.num_cus = in->num_cus;
    if (in->lds_per_cu) d.lds_per_cu = in->lds_per_cu;
    for (uint32_t i = 0; i < bgr::kResidentKernels; ++i) if (in->resident_waves[i]) d.resident[i] = in->resident_waves[i];
    bgr::PlanTuning t;
    t.cfg_waves = in->cfg_waves; t.cfg_blocks_per_cu = in->cfg_blocks_per_cu; t.cfg_lds_mphf = in->cfg_lds_mphf;
    bgr::PlanBatch b;
    b.mode = in->mode; b.max_mismatch = in->max_mismatch; b.partial = in->partial; b.max_read_len = in->max_read_len; b.n_reads = in->n_reads; b.total_bases = in->total_bases;
    const bgr::LaunchPlan P = bgr::plan_launch(g, d, t, b);
    memset(out, 0, sizeof(*out));
    if (P.error) return fail(BGR_E_ARG, P.error);
    auto put = [out](int slot, const bgr::LaunchCfg& c) {
        out->pass[slot] = bgr_plan_pass{1, c.blocks, c.waves_per_block, c.lds_bytes, c.stage_mphf};
    };
    // slot 0: the mode's general kernel, the first pass that maps one read per wave (in a launch that sends every read to the last pass: that pass)
    const uint32_t general = bgr::many_reads_per_wave(P.pass[0].kernel) ? 1 : 0;
    for (uint32_t i = 0; i < P.n_passes; ++i) {
        const bgr::Pass& ps = P.pass[i];
        if (i == general) put(0, ps.cfg);
        switch (ps.kernel) {
            case bgr::KernelId::kGreedyMulti: put(1, ps.cfg); break;
            case bgr::KernelId::kExhaustive4: put(2, ps.cfg); break;
            case bgr::KernelId::kAnchors4: put(3, ps.cfg); break;
            case bgr::KernelId::kExhaustive: if (i != general) put(4, ps.cfg); break;  // (behind the level search)
            case bgr::KernelId::kExhaustiveLast: put(5, ps.cfg); break;
            default: break;
        }
    }
    out->level_search = P.level_search; out->deep_only = P.pass[0].kernel == bgr::KernelId::kExhaustiveLast; out->x4_levels = P.x4_levels; out->memo_cap = P.memo_cap;
    out->deep_scratch_bytes = P.deep_scratch_bytes;
    out->arena_ints = P.arena_cap;
    return BGR_OK;
}

// The buffer of each list of reads a pass leaves to a later one (bgr::List; greedy mode keeps the follow-up items' rings in `ovf`)
static DevBuf* list_buf(bgr_aligner* a, bgr::List l) {
    switch (l) {
        case bgr::List::kSearch: return &a->ovf;
        case bgr::List::kDepthFirst: case bgr::List::kGeneral: return &a->ovf2;
        case bgr::List::kFirst: return &a->lst;
        case bgr::List::kRetry: return &a->retry;
        default: return nullptr;
    }
}

// The mapping launch of one batch: the passes come from plan_launch (launch_plan.h, a pure function of numbers), this function sizes the
// buffers and enqueues.  planes_ready: the aligner's 2-bit planes (pk_fw3 / pk_nm / pk_hasn) already hold the batch
// (bgr_align_batch_packed copied them in); else they are made from the ASCII reads at d_reads by the pre-pass.
// d_src_off (may be null): where each read's characters start in d_reads when they lie scattered in a text (text route); reads_bytes: bytes of d_reads.
// the geometry and form of the abundance kernel behind a launch of this size (bgr_aligner_abundance_plan reports what this returns)
static bgr::AbundancePlan abundance_plan_of(const bgr_aligner* a, uint64_t n_reads, uint64_t total_bases) {
    return bgr::plan_abundance(a->graph->header.n_unitigs, a->dg.k, n_reads, total_bases, (uint32_t)a->num_cus, a->lds_per_cu, a->knob_abundance_form);
}

static int align_device_impl(bgr_aligner* a, const bgr_params* p, const void* d_reads, const void* d_read_offsets, uint64_t n_reads,
                             uint64_t total_bases, uint32_t max_read_len, bool planes_ready, const void* d_src_off = nullptr, uint64_t reads_bytes = 0,
                             bool cursor_is_zero = false) {
    if (!a || !p) return fail(BGR_E_ARG, "bgr_align_device: null argument");
    if (p->mode > BGR_MODE_ANCHORS) return fail(BGR_E_ARG, "bgr_align_device: unknown mode");
    if (p->mode == BGR_MODE_ANCHORS && !a->graph->header.anc_n)
        return fail(BGR_E_ARG, "bgr_align_device: BGR_MODE_ANCHORS needs a graph built with BGR_BUILD_ANCHORS");
    if (p->mode != BGR_MODE_GREEDY && a->graph->header.wide_keys)
        return fail(BGR_E_ARG, "bgr_align_device: a graph with k > 32 (two-word keys) maps in greedy mode only; exhaustive mode (-b) needs k <= 32");
    if (a->abundance_on && p->mode == BGR_MODE_EXHAUSTIVE)
        return fail(BGR_E_ARG, "bgr_align_device: this aligner counts unitig abundance (bgr_aligner_abundance_enable), which is defined on the rows of the greedy modes; exhaustive mode (-b) is refused");
    if (a->links_on && p->mode == BGR_MODE_EXHAUSTIVE)
        return fail(BGR_E_ARG, "bgr_align_device: this aligner counts links (bgr_aligner_links_enable), which are defined on the rows of the greedy modes; exhaustive mode (-b) is refused");
    if (a->pileup_on && p->mode == BGR_MODE_EXHAUSTIVE)
        return fail(BGR_E_ARG, "bgr_align_device: this aligner counts a pileup (bgr_aligner_pileup_enable), which is defined on the rows of the greedy modes; exhaustive mode (-b) is refused");
    a->last_n = n_reads;
    a->last_mode = p->mode;
    a->deep.open = false;
    a->deep.runs = 0; a->deep.memo_cap = 0;
    if (n_reads == 0) return BGR_OK;
    if ((!d_reads && !planes_ready) || !d_read_offsets) return fail(BGR_E_ARG, "bgr_align_device: null device buffer");
    if (n_reads >= 0xFFFFFFFFull) return fail(BGR_E_ARG, "bgr_align_device: more than 2^32-2 reads in one batch");
    HIP_TRY(hipSetDevice(a->device));
    if (a->ev_used == kTimerRing) { int rc = drain_timers(a); if (rc != BGR_OK) return rc; }
    HIP_TRY(a->results.ensure(n_reads * 8));

    // ---- launch geometry (launch_plan.h) ------------------------------------------------------------
    if (!a->plan_dev_known) {
        a->plan_dev.num_cus = (uint32_t)a->num_cus;
        a->plan_dev.lds_per_cu = a->lds_per_cu;
        for (uint32_t k = 0; k < bgr::kResidentKernels; ++k) a->plan_dev.resident[k] = bgr::resident_waves_per_cu(static_cast<bgr::KernelId>(k));
        a->plan_dev_known = true;
    }
    bgr::PlanBatch pb;
    pb.mode = p->mode; pb.max_mismatch = p->max_mismatch; pb.partial = p->partial; pb.max_read_len = max_read_len;
    pb.n_reads = n_reads; pb.total_bases = total_bases;
    const bgr::LaunchPlan P = bgr::plan_launch(plan_graph_of(a->graph->header), a->plan_dev, plan_tuning_of(a), pb);
    if (P.error) return fail(BGR_E_ARG, P.error);
    const bgr::Pass& first = P.pass[0];
    if (P.deep_scratch_bytes) HIP_TRY(a->deepbuf.ensure(P.deep_scratch_bytes));
    HIP_TRY(a->arena.ensure(P.arena_cap * 4));
    for (uint32_t i = 0; i < P.n_passes; ++i) {  // the lists the passes leave each other, and the rings of follow-up items of the sixteen-reads-per-wave kernel
        const bgr::Pass& ps = P.pass[i];
        if (ps.appends != bgr::List::kNone) HIP_TRY(list_buf(a, ps.appends)->ensure(n_reads * 4));
        if (ps.kernel == bgr::KernelId::kGreedyMulti) HIP_TRY(a->ovf.ensure((uint64_t)ps.cfg.blocks * ps.cfg.waves_per_block * P.q_cap * 8));
    }
    // (bgr_aligner_launch_info: the first pass; the level search ran unless every read went to the last pass)
    a->last_launch[0] = first.cfg.blocks; a->last_launch[1] = first.cfg.waves_per_block * 64; a->last_launch[2] = first.cfg.lds_bytes;
    a->last_launch[3] = first.cfg.stage_mphf | (P.level_search && first.kernel != bgr::KernelId::kExhaustiveLast ? 2u : 0u) | (bgr::many_reads_per_wave(first.kernel) ? 4u : 0u);

    // A launch handed ASCII reads maps them straight from the characters: the mapping kernels stage each read's 2-bit words themselves (round 5:
    // the pre-pass was 4-11 % of a launch and existed only to write 40 B per read that the next kernel read back).  BGR_KNOB_GREEDY_PREPASS 1 = the
    // pre-pass over the ASCII bytes and 2-bit planes as in rounds 2-4 (what bgr_align_batch_packed's host-packed planes still use)
    // (greedy and exhaustive mode: their several-reads-per-wave kernels stage their groups, the one-read-per-wave kernels go through load_packed.  Anchors
    // mode keeps the pre-pass: its four-reads-per-wave kernel -- BooPHF arithmetic at 96 VGPRs -- lost more inside than the pre-pass cost: 934 vs 965-1 000 Mreads/s)
    // ... and so do launches without a several-reads-per-wave pass (-i, budgets beyond 254, exception planes, the knobs): the one-read-per-wave kernels alone are
    // faster from planes (depth-first 11.8 vs 12.8 ms per 5 M reads, level search 14.0 vs 14.3 per 2 M)
    const bool inline_pack = (first.kernel == bgr::KernelId::kGreedyMulti || first.kernel == bgr::KernelId::kExhaustive4) && !planes_ready && d_reads && !a->knob_prepass;
    if (!reads_bytes) reads_bytes = total_bases;  // (reads end to end: the buffer holds exactly their bases)
    if (!inline_pack) {
        HIP_TRY(a->pk_fw3.ensure(P.plane_words * 8));
        HIP_TRY(a->pk_nm.ensure(P.plane_words * 8));
        HIP_TRY(a->pk_hasn.ensure((n_reads + 31) / 32 * 4 + 4));
    }
    bgr::BatchIO io{};  // what every pass shares; the loop below sets the rest
    io.ascii = inline_pack ? static_cast<const uint8_t*>(d_reads) : nullptr;
    io.ascii_src = inline_pack ? static_cast<const uint32_t*>(d_src_off) : nullptr;
    io.ascii_bytes = reads_bytes;
    io.fw3 = static_cast<const uint64_t*>(a->pk_fw3.p);
    io.nmw = static_cast<const uint64_t*>(a->pk_nm.p);
    io.hasn = static_cast<const uint32_t*>(a->pk_hasn.p);
    io.read_offs = static_cast<const uint64_t*>(d_read_offsets);
    io.results = static_cast<uint2*>(a->results.p);
    io.arena = static_cast<int32_t*>(a->arena.p);
    io.cursor = static_cast<uint32_t*>(a->small.p);
    io.n_reads = (uint32_t)n_reads;
    io.path_cap = P.path_cap;
    io.arena_cap = (uint32_t)P.arena_cap;
    io.arena_chunk = P.arena_chunk;
    io.arena_own = (uint32_t)P.arena_own;  // (< 2^32: plan_launch refuses a launch whose arena is larger)
    io.deep_stride = (uint32_t)P.deep_stride;
    io.deep_memo_cap = P.memo_cap;
    io.search_iters = P.search_iters;
    io.wide_scan = P.wide_scan ? 1u : 0u;
    io.task_ctr = bgr::kCurTasks;
    bgr::KernelParams kp = {p->max_mismatch, p->effort, p->partial, p->mode, a->knob_debug_stop};
    // the filter in front of a large key table pays where many read positions are probed per anchor (greedy scans: chr1-scale graph
    // 1 020 -> 1 184 Mreads/s, L2 requests per read 135 -> 28).  The exhaustive scan meets its first hit within a few positions; with
    // fingerprints behind it the filter cost it more than it saved (4-allele graph: 697 without, 664 with), with the bucket's keys compared
    // directly behind it, it pays there too (4-allele graph 702 -> 720, chr1-scale graph 1 111 -> 1 231): on by default for the minimizer
    // kind (option exh_filter = 0: without); the one-hash kind of short k stays off in exhaustive mode
    BgrDeviceGraph dgl = a->dg;
    if (p->mode == BGR_MODE_EXHAUSTIVE && !(dgl.filter_kind == BGR_FILTER_MINIMIZER && a->exh_filter)) dgl.bloom = nullptr;

    // the cursor block: arena cursor, overflow flag, list counts (the text form: the parse launch cleared it)
    if (!cursor_is_zero) HIP_TRY(hipMemsetAsync(a->small.p, 0, bgr::kCurWords * 4, a->stream));
    // HIP events on the aligner's stream: one in front of the launch, one behind every kernel of it (bgr_aligner_kernel_times)
    int marks = 0;
    // (timing a kernel is not free: the events make the runtime dispatch with completion stamps and keep the kernels of a launch apart -- three events around two
    // kernels cost a 262 144-read launch 16 of its 167 us, 1 730 -> 1 560 Mreads/s, and stamps taken by the dispatch packets themselves (hipExtLaunchKernelGGL)
    // cost the same, profiles/r05_mode_by_batch_size.txt; BGR_KNOB_KERNEL_EVENTS 0: none -- bgr_align_all without its timing option)
    const bool timed = !a->knob_no_events;
    auto mark = [&](const char* name) -> hipError_t {
        if (!timed || marks >= kTimerSlots) return hipSuccess;
        a->t_slot_name[marks] = name;
        return hipEventRecord(a->ev[a->ev_used][++marks], a->stream);
    };
    if (timed) HIP_TRY(hipEventRecord(a->ev[a->ev_used][0], a->stream));
    hipError_t e = hipSuccess;
    if (!planes_ready && !inline_pack) {
        HIP_TRY(hipMemsetAsync(a->pk_hasn.p, 0, (n_reads + 31) / 32 * 4, a->stream));
        e = d_src_off ? bgr::launch_pack_reads_at(static_cast<const uint8_t*>(d_reads), static_cast<const uint32_t*>(d_src_off), io.read_offs, io.n_reads, reads_bytes, total_bases,
                                                  static_cast<uint64_t*>(a->pk_fw3.p), static_cast<uint64_t*>(a->pk_nm.p), static_cast<uint32_t*>(a->pk_hasn.p), a->stream)
                      : bgr::launch_pack_reads(static_cast<const uint8_t*>(d_reads), io.read_offs, io.n_reads, total_bases, static_cast<uint64_t*>(a->pk_fw3.p),
                                               static_cast<uint64_t*>(a->pk_nm.p), static_cast<uint32_t*>(a->pk_hasn.p), a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("pre-pass launch: ") + hipGetErrorString(e));
        HIP_TRY(mark("bgr_pack_reads_kernel"));
    }
    // The passes, back to back on the stream.  A pass behind a list maps what an earlier pass listed; with an empty list its waves exit at once
    // (no host round trip in between).  The sixteen-reads-per-wave kernel works off the follow-up items of its reads (the next anchors of a read whose
    // first ones failed, then its reverse complement: alignerGreedy.cpp:41-56) in its own per-wave queues, inside the launch.
    for (uint32_t i = 0; i < P.n_passes; ++i) {
        const bgr::Pass& ps = P.pass[i];
        bgr::BatchIO pio = io;
        pio.words_per_read = ps.words;
        pio.frames_per_wave = ps.frames;
        pio.subset = ps.maps == bgr::List::kNone ? nullptr : static_cast<const uint32_t*>(list_buf(a, ps.maps)->p);
        pio.subset_ctr = bgr::list_word(ps.maps);
        uint32_t* appends = ps.appends == bgr::List::kNone ? nullptr : static_cast<uint32_t*>(list_buf(a, ps.appends)->p);
        if (ps.kernel == bgr::KernelId::kGreedyMulti) {
            pio.queue = static_cast<uint2*>(a->ovf.p);
            pio.q_cap = P.q_cap;
            pio.gen_list = appends;
            pio.gen_ctr = bgr::list_word(ps.appends);
        } else {
            pio.ovf_list = appends;
            pio.ovf_ctr = bgr::list_word(ps.appends);
        }
        if (ps.kernel == bgr::KernelId::kExhaustiveLast) pio.deep_scratch = static_cast<uint32_t*>(a->deepbuf.p);
#ifdef BGR_PHASE_TIMING
        if (ps.kernel == bgr::KernelId::kGreedyMulti || ps.kernel == bgr::KernelId::kExhaustive4) {  // time stamps per wave (the greedy kernel: then its scan counts)
            const uint64_t waves = (uint64_t)ps.cfg.blocks * ps.cfg.waves_per_block, bytes = waves * (ps.kernel == bgr::KernelId::kGreedyMulti ? 64 : 32);
            HIP_TRY(a->wave_times.ensure(bytes));
            if (ps.kernel == bgr::KernelId::kGreedyMulti) HIP_TRY(hipMemsetAsync(a->wave_times.p, 0, bytes, a->stream));  // (waves with no reads write nothing)
            pio.wave_times = static_cast<unsigned long long*>(a->wave_times.p);
            a->wave_times_n = waves;
        }
#endif
        e = bgr::launch_align(ps.kernel, ps.variant, dgl, pio, kp, ps.cfg, a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("kernel launch (") + ps.name + "): " + hipGetErrorString(e));
        HIP_TRY(mark(ps.name));
        if (ps.kernel == bgr::KernelId::kExhaustiveLast) {  // what settle_launch needs to run the last pass again for the reads it handed back
            a->deep.open = true;
            a->deep.pass = ps; a->deep.io = pio; a->deep.kp = kp; a->deep.dg = dgl;
            a->deep.per_wave_lds = bgr::deep_lds_bytes_per_wave(max_read_len);
            a->deep.path_cap = P.path_cap; a->deep.memo_cap = P.memo_cap;
            a->deep.runs = 1;
        }
    }
    // Unitig abundance (bgr_aligner_abundance_enable): one kernel behind the last pass adds this launch's rows to the aligner's table.  Every route
    // comes through here once per batch (a fetch into larger buffers after BGR_E_CAPACITY launches nothing), so nothing is counted twice.
    // (The kernel is queued before anybody knows how the launch ends: one that fails later -- an arena overflow, found when its cursors are read -- has
    // added the rows it did write.  include/bgreat_gpu.h says so: after a failed launch the table is undefined until bgr_aligner_reset_abundance.)
    if (a->abundance_on) {
        const uint64_t nu = a->graph->header.n_unitigs;
        const bgr::AbundancePlan ap = abundance_plan_of(a, n_reads, total_bases);
        e = bgr::launch_abundance(a->dg, nu, static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p), P.arena_cap, io.read_offs, io.n_reads,
                                  static_cast<unsigned long long*>(a->abundance.p), ap, a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("kernel launch (bgr_abundance_kernel): ") + hipGetErrorString(e));
        HIP_TRY(mark("bgr_abundance_kernel"));
    }
    // Links (bgr_aligner_links_enable): likewise one kernel that adds the consecutive pairs of this launch's rows to the aligner's hash table.
    if (a->links_on) {
        const bgr::LinksPlan lp = bgr::plan_links(a->links_bound, n_reads, (uint32_t)a->num_cus, a->knob_links_form);
        e = bgr::launch_links(a->graph->header.n_unitigs, static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p), P.arena_cap, io.n_reads, a->links_tab,
                              a->links_cap, lp, a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("kernel launch (bgr_links_kernel): ") + hipGetErrorString(e));
        HIP_TRY(mark("bgr_links_kernel"));
    }
    // Pileup (bgr_aligner_pileup_enable): likewise one kernel that adds per-base depth and mismatches.  It reads the read characters where this launch
    // has them: the ASCII bytes when the mapping kernels packed them themselves, else the 2-bit planes (host-packed, or made by the pre-pass).
    if (a->pileup_on) {
        bgr::PileupReads pr;
        if (inline_pack) { pr.ascii = static_cast<const uint8_t*>(d_reads); pr.src_off = static_cast<const uint32_t*>(d_src_off); pr.ascii_bytes = reads_bytes; }
        else { pr.fw3 = io.fw3; pr.nmw = io.nmw; pr.hasn = io.hasn; }
        e = bgr::launch_pileup(a->dg, a->graph->header.n_unitigs, a->graph->header.total_bases / 2, static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p),
                               P.arena_cap, io.read_offs, io.n_reads, pr, a->pileup_base_offs, a->pileup_tab, a->strands_on ? a->pileup_fwd_tab : nullptr, (uint32_t)a->num_cus, a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("kernel launch (bgr_pileup_kernel): ") + hipGetErrorString(e));
        HIP_TRY(mark("bgr_pileup_kernel"));
    }
    if (timed) {
        a->ev_marks[a->ev_used] = marks;
        ++a->ev_used;
    }
    return BGR_OK;
}

// Behind a mapping launch, with its stream waited for and the cursor block on the host (`cur`): the arena must not have overflowed, and in
// exhaustive mode the last pass may have handed reads back whose table of remembered calls filled up (exh_memo, exhaustive_kernels.hip):
// those run again -- the last pass only, over that list -- with a table sixteen times as large and as few waves as the list has reads, until
// none is left.  A search visits at most positions x halves x 2 nodes, so this ends; what can end it early is the device's memory.
static int settle_launch(bgr_aligner* a, uint32_t* cur) {
    if (cur[bgr::kCurOverflow]) return fail(BGR_E_INTERNAL, "path arena overflow (internal sizing error)");
    if (!a->deep.open) return BGR_OK;
    const uint32_t kRetry = bgr::list_word(bgr::List::kRetry);
    while (cur[kRetry]) {
        const uint32_t n_retry = cur[kRetry];
        auto& D = a->deep;
        if (D.runs >= bgr::kDeepRuns || D.memo_cap >= (1u << 28))
            return fail(BGR_E_NOMEM, "exhaustive search: a read's table of remembered calls outgrew 2^28 entries per wave (8 GiB)");
        D.memo_cap *= 16;
        const uint64_t stride = bgr::deep_scratch_words(D.path_cap, D.pass.frames, D.memo_cap);
        if (stride > 0xFFFFFFFFull) return fail(BGR_E_NOMEM, "exhaustive search: a read's table of remembered calls outgrew the 16 GiB a wave can address");
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const uint64_t room = (uint64_t)free_b + a->deepbuf.cap;
        uint64_t waves = std::min<uint64_t>(n_retry, (uint64_t)D.pass.cfg.blocks * D.pass.cfg.waves_per_block);
        waves = std::min<uint64_t>(waves, std::max<uint64_t>(1, room / 2 / (stride * 4)));
        if (stride * 4 > room - room / 8) return fail(BGR_E_NOMEM, "exhaustive search: not enough device memory for a read's table of remembered calls");
        HIP_TRY(a->deepbuf.ensure(waves * stride * 4));
        // the list handed back becomes the list to map; the kernel appends to the other one
        DevBuf& other = a->retry2;
        HIP_TRY(other.ensure((uint64_t)n_retry * 4));
        bgr::BatchIO io = D.io;
        io.subset = io.ovf_list;
        io.subset_ctr = bgr::kCurRetrySubset;
        io.ovf_list = static_cast<uint32_t*>(other.p);
        io.ovf_ctr = kRetry;
        io.deep_scratch = static_cast<uint32_t*>(a->deepbuf.p);
        io.deep_stride = (uint32_t)stride;
        io.deep_memo_cap = D.memo_cap;
        uint32_t ctr[2] = {0, n_retry};  // the count of the list handed back = 0, the count of the list to map (kCurRetrySubset, the word behind it) = n
        HIP_TRY(hipMemcpyAsync(static_cast<uint32_t*>(a->small.p) + kRetry, ctr, 8, hipMemcpyHostToDevice, a->stream));
        bgr::LaunchCfg cfg = D.pass.cfg;
        cfg.waves_per_block = (uint32_t)std::min<uint64_t>(cfg.waves_per_block, waves);
        cfg.blocks = (uint32_t)std::max<uint64_t>(1, waves / cfg.waves_per_block);
        cfg.lds_bytes = bgr::kLdsFixed + cfg.waves_per_block * D.per_wave_lds;
        hipError_t e = bgr::launch_align(D.pass.kernel, D.pass.variant, D.dg, io, D.kp, cfg, a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("kernel launch (last pass, run again): ") + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(cur, a->small.p, bgr::kCurWords * 4, hipMemcpyDeviceToHost, a->stream));
        HIP_TRY(wait_stream(a));
        if (cur[bgr::kCurOverflow]) return fail(BGR_E_INTERNAL, "path arena overflow (internal sizing error)");
        std::swap(a->retry, a->retry2);  // (D.io.ovf_list names the list the next round maps)
        D.io.ovf_list = io.ovf_list;
        ++D.runs;
    }
    a->deep.open = false;
    return BGR_OK;
}
// ... for callers that have not looked at the cursor yet (exhaustive launches only: nothing to settle otherwise but the arena flag, which every fetch checks)
static int settle_launch_sync(bgr_aligner* a) {
    if (!a->deep.open) return BGR_OK;
    uint32_t cur[bgr::kCurWords];
    HIP_TRY(hipMemcpyAsync(cur, a->small.p, sizeof(cur), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    return settle_launch(a, cur);
}

// ---- unitig abundance (bgr_run_options.abundance has the definition) ------------------------------------------------------------------
static int abundance_set(bgr_aligner* a, bool on) {
    if (on && !a->abundance.p) {
        HIP_TRY(hipSetDevice(a->device));
        HIP_TRY(a->abundance.ensure((a->graph->header.n_unitigs + 1) * sizeof(bgr_unitig_abundance)));
        HIP_TRY(hipMemsetAsync(a->abundance.p, 0, a->abundance.cap, a->stream));   // (on the aligner's own stream, as bgr_aligner_reset_counters)
        HIP_TRY(hipStreamSynchronize(a->stream));
        HIP_TRY(bgr::prepare_abundance(a->lds_per_cu));   // (once per aligner, not per launch: form B's tables beyond 48 KB)
    }
    a->abundance_on = on;
    return BGR_OK;
}

int bgr_aligner_abundance_enable(bgr_aligner* a, uint32_t on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_abundance_enable: null aligner");
    for (bgr_aligner* x = a; x; x = x->twin) { const int rc = abundance_set(x, on != 0); if (rc != BGR_OK) return rc; }
    return BGR_OK;
}

int bgr_aligner_abundance(bgr_aligner* a, bgr_unitig_abundance* out, uint64_t n_rows) {
    static_assert(sizeof(bgr_unitig_abundance) == 24, "three u64 per unitig, as the kernel adds them");
    if (!a || (n_rows && !out)) return fail(BGR_E_ARG, "bgr_aligner_abundance: null argument");
    if (n_rows != a->graph->header.n_unitigs) return fail(BGR_E_ARG, "bgr_aligner_abundance: n_rows is not the graph's number of unitigs");
    if (!a->abundance.p) return fail(BGR_E_ARG, "bgr_aligner_abundance: abundance was never enabled on this aligner (bgr_aligner_abundance_enable)");
    if (n_rows == 0) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    HIP_TRY(hipMemcpy(out, static_cast<const bgr_unitig_abundance*>(a->abundance.p) + 1, n_rows * sizeof(bgr_unitig_abundance), hipMemcpyDeviceToHost));
    std::vector<bgr_unitig_abundance> t;
    for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) {  // the pieces of overlapped batches its other streams mapped
        if (!tw->abundance.p) continue;
        t.resize(n_rows);
        HIP_TRY(hipStreamSynchronize(tw->stream));
        HIP_TRY(hipMemcpy(t.data(), static_cast<const bgr_unitig_abundance*>(tw->abundance.p) + 1, n_rows * sizeof(bgr_unitig_abundance), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n_rows; ++i) { out[i].reads += t[i].reads; out[i].bases += t[i].bases; out[i].kmers += t[i].kmers; }
    }
    return BGR_OK;
}

int bgr_aligner_abundance_plan(bgr_aligner* a, uint64_t n_reads, uint64_t total_bases, uint32_t out[4]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_abundance_plan: null argument");
    const bgr::AbundancePlan ap = abundance_plan_of(a, n_reads, total_bases);
    out[0] = ap.form; out[1] = ap.blocks; out[2] = ap.threads; out[3] = ap.lds_bytes;
    return BGR_OK;
}

int bgr_plan_abundance(uint64_t n_unitigs, uint32_t k, uint64_t n_reads, uint64_t total_bases, uint32_t num_cus, uint64_t lds_per_cu, uint32_t form_knob, uint32_t out[4]) {
    if (!out || form_knob > 2) return fail(BGR_E_ARG, "bgr_plan_abundance: null argument or a form beyond 2");
    const bgr::AbundancePlan ap = bgr::plan_abundance(n_unitigs, k, n_reads, total_bases, num_cus, lds_per_cu, form_knob);
    out[0] = ap.form; out[1] = ap.blocks; out[2] = ap.threads; out[3] = ap.lds_bytes;
    return BGR_OK;
}

int bgr_aligner_reset_abundance(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_reset_abundance: null aligner");
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) {
        if (!x->abundance.p) continue;
        HIP_TRY(hipMemsetAsync(x->abundance.p, 0, x->abundance.cap, x->stream));
        HIP_TRY(hipStreamSynchronize(x->stream));
    }
    return BGR_OK;
}

// what a whole run calls (run_abundance.h)
static int run_abundance_enable(bgr_aligner* a) { return bgr_aligner_abundance_enable(a, 1); }
static int run_abundance_collect(bgr_graph* g, bgr_aligner* a) {
    std::vector<bgr_unitig_abundance> rows(g->header.n_unitigs);
    const int rc = bgr_aligner_abundance(a, rows.data(), rows.size());
    if (rc == BGR_OK) graph_abundance_add(g, rows.data(), rows.size());
    return rc;
}
static const bool g_run_abundance_registered = (bgr::g_run_abundance = bgr::RunAbundance{graph_abundance_begin, run_abundance_enable, run_abundance_collect, graph_abundance_end}, true);

int bgr_graph_abundance(const bgr_graph* g, bgr_unitig_abundance* out, uint64_t n_rows) {
    if (!g || (n_rows && !out)) return fail(BGR_E_ARG, "bgr_graph_abundance: null argument");
    if (!g->abundance_valid) return fail(BGR_E_ARG, "bgr_graph_abundance: no totals -- they are those of the last successful bgr_align_all with bgr_run_options.abundance = 1");
    if (n_rows != g->header.n_unitigs) return fail(BGR_E_ARG, "bgr_graph_abundance: n_rows is not the graph's number of unitigs");
    if (n_rows) memcpy(out, g->abundance.data(), n_rows * sizeof(bgr_unitig_abundance));
    return BGR_OK;
}

int bgr_write_abundance(const char* path, const bgr_graph* g, const bgr_unitig_abundance* rows, uint64_t n_rows) {
    if (!path || !g || (n_rows && !rows)) return fail(BGR_E_ARG, "bgr_write_abundance: null argument");
    if (n_rows != g->header.n_unitigs) return fail(BGR_E_ARG, "bgr_write_abundance: n_rows is not the graph's number of unitigs");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_write_abundance: the graph has no host blob (the unitig lengths are read from it)");
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string("bgr_write_abundance: cannot open ") + path);
    std::string buf = "#unitig\tlength\treads\tbases\tkmers\n";
    bool ok = true;
    for (uint64_t i = 0; i < n_rows && ok; ++i) {
        buf += std::to_string(i + 1); buf += '\t';
        buf += std::to_string(meta[i + 1].len); buf += '\t';
        buf += std::to_string(rows[i].reads); buf += '\t';
        buf += std::to_string(rows[i].bases); buf += '\t';
        buf += std::to_string(rows[i].kmers); buf += '\n';
        if (buf.size() > (1u << 20)) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); }
    }
    if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string("bgr_write_abundance: write to ") + path + " failed");
    return BGR_OK;
}


// ---- pileup (bgr_pileup_base in include/bgreat_gpu.h has the definition) -------------------------------------------------------------------
static int graph_base_offs(bgr_graph* g, const char* who) {   // prefix sums of the unitig lengths, once per graph
    if (g->host.blob.empty()) return fail(BGR_E_ARG, std::string(who) + ": the graph has no host blob (the unitig lengths and characters are read from it)");
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (g->base_offs.empty()) {
        const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
        std::vector<uint64_t> o(g->header.n_unitigs + 2, 0);
        for (uint64_t i = 1; i <= g->header.n_unitigs; ++i) o[i + 1] = o[i] + meta[i].len;
        g->base_offs.swap(o);
    }
    return BGR_OK;
}
static int pileup_refusal(const bgr_graph* g, const char* who) {
    if (g->header.has_exc)
        return fail(BGR_E_ARG, std::string(who) + ": the pileup (--pileup, --depth) needs a graph of ACGT-only unitigs: on one with other characters the 2-bit store does not spell them and a path read backwards does not spell the reverse complement");
    return BGR_OK;
}
static void pileup_share(bgr_aligner* a) {   // the twins add to the aligner's table
    for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) {
        tw->pileup_tab = a->pileup_tab; tw->pileup_base_offs = a->pileup_base_offs; tw->pileup_on = a->pileup_on;
        tw->pileup_fwd_tab = a->pileup_fwd_tab; tw->strands_on = a->strands_on;
    }
}

int bgr_aligner_pileup_enable(bgr_aligner* a, uint32_t on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_pileup_enable: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_pileup_enable: an internal stream of another aligner");
    if (on) {
        int rc = pileup_refusal(a->graph, "bgr_aligner_pileup_enable");
        if (rc == BGR_OK) rc = graph_base_offs(a->graph, "bgr_aligner_pileup_enable");
        if (rc == BGR_OK) rc = bgr_aligner_abundance_enable(a, 1);   // (its reads column bounds every depth: bgr_aligner_pileup checks it)
        if (rc != BGR_OK) return rc;
    }
    if (on && !a->pileup_tab) {
        const uint64_t n = a->graph->header.n_unitigs, T = a->graph->header.total_bases / 2, bytes = bgr::pileup_table_bytes(T, n);
        HIP_TRY(hipSetDevice(a->device));
        hipError_t e = a->pileup.ensure(bytes);
        if (e == hipSuccess) e = a->pileup_offs.ensure((n + 2) * 8);
        if (e != hipSuccess) {
            a->pileup.release(); a->pileup_offs.release();
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, "bgr_aligner_pileup_enable: " + std::to_string(bytes) + " bytes for the pileup table (20 per base of the graph): " + hipGetErrorString(e));
        }
        HIP_TRY(hipMemsetAsync(a->pileup.p, 0, bytes, a->stream));   // (on the aligner's own stream, as bgr_aligner_reset_counters)
        HIP_TRY(hipMemcpyAsync(a->pileup_offs.p, a->graph->base_offs.data(), (n + 2) * 8, hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipStreamSynchronize(a->stream));
        a->pileup_tab = static_cast<uint32_t*>(a->pileup.p);
        a->pileup_base_offs = static_cast<const uint64_t*>(a->pileup_offs.p);
    }
    a->pileup_on = on != 0;
    pileup_share(a);
    return BGR_OK;
}

int bgr_aligner_pileup_strands_enable(bgr_aligner* a, uint32_t on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_pileup_strands_enable: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_pileup_strands_enable: an internal stream of another aligner");
    bool fresh = false;
    if (on && !a->pileup_fwd_tab) {   // the second table first: a refusal leaves the aligner as it was
        const int rc0 = pileup_refusal(a->graph, "bgr_aligner_pileup_strands_enable");
        if (rc0 != BGR_OK) return rc0;
        const uint64_t n = a->graph->header.n_unitigs, T = a->graph->header.total_bases / 2, bytes = bgr::pileup_table_bytes(T, n);
        HIP_TRY(hipSetDevice(a->device));
        const hipError_t e = a->pileup_fwd.ensure(bytes);
        if (e != hipSuccess) {
            a->pileup_fwd.release();
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, "bgr_aligner_pileup_strands_enable: " + std::to_string(bytes) + " bytes for the forward pileup table (20 more per base of the graph): " + hipGetErrorString(e));
        }
        HIP_TRY(hipMemsetAsync(a->pileup_fwd.p, 0, bytes, a->stream));
        HIP_TRY(hipStreamSynchronize(a->stream));
        a->pileup_fwd_tab = static_cast<uint32_t*>(a->pileup_fwd.p);
        fresh = true;
    }
    if (on) {
        const int rc = bgr_aligner_pileup_enable(a, 1);   // (as the pileup enables abundance)
        if (rc != BGR_OK) {
            if (fresh) { a->pileup_fwd.release(); a->pileup_fwd_tab = nullptr; }   // (nothing stays allocated behind a refusal)
            return rc;
        }
    }
    a->strands_on = on != 0;
    pileup_share(a);
    return BGR_OK;
}

// alt / delta words -> rows: the depth is the running sum of a unitig's delta words, N lies in the alt word of the unitig's own base
static void pileup_unitig_rows(const bgr_graph* g, const uint32_t* words, uint64_t id, bgr_pileup_base* out) {   // the len rows of one unitig
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
    const uint64_t* seq = reinterpret_cast<const uint64_t*>(g->host.base() + g->header.off_seq);
    const uint32_t* alt = words;
    const uint32_t* delta = words + bgr::pileup_alt_words(g->header.total_bases / 2);
    const uint64_t b0 = g->base_offs[id], d0 = b0 + id - 1, F = meta[id].F;
    uint32_t depth = 0;
    for (uint64_t pos = 0; pos < meta[id].len; ++pos) {
        depth += delta[d0 + pos];   // (mod 2^32)
        const uint64_t p = F + pos;
        const uint32_t ref = (uint32_t)(seq[p >> 5] >> (62 - 2 * (p & 31))) & 3u;
        const uint32_t* w = alt + 4 * (b0 + pos);
        uint32_t c[4] = {w[0], w[1], w[2], w[3]};
        c[ref] = 0;   // (nothing that differs from the base has the base's code: that word counted the Ns)
        out[pos] = bgr_pileup_base{depth, c[0], c[1], c[2], c[3], w[ref]};
    }
}
static void pileup_rows(const bgr_graph* g, const uint32_t* words, bgr_pileup_base* out) {
    for (uint64_t id = 1; id <= g->header.n_unitigs; ++id) pileup_unitig_rows(g, words, id, out + g->base_offs[id]);
}
// this aligner's reads column may not have reached 2^32 anywhere: it bounds every depth on the unitig, and a depth is kept mod 2^32
static int pileup_guard(const bgr_unitig_abundance* rows, uint64_t n, const char* who) {
    for (uint64_t i = 0; i < n; ++i)
        if (rows[i].reads >> 32)
            return fail(BGR_E_CAPACITY, std::string(who) + ": unitig " + std::to_string(i + 1) + " lies on " + std::to_string(rows[i].reads) + " reads' paths: a per-base depth (32 bits) may have wrapped; no pileup is delivered");
    return BGR_OK;
}
// the aligner's table on the host (every stream that adds to it waited for), behind the guard
static int pileup_snapshot(bgr_aligner* a, const char* who, std::vector<uint32_t>& words, uint64_t* skipped, bool fwd = false) {
    if (fwd && !a->pileup_fwd_tab) return fail(BGR_E_ARG, std::string(who) + ": strands were never counted on this aligner (bgr_aligner_pileup_strands_enable)");
    if (!a->pileup_tab) return fail(BGR_E_ARG, std::string(who) + ": the pileup was never enabled on this aligner (bgr_aligner_pileup_enable)");
    const uint64_t n = a->graph->header.n_unitigs, T = a->graph->header.total_bases / 2;
    std::vector<bgr_unitig_abundance> ab(n);
    int rc = bgr_aligner_abundance(a, ab.data(), n);   // (synchronises the aligner's stream and its twins')
    if (rc == BGR_OK) rc = pileup_guard(ab.data(), n, who);
    if (rc != BGR_OK) return rc;
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) HIP_TRY(hipStreamSynchronize(x->stream));
    words.resize(bgr::pileup_alt_words(T) + bgr::pileup_delta_words(T, n));
    const uint32_t* tab = fwd ? a->pileup_fwd_tab : a->pileup_tab;
    if (!words.empty()) HIP_TRY(hipMemcpy(words.data(), tab, words.size() * 4, hipMemcpyDeviceToHost));
    unsigned long long sk = 0;
    HIP_TRY(hipMemcpy(&sk, reinterpret_cast<const char*>(tab) + bgr::pileup_tail_byte(T, n), 8, hipMemcpyDeviceToHost));
    *skipped = sk;
    return BGR_OK;
}

int bgr_aligner_pileup(bgr_aligner* a, bgr_pileup_base* out, uint64_t n_bases, uint64_t* skipped) {
    static_assert(sizeof(bgr_pileup_base) == 24, "six u32 per base");
    if (!a || (n_bases && !out)) return fail(BGR_E_ARG, "bgr_aligner_pileup: null argument");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_pileup: an internal stream of another aligner");
    if (n_bases != a->graph->header.total_bases / 2) return fail(BGR_E_ARG, "bgr_aligner_pileup: n_bases is not the sum of the graph's unitig lengths");
    std::vector<uint32_t> words;
    uint64_t sk = 0;
    const int rc = pileup_snapshot(a, "bgr_aligner_pileup", words, &sk);
    if (rc != BGR_OK) return rc;
    pileup_rows(a->graph, words.data(), out);
    if (skipped) *skipped = sk;
    return BGR_OK;
}

int bgr_aligner_pileup_forward(bgr_aligner* a, bgr_pileup_base* out, uint64_t n_bases) {
    if (!a || (n_bases && !out)) return fail(BGR_E_ARG, "bgr_aligner_pileup_forward: null argument");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_pileup_forward: an internal stream of another aligner");
    if (n_bases != a->graph->header.total_bases / 2) return fail(BGR_E_ARG, "bgr_aligner_pileup_forward: n_bases is not the sum of the graph's unitig lengths");
    std::vector<uint32_t> words;
    uint64_t sk = 0;
    const int rc = pileup_snapshot(a, "bgr_aligner_pileup_forward", words, &sk, true);
    if (rc != BGR_OK) return rc;
    pileup_rows(a->graph, words.data(), out);
    return BGR_OK;
}

int bgr_aligner_reset_pileup(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_reset_pileup: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_reset_pileup: an internal stream of another aligner");
    if (!a->pileup.p) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemsetAsync(a->pileup.p, 0, bgr::pileup_table_bytes(a->graph->header.total_bases / 2, a->graph->header.n_unitigs), a->stream));
    if (a->pileup_fwd.p) HIP_TRY(hipMemsetAsync(a->pileup_fwd.p, 0, bgr::pileup_table_bytes(a->graph->header.total_bases / 2, a->graph->header.n_unitigs), a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return BGR_OK;   // (the abundance table stays: the guard's column then counts more launches than the pileup holds, which errs on the safe side)
}

// what a whole run calls (run_pileup.h): the graph's pileup switch gathers the tables on the host, its variants switch (further down) on a device
static int variants_collect(bgr_graph* g, bgr_aligner* a);
static int variants_end(bgr_graph* g, bool ok);
static bool run_pileup_wanted(const bgr_graph* g) { return g && (g->pileup_on || g->variants_on); }
static bool run_pileup_variants(const bgr_graph* g) { return g && g->variants_on; }
static bool run_pileup_strands(const bgr_graph* g) { return g && ((g->pileup_on && g->pileup_strands_on) || (g->variants_on && g->variants_strands_on)); }
static void run_pileup_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (g->pileup_on) {
        g->pileup_words.clear();
        g->pileup_skipped = 0;
        g->pileup_valid = false;
        g->pileup_fwd_words.clear();
        g->pileup_fwd_valid = false;
    }
    if (g->variants_on) {
        variants_run_free(g);
        g->variants_sites.clear();
        g->variants_valid = false;
        g->variants_strand_sites.clear();
        g->variants_strands_valid = false;
    }
}
static int run_pileup_enable(bgr_aligner* a) { return bgr_aligner_pileup_enable(a, 1); }
static int run_pileup_enable_strands(bgr_aligner* a) { return bgr_aligner_pileup_strands_enable(a, 1); }
static int run_pileup_collect(bgr_graph* g, bgr_aligner* a) {
    if (g->pileup_on) {
        std::vector<uint32_t> words;
        uint64_t sk = 0;
        const int rc = pileup_snapshot(a, "bgr_align_all", words, &sk);
        if (rc != BGR_OK) return rc;
        std::lock_guard<std::mutex> l(g->abundance_m);
        if (g->pileup_words.empty()) g->pileup_words.swap(words);
        else for (size_t i = 0; i < words.size(); ++i) g->pileup_words[i] += words[i];   // (mod 2^32: the delta sums commute)
        g->pileup_skipped += sk;
    }
    if (g->pileup_on && g->pileup_strands_on) {   // the forward table likewise (its tail is 0)
        std::vector<uint32_t> words;
        uint64_t sk = 0;
        const int rc = pileup_snapshot(a, "bgr_align_all", words, &sk, true);
        if (rc != BGR_OK) return rc;
        std::lock_guard<std::mutex> l(g->abundance_m);
        if (g->pileup_fwd_words.empty()) g->pileup_fwd_words.swap(words);
        else for (size_t i = 0; i < words.size(); ++i) g->pileup_fwd_words[i] += words[i];
    }
    return g->variants_on ? variants_collect(g, a) : BGR_OK;   // (behind the snapshot: the first aligner's table leaves it here)
}
static int run_pileup_end(bgr_graph* g, bool ok) {   // behind the abundance's end: the summed reads column guards the summed table
    int rc = BGR_OK;
    if (g->pileup_on) {
        std::lock_guard<std::mutex> l(g->abundance_m);
        if (ok) {
            const uint64_t T = g->header.total_bases / 2, n = g->header.n_unitigs;
            if (g->pileup_words.empty()) g->pileup_words.assign(bgr::pileup_alt_words(T) + bgr::pileup_delta_words(T, n), 0u);   // (a run without aligners' tables: nothing mapped)
            rc = g->abundance_valid ? pileup_guard(g->abundance.data(), g->abundance.size(), "bgr_align_all") : fail(BGR_E_INTERNAL, "bgr_align_all: a pileup without the abundance totals that guard it");
        }
        if (!ok || rc != BGR_OK) { g->pileup_words.clear(); g->pileup_words.shrink_to_fit(); }
        g->pileup_valid = ok && rc == BGR_OK;
        if (g->pileup_strands_on && g->pileup_valid && g->pileup_fwd_words.empty()) g->pileup_fwd_words.assign(g->pileup_words.size(), 0u);
        if (!g->pileup_strands_on || !g->pileup_valid) { g->pileup_fwd_words.clear(); g->pileup_fwd_words.shrink_to_fit(); }
        g->pileup_fwd_valid = g->pileup_strands_on && g->pileup_valid;
    }
    if (g->variants_on) {
        const int vrc = variants_end(g, ok && rc == BGR_OK);
        if (rc == BGR_OK) rc = vrc;
    }
    return rc;
}
static const bool g_run_pileup_registered = (bgr::g_run_pileup = bgr::RunPileup{run_pileup_wanted, run_pileup_begin, run_pileup_enable, run_pileup_collect, run_pileup_end, run_pileup_variants, run_pileup_strands, run_pileup_enable_strands}, true);

int bgr_graph_pileup_enable(bgr_graph* g, uint32_t on) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_pileup_enable: null graph");
    if (on) {
        int rc = pileup_refusal(g, "bgr_graph_pileup_enable");
        if (rc == BGR_OK) rc = graph_base_offs(g, "bgr_graph_pileup_enable");
        if (rc != BGR_OK) return rc;
    }
    g->pileup_on = on != 0;
    return BGR_OK;
}

int bgr_graph_pileup_enabled(const bgr_graph* g) { return g && g->pileup_on ? 1 : 0; }

int bgr_graph_pileup_strands_enable(bgr_graph* g, uint32_t on) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_pileup_strands_enable: null graph");
    if (on) {
        const int rc = bgr_graph_pileup_enable(g, 1);   // (as the aligner's switch enables the aligner's pileup)
        if (rc != BGR_OK) return rc;
    }
    g->pileup_strands_on = on != 0;
    return BGR_OK;
}

int bgr_graph_pileup_strands_enabled(const bgr_graph* g) { return g && g->pileup_strands_on ? 1 : 0; }

static int graph_pileup_check(const bgr_graph* g, const char* who) {
    if (!g->pileup_valid) return fail(BGR_E_ARG, std::string(who) + ": no totals -- they are those of the last successful bgr_align_all with bgr_graph_pileup_enable on");
    return BGR_OK;
}

int bgr_graph_pileup(const bgr_graph* g, bgr_pileup_base* out, uint64_t n_bases, uint64_t* skipped) {
    if (!g || (n_bases && !out)) return fail(BGR_E_ARG, "bgr_graph_pileup: null argument");
    const int rc = graph_pileup_check(g, "bgr_graph_pileup");
    if (rc != BGR_OK) return rc;
    if (n_bases != g->header.total_bases / 2) return fail(BGR_E_ARG, "bgr_graph_pileup: n_bases is not the sum of the graph's unitig lengths");
    pileup_rows(g, g->pileup_words.data(), out);
    if (skipped) *skipped = g->pileup_skipped;
    return BGR_OK;
}

static int graph_pileup_fwd_check(const bgr_graph* g, const char* who) {
    if (!g->pileup_valid || !g->pileup_fwd_valid)
        return fail(BGR_E_ARG, std::string(who) + ": no forward totals -- they are those of the last successful bgr_align_all with bgr_graph_pileup_strands_enable on");
    return BGR_OK;
}

int bgr_graph_pileup_forward(const bgr_graph* g, bgr_pileup_base* out, uint64_t n_bases) {
    if (!g || (n_bases && !out)) return fail(BGR_E_ARG, "bgr_graph_pileup_forward: null argument");
    const int rc = graph_pileup_fwd_check(g, "bgr_graph_pileup_forward");
    if (rc != BGR_OK) return rc;
    if (n_bases != g->header.total_bases / 2) return fail(BGR_E_ARG, "bgr_graph_pileup_forward: n_bases is not the sum of the graph's unitig lengths");
    pileup_rows(g, g->pileup_fwd_words.data(), out);
    return BGR_OK;
}

// the writers: host code, deterministic bytes, straight from the graph's totals
static int pileup_write(const char* path, const bgr_graph* g, bool sites, const char* who, bool strands = false) {
    if (!path || !g) return fail(BGR_E_ARG, std::string(who) + ": null argument");
    const int rc = strands ? graph_pileup_fwd_check(g, who) : graph_pileup_check(g, who);
    if (rc != BGR_OK) return rc;
    std::vector<bgr_pileup_base> frows(strands ? g->header.max_unitig_len + 1 : 0);
    const uint64_t n = g->header.n_unitigs;
    std::vector<bgr_pileup_base> rows(g->header.max_unitig_len + 1);   // (converted unitig by unitig: no second table on the host)
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
    const uint64_t* seq = reinterpret_cast<const uint64_t*>(g->host.base() + g->header.off_seq);
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string(who) + ": cannot open " + path);
    std::string buf = strands ? "#unitig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tdepth+\tA+\tC+\tG+\tT+\tN+\n" : sites ? "#unitig\tpos\tref\tdepth\tA\tC\tG\tT\tN\n" : "";
    bool ok = true;
    auto flush = [&](bool all) { if (ok && !buf.empty() && (all || buf.size() > (1u << 20))) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); } };
    for (uint64_t id = 1; id <= n && ok; ++id) {
        const uint64_t len = meta[id].len;
        if (len > rows.size()) rows.resize(len);
        pileup_unitig_rows(g, g->pileup_words.data(), id, rows.data());
        if (strands) {
            if (len > frows.size()) frows.resize(len);
            pileup_unitig_rows(g, g->pileup_fwd_words.data(), id, frows.data());
        }
        const bgr_pileup_base* r = rows.data();
        if (sites) {
            for (uint64_t pos = 0; pos < len; ++pos) {
                const bgr_pileup_base& b = r[pos];
                if (!(b.depth | b.a | b.c | b.g | b.t | b.n)) continue;
                const uint64_t p = meta[id].F + pos;
                buf += std::to_string(id); buf += '\t'; buf += std::to_string(pos); buf += '\t';
                buf += "ACGT"[(seq[p >> 5] >> (62 - 2 * (p & 31))) & 3u];
                for (const uint32_t v : {b.depth, b.a, b.c, b.g, b.t, b.n}) { buf += '\t'; buf += std::to_string(v); }
                if (strands) { const bgr_pileup_base& fb = frows[pos]; for (const uint32_t v : {fb.depth, fb.a, fb.c, fb.g, fb.t, fb.n}) { buf += '\t'; buf += std::to_string(v); } }
                buf += '\n';
            }
        } else {
            for (uint64_t pos = 0; pos < len;) {   // maximal runs of equal non-zero depth
                uint64_t e = pos + 1;
                while (e < len && r[e].depth == r[pos].depth) ++e;
                if (r[pos].depth) { buf += std::to_string(id); buf += '\t'; buf += std::to_string(pos); buf += '\t'; buf += std::to_string(e); buf += '\t'; buf += std::to_string(r[pos].depth); buf += '\n'; }
                pos = e;
            }
        }
        flush(false);
    }
    flush(true);
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string(who) + ": write to " + path + " failed");
    return BGR_OK;
}
int bgr_write_pileup(const char* path, const bgr_graph* g) { return pileup_write(path, g, true, "bgr_write_pileup"); }
int bgr_write_depth(const char* path, const bgr_graph* g) { return pileup_write(path, g, false, "bgr_write_depth"); }
int bgr_write_pileup_strands(const char* path, const bgr_graph* g) { return pileup_write(path, g, true, "bgr_write_pileup_strands", true); }


// ---- SNV sites (bgr_variant_site in include/bgreat_gpu.h has the definition; variants_kernels.h the passes) -------------------------------------
// the five launches over one table on `stream` of the current device, then the records' way to the host: into `vec` (as many as there are), or into
// `out` when they are at most `cap`.  *n = their number in any case.  ms: null, or the five launches' milliseconds
static int variants_call(const BgrDeviceGraph& dg, const bgr_graph* g, const uint32_t* table, const uint64_t* base_offs, const bgr_variant_params& prm, DevBuf& scratch,
                         DevBuf& outbuf, hipStream_t stream, const char* who, std::vector<bgr_variant_site>* vec, bgr_variant_site* out, uint64_t cap, uint64_t* n, double* ms) {
    static_assert(sizeof(bgr_variant_site) == 32, "eight u32 per site");
    const uint64_t nu = g->header.n_unitigs, T = g->header.total_bases / 2, tiles = bgr::variants_tiles(T, nu);
    *n = 0;
    if (ms) for (int i = 0; i < 5; ++i) ms[i] = 0;
    if (vec) vec->clear();
    if (tiles == 0 || nu == 0) return BGR_OK;
    hipError_t e = scratch.ensure(bgr::variants_scratch_bytes(tiles));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": the passes' tile arrays: " + hipGetErrorString(e)); }
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 6; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } guard{ev};
    if (ms) {
        for (int i = 0; i < 6; ++i) HIP_TRY(hipEventCreate(&ev[i]));
        HIP_TRY(hipEventRecord(ev[0], stream));
    }
    e = bgr::launch_variants_count(dg, nu, T, table, base_offs, prm, scratch.p, stream, ms ? ev + 1 : nullptr);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_variants_*_kernel): " + hipGetErrorString(e));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, bgr::variants_total_word(scratch.p, tiles), 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *n = total;
    if (total > T) return fail(BGR_E_INTERNAL, std::string(who) + ": more sites than bases");
    if (!vec && total > cap) return fail(BGR_E_CAPACITY, std::string(who) + ": " + std::to_string(total) + " sites, room for " + std::to_string(cap));
    if (total) {
        e = outbuf.ensure(total * sizeof(bgr_variant_site));
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": " + std::to_string(total) + " site records on the device: " + hipGetErrorString(e)); }
        e = bgr::launch_variants_emit(dg, nu, T, table, base_offs, prm, scratch.p, static_cast<bgr_variant_site*>(outbuf.p), stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_variants_classify_kernel, emit): " + hipGetErrorString(e));
        if (ms) HIP_TRY(hipEventRecord(ev[5], stream));
        if (vec) { vec->resize(total); out = vec->data(); }
        HIP_TRY(hipMemcpyAsync(out, outbuf.p, total * sizeof(bgr_variant_site), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    if (ms)
        for (int i = 0; i < (total ? 5 : 4); ++i) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, ev[i], ev[i + 1])); ms[i] = f; }
    return BGR_OK;
}

// the same with the forward table next to the total one: 64-byte records under the strand filter
static int variants_strands_call(const BgrDeviceGraph& dg, const bgr_graph* g, const uint32_t* table, const uint32_t* table_fwd, const uint64_t* base_offs, const bgr_variant_strand_params& prm,
                                 DevBuf& scratch, DevBuf& outbuf, hipStream_t stream, const char* who, std::vector<bgr_variant_strand_site>* vec, bgr_variant_strand_site* out, uint64_t cap,
                                 uint64_t* n, double* ms) {
    static_assert(sizeof(bgr_variant_strand_site) == 64, "sixteen u32 per site");
    const uint64_t nu = g->header.n_unitigs, T = g->header.total_bases / 2, tiles = bgr::variants_tiles(T, nu);
    *n = 0;
    if (ms) for (int i = 0; i < 5; ++i) ms[i] = 0;
    if (vec) vec->clear();
    if (tiles == 0 || nu == 0) return BGR_OK;
    hipError_t e = scratch.ensure(bgr::variants_strands_scratch_bytes(tiles));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": the passes' tile arrays: " + hipGetErrorString(e)); }
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 6; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } guard{ev};
    if (ms) {
        for (int i = 0; i < 6; ++i) HIP_TRY(hipEventCreate(&ev[i]));
        HIP_TRY(hipEventRecord(ev[0], stream));
    }
    e = bgr::launch_variants_strands_count(dg, nu, T, table, table_fwd, base_offs, prm, scratch.p, stream, ms ? ev + 1 : nullptr);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_variants_*_kernel, strands): " + hipGetErrorString(e));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, bgr::variants_total_word(scratch.p, tiles), 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *n = total;
    if (total > T) return fail(BGR_E_INTERNAL, std::string(who) + ": more sites than bases");
    if (!vec && total > cap) return fail(BGR_E_CAPACITY, std::string(who) + ": " + std::to_string(total) + " sites, room for " + std::to_string(cap));
    if (total) {
        e = outbuf.ensure(total * sizeof(bgr_variant_strand_site));
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": " + std::to_string(total) + " site records on the device: " + hipGetErrorString(e)); }
        e = bgr::launch_variants_strands_emit(dg, nu, T, table, table_fwd, base_offs, prm, scratch.p, static_cast<bgr_variant_strand_site*>(outbuf.p), stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_variants_classify_kernel, strands, emit): " + hipGetErrorString(e));
        if (ms) HIP_TRY(hipEventRecord(ev[5], stream));
        if (vec) { vec->resize(total); out = vec->data(); }
        HIP_TRY(hipMemcpyAsync(out, outbuf.p, total * sizeof(bgr_variant_strand_site), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    if (ms)
        for (int i = 0; i < (total ? 5 : 4); ++i) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, ev[i], ev[i + 1])); ms[i] = f; }
    return BGR_OK;
}

// dst += src, two whole pileup tables of `bytes` bytes; the current device is dst's, `stream` one of its streams, waited for before the return.
// On one device one kernel; across devices -- or whenever the test hook names a piece size -- through `stage`, a piece of at most 64 MiB at a time
static int variants_table_add(uint32_t* dst, int dst_device, const uint32_t* src, int src_device, uint64_t bytes, DevBuf& stage, uint32_t num_cus, hipStream_t stream, const char* who) {
    const int64_t hook = bgr::opt("test.variants_stage_bytes");
    hipError_t e;
    if (dst_device == src_device && hook == 0) {
        e = bgr::launch_pileup_add(dst, src, bytes / 4, true, num_cus, stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_pileup_add_kernel): " + hipGetErrorString(e));
    } else {
        uint64_t piece = hook > 0 ? ((uint64_t)hook + 15) / 16 * 16 : (64ull << 20);
        if (piece > (64ull << 20)) piece = 64ull << 20;
        if (piece > bytes) piece = (bytes + 15) / 16 * 16;
        e = stage.ensure(piece);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": the staging piece of a table from another device: " + hipGetErrorString(e)); }
        for (uint64_t off = 0; off < bytes; off += piece) {   // (the pieces follow each other on one stream: the copy of the next waits for the add of this one)
            const uint64_t len = bytes - off < piece ? bytes - off : piece;
            if (dst_device == src_device) HIP_TRY(hipMemcpyAsync(stage.p, reinterpret_cast<const char*>(src) + off, len, hipMemcpyDeviceToDevice, stream));
            else HIP_TRY(hipMemcpyPeerAsync(stage.p, dst_device, reinterpret_cast<const char*>(src) + off, src_device, len, stream));
            e = bgr::launch_pileup_add(dst + off / 4, static_cast<const uint32_t*>(stage.p), len / 4, off + len == bytes, num_cus, stream);
            if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_pileup_add_kernel): " + hipGetErrorString(e));
        }
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return BGR_OK;
}

int bgr_aligner_pileup_sites(bgr_aligner* a, const bgr_variant_params* params, bgr_variant_site* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!a || !params || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_aligner_pileup_sites: null argument");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_pileup_sites: an internal stream of another aligner");
    if (!bgr::variants_params_ok(*params)) return fail(BGR_E_ARG, "bgr_aligner_pileup_sites: thresholds out of range (min_depth >= 1, min_alt >= 1, min_af_ppm <= 1000000)");
    if (!a->pileup_tab) return fail(BGR_E_ARG, "bgr_aligner_pileup_sites: the pileup was never enabled on this aligner (bgr_aligner_pileup_enable)");
    const uint64_t nu = a->graph->header.n_unitigs;
    std::vector<bgr_unitig_abundance> ab(nu);
    int rc = bgr_aligner_abundance(a, ab.data(), nu);   // (synchronises the aligner's stream and its twins')
    if (rc == BGR_OK) rc = pileup_guard(ab.data(), nu, "bgr_aligner_pileup_sites");
    if (rc != BGR_OK) return rc;
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) HIP_TRY(hipStreamSynchronize(x->stream));
    return variants_call(a->dg, a->graph, a->pileup_tab, a->pileup_base_offs, *params, a->var_scratch, a->var_out, a->stream, "bgr_aligner_pileup_sites", nullptr, out, cap, n,
                         a->knob_no_events ? nullptr : a->var_ms);
}

int bgr_aligner_pileup_strand_sites(bgr_aligner* a, const bgr_variant_strand_params* params, bgr_variant_strand_site* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!a || !params || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_aligner_pileup_strand_sites: null argument");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_pileup_strand_sites: an internal stream of another aligner");
    if (!bgr::variants_params_ok(bgr_variant_params{params->min_depth, params->min_alt, params->min_af_ppm}))
        return fail(BGR_E_ARG, "bgr_aligner_pileup_strand_sites: thresholds out of range (min_depth >= 1, min_alt >= 1, min_af_ppm <= 1000000)");
    if (!a->pileup_tab || !a->pileup_fwd_tab) return fail(BGR_E_ARG, "bgr_aligner_pileup_strand_sites: strands were never counted on this aligner (bgr_aligner_pileup_strands_enable)");
    const uint64_t nu = a->graph->header.n_unitigs;
    std::vector<bgr_unitig_abundance> ab(nu);
    int rc = bgr_aligner_abundance(a, ab.data(), nu);   // (synchronises the aligner's stream and its twins')
    if (rc == BGR_OK) rc = pileup_guard(ab.data(), nu, "bgr_aligner_pileup_strand_sites");
    if (rc != BGR_OK) return rc;
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) HIP_TRY(hipStreamSynchronize(x->stream));
    return variants_strands_call(a->dg, a->graph, a->pileup_tab, a->pileup_fwd_tab, a->pileup_base_offs, *params, a->var_scratch, a->var_out, a->stream, "bgr_aligner_pileup_strand_sites", nullptr,
                                 out, cap, n, a->knob_no_events ? nullptr : a->var_ms);
}

int bgr_aligner_pileup_sites_times(bgr_aligner* a, double ms[5]) {
    if (!a || !ms) return fail(BGR_E_ARG, "bgr_aligner_pileup_sites_times: null argument");
    for (int i = 0; i < 5; ++i) ms[i] = a->var_ms[i];
    return BGR_OK;
}

int bgr_aligner_pileup_add(bgr_aligner* dst, bgr_aligner* src) {
    if (!dst || !src) return fail(BGR_E_ARG, "bgr_aligner_pileup_add: null aligner");
    if (dst->is_twin || src->is_twin) return fail(BGR_E_ARG, "bgr_aligner_pileup_add: an internal stream of another aligner");
    if (dst == src || dst->graph != src->graph) return fail(BGR_E_ARG, "bgr_aligner_pileup_add: two different aligners of one graph are needed");
    if (!dst->pileup_tab || !src->pileup_tab) return fail(BGR_E_ARG, "bgr_aligner_pileup_add: the pileup was never enabled on one of the aligners (bgr_aligner_pileup_enable)");
    if (!dst->pileup_fwd_tab != !src->pileup_fwd_tab)
        return fail(BGR_E_ARG, "bgr_aligner_pileup_add: one of the aligners has a forward table (bgr_aligner_pileup_strands_enable) and the other has none");
    HIP_TRY(hipSetDevice(src->device));
    for (bgr_aligner* x = src; x; x = x->twin) HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipSetDevice(dst->device));
    for (bgr_aligner* x = dst; x; x = x->twin) HIP_TRY(hipStreamSynchronize(x->stream));
    const uint64_t bytes = bgr::pileup_table_bytes(dst->graph->header.total_bases / 2, dst->graph->header.n_unitigs);
    const int rc = variants_table_add(dst->pileup_tab, dst->device, src->pileup_tab, src->device, bytes, dst->var_stage, (uint32_t)dst->num_cus, dst->stream, "bgr_aligner_pileup_add");
    if (rc != BGR_OK || !dst->pileup_fwd_tab) return rc;
    return variants_table_add(dst->pileup_fwd_tab, dst->device, src->pileup_fwd_tab, src->device, bytes, dst->var_stage, (uint32_t)dst->num_cus, dst->stream, "bgr_aligner_pileup_add");
}

// a run's aligner, its streams idle from here on: the first one's table becomes the run's (the buffers move: nothing is allocated), the others' are added
static int variants_collect(bgr_graph* g, bgr_aligner* a) {
    if (!a->pileup_tab) return fail(BGR_E_ARG, "bgr_align_all: the pileup was never enabled on an aligner of the run");
    const bool strands = g->variants_strands_on;   // the forward table travels with the total one
    if (strands && !a->pileup_fwd_tab) return fail(BGR_E_ARG, "bgr_align_all: strands were never counted on an aligner of the run");
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) HIP_TRY(hipStreamSynchronize(x->stream));
    std::lock_guard<std::mutex> l(g->abundance_m);   // (the lanes of a split run end side by side: one at a time here)
    if (!g->variants_run) {
        VariantsRun* r = new VariantsRun();
        r->device = a->device; r->num_cus = a->num_cus; r->dg = a->dg;
        if (hipStreamCreate(&r->stream) != hipSuccess) { delete r; (void)hipGetLastError(); return fail(BGR_E_HIP, "bgr_align_all: a stream for the run's pileup table"); }
        std::swap(r->table, a->pileup);
        std::swap(r->offs, a->pileup_offs);
        if (strands) { std::swap(r->table_fwd, a->pileup_fwd); a->pileup_fwd_tab = nullptr; a->strands_on = false; }
        a->pileup_tab = nullptr; a->pileup_base_offs = nullptr; a->pileup_on = false;
        pileup_share(a);
        g->variants_run = r;
        return BGR_OK;
    }
    VariantsRun* r = g->variants_run;
    HIP_TRY(hipSetDevice(r->device));
    const uint64_t bytes = bgr::pileup_table_bytes(g->header.total_bases / 2, g->header.n_unitigs);
    const int rc = variants_table_add(static_cast<uint32_t*>(r->table.p), r->device, a->pileup_tab, a->device, bytes, r->stage, (uint32_t)r->num_cus, r->stream, "bgr_align_all");
    if (rc != BGR_OK || !strands) return rc;
    if (!r->table_fwd.p) return fail(BGR_E_INTERNAL, "bgr_align_all: the run's pileup table has no forward table");
    return variants_table_add(static_cast<uint32_t*>(r->table_fwd.p), r->device, a->pileup_fwd_tab, a->device, bytes, r->stage, (uint32_t)r->num_cus, r->stream, "bgr_align_all");
}
// the run's end: behind the guard of the summed abundance the passes run once on the run's table; the table is freed whatever happens
static int variants_end(bgr_graph* g, bool ok) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    int rc = BGR_OK;
    if (ok) {
        rc = g->abundance_valid ? pileup_guard(g->abundance.data(), g->abundance.size(), "bgr_align_all") : fail(BGR_E_INTERNAL, "bgr_align_all: sites without the abundance totals that guard them");
        if (rc == BGR_OK && g->variants_run) {
            VariantsRun* r = g->variants_run;
            DevBuf scratch, outbuf;
            uint64_t n = 0;
            if (hipSetDevice(r->device) != hipSuccess) rc = fail(BGR_E_HIP, "bgr_align_all: hipSetDevice for the run's pileup table");
            else if (!g->variants_strands_on)
                rc = variants_call(r->dg, g, static_cast<const uint32_t*>(r->table.p), static_cast<const uint64_t*>(r->offs.p), g->variants_prm, scratch, outbuf, r->stream, "bgr_align_all",
                                   &g->variants_sites, nullptr, 0, &n, nullptr);
            else if (!r->table_fwd.p) rc = fail(BGR_E_INTERNAL, "bgr_align_all: the run's pileup table has no forward table");
            else {
                const bgr_variant_strand_params sp = {g->variants_prm.min_depth, g->variants_prm.min_alt, g->variants_prm.min_af_ppm, g->variants_min_alt_strand};
                rc = variants_strands_call(r->dg, g, static_cast<const uint32_t*>(r->table.p), static_cast<const uint32_t*>(r->table_fwd.p), static_cast<const uint64_t*>(r->offs.p), sp, scratch,
                                           outbuf, r->stream, "bgr_align_all", &g->variants_strand_sites, nullptr, 0, &n, nullptr);
                if (rc == BGR_OK) {   // (bgr_graph_variants then delivers the same sites without the forward numbers)
                    g->variants_sites.resize(g->variants_strand_sites.size());
                    for (size_t i = 0; i < g->variants_sites.size(); ++i) memcpy(&g->variants_sites[i], &g->variants_strand_sites[i], sizeof(bgr_variant_site));
                }
            }
            scratch.release(); outbuf.release();
        }
    }
    variants_run_free(g);
    if (!ok || rc != BGR_OK) { g->variants_sites.clear(); g->variants_sites.shrink_to_fit(); g->variants_strand_sites.clear(); g->variants_strand_sites.shrink_to_fit(); }
    g->variants_called = g->variants_prm;
    g->variants_called_strand = g->variants_min_alt_strand;
    g->variants_valid = ok && rc == BGR_OK;
    g->variants_strands_valid = g->variants_valid && g->variants_strands_on;
    return rc;
}

int bgr_graph_variants_enable(bgr_graph* g, const bgr_variant_params* params) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_variants_enable: null graph");
    if (params) {
        if (!bgr::variants_params_ok(*params)) return fail(BGR_E_ARG, "bgr_graph_variants_enable: thresholds out of range (min_depth >= 1, min_alt >= 1, min_af_ppm <= 1000000)");
        int rc = pileup_refusal(g, "bgr_graph_variants_enable");
        if (rc == BGR_OK) rc = graph_base_offs(g, "bgr_graph_variants_enable");
        if (rc != BGR_OK) return rc;
        g->variants_prm = *params;
    }
    g->variants_on = params != nullptr;
    g->variants_strands_on = false;   // (the plain switch: 32-byte records, no forward table)
    return BGR_OK;
}

int bgr_graph_variants_strands_enable(bgr_graph* g, const bgr_variant_strand_params* params) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_variants_strands_enable: null graph");
    if (!params) return bgr_graph_variants_enable(g, nullptr);
    const bgr_variant_params prm = {params->min_depth, params->min_alt, params->min_af_ppm};
    const int rc = bgr_graph_variants_enable(g, &prm);
    if (rc != BGR_OK) return rc;
    g->variants_strands_on = true;
    g->variants_min_alt_strand = params->min_alt_strand;
    return BGR_OK;
}

int bgr_graph_variant_strand_sites(const bgr_graph* g, bgr_variant_strand_site* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!g || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_graph_variant_strand_sites: null argument");
    if (!g->variants_strands_valid) return fail(BGR_E_ARG, "bgr_graph_variant_strand_sites: no totals -- they are those of the last successful bgr_align_all with bgr_graph_variants_strands_enable on");
    *n = g->variants_strand_sites.size();
    if (g->variants_strand_sites.size() > cap) return fail(BGR_E_CAPACITY, "bgr_graph_variant_strand_sites: " + std::to_string(g->variants_strand_sites.size()) + " sites, room for " + std::to_string(cap));
    if (!g->variants_strand_sites.empty()) memcpy(out, g->variants_strand_sites.data(), g->variants_strand_sites.size() * sizeof(bgr_variant_strand_site));
    return BGR_OK;
}

int bgr_graph_variants_enabled(const bgr_graph* g) { return g && g->variants_on ? 1 : 0; }

int bgr_graph_variants(const bgr_graph* g, bgr_variant_site* out, uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    if (!g || !n || (cap && !out)) return fail(BGR_E_ARG, "bgr_graph_variants: null argument");
    if (!g->variants_valid) return fail(BGR_E_ARG, "bgr_graph_variants: no totals -- they are those of the last successful bgr_align_all with bgr_graph_variants_enable on");
    *n = g->variants_sites.size();
    if (g->variants_sites.size() > cap) return fail(BGR_E_CAPACITY, "bgr_graph_variants: " + std::to_string(g->variants_sites.size()) + " sites, room for " + std::to_string(cap));
    if (!g->variants_sites.empty()) memcpy(out, g->variants_sites.data(), g->variants_sites.size() * sizeof(bgr_variant_site));
    return BGR_OK;
}

int bgr_graph_variants_params(const bgr_graph* g, bgr_variant_params* out) {
    if (!g || !out) return fail(BGR_E_ARG, "bgr_graph_variants_params: null argument");
    if (!g->variants_valid) return fail(BGR_E_ARG, "bgr_graph_variants_params: no totals -- they are those of the last successful bgr_align_all with bgr_graph_variants_enable on");
    *out = g->variants_called;
    return BGR_OK;
}

int bgr_write_vcf(const char* path, const bgr_graph* g, const bgr_variant_params* params, const bgr_variant_site* sites, uint64_t n) {
    if (!path || !g || !params || (n && !sites)) return fail(BGR_E_ARG, "bgr_write_vcf: null argument");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_write_vcf: the graph has no host blob (the reference letters are read from it)");
    if (g->header.has_exc) return fail(BGR_E_ARG, "bgr_write_vcf: a graph of ACGT-only unitigs is needed (--vcf): the 2-bit store does not spell other characters");
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
    const uint64_t* seq = reinterpret_cast<const uint64_t*>(g->host.base() + g->header.off_seq);
    std::string err;
    if (!bgr::vcf_write(nullptr, meta, seq, g->header.n_unitigs, *params, sites, n, &err)) return fail(BGR_E_ARG, "bgr_write_vcf: " + err);   // (the checks alone: no file for sites that are none)
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string("bgr_write_vcf: cannot open ") + path);
    bool ok = bgr::vcf_write(f, meta, seq, g->header.n_unitigs, *params, sites, n, &err);
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string("bgr_write_vcf: write to ") + path + " failed");
    return BGR_OK;
}

int bgr_write_vcf_strands(const char* path, const bgr_graph* g, const bgr_variant_strand_params* params, const bgr_variant_strand_site* sites, uint64_t n) {
    if (!path || !g || !params || (n && !sites)) return fail(BGR_E_ARG, "bgr_write_vcf_strands: null argument");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_write_vcf_strands: the graph has no host blob (the reference letters are read from it)");
    if (g->header.has_exc) return fail(BGR_E_ARG, "bgr_write_vcf_strands: a graph of ACGT-only unitigs is needed (--vcf): the 2-bit store does not spell other characters");
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
    const uint64_t* seq = reinterpret_cast<const uint64_t*>(g->host.base() + g->header.off_seq);
    std::string err;
    if (!bgr::vcf_strands_write(nullptr, meta, seq, g->header.n_unitigs, *params, sites, n, &err)) return fail(BGR_E_ARG, "bgr_write_vcf_strands: " + err);   // (the checks alone)
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string("bgr_write_vcf_strands: cannot open ") + path);
    bool ok = bgr::vcf_strands_write(f, meta, seq, g->header.n_unitigs, *params, sites, n, &err);
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string("bgr_write_vcf_strands: write to ") + path + " failed");
    return BGR_OK;
}

int bgr_parse_min_alt_strand(const char* text, uint32_t* out) {
    if (!text || !out) return fail(BGR_E_ARG, "bgr_parse_min_alt_strand: null argument");
    if (!bgr::parse_min_alt_strand(text, out)) return fail(BGR_E_ARG, std::string("bgr_parse_min_alt_strand: '") + text + "' is no non-negative integer of at most nine digits");
    return BGR_OK;
}

int bgr_parse_af_ppm(const char* text, uint32_t* ppm) {
    if (!text || !ppm) return fail(BGR_E_ARG, "bgr_parse_af_ppm: null argument");
    if (!bgr::parse_af_ppm(text, ppm)) return fail(BGR_E_ARG, std::string("bgr_parse_af_ppm: '") + text + "' is no fraction between 0 and 1 with at most six decimals");
    return BGR_OK;
}


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

static void links_share(bgr_aligner* a) {   // the twins add to the aligner's table
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
static int links_tail(bgr_aligner* a, const char* who, uint64_t tail[bgr::kLinksTailWords]) {
    if (!a->links_tab) return fail(BGR_E_ARG, std::string(who) + ": links were never enabled on this aligner (bgr_aligner_links_enable)");
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) HIP_TRY(hipStreamSynchronize(x->stream));
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
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) HIP_TRY(hipStreamSynchronize(x->stream));   // (the twins add to the same table)
    HIP_TRY(hipMemsetAsync(a->links.p, 0, a->links.cap, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return BGR_OK;
}

// what a whole run calls (run_links.h)
static bool run_links_wanted(const bgr_graph* g) { return g && g->links_on; }
static void run_links_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->links.clear();
    g->links_valid = false;
}
static int run_links_enable(bgr_aligner* a) { return bgr_aligner_links_enable(a, 1); }
static int run_links_collect(bgr_graph* g, bgr_aligner* a) {
    std::vector<std::pair<uint64_t, uint64_t>> kv;
    uint64_t tail[bgr::kLinksTailWords];
    const int rc = links_snapshot(a, "bgr_align_all", ~0ull, kv, tail);
    if (rc != BGR_OK) return rc;
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->links.insert(g->links.end(), kv.begin(), kv.end());
    return BGR_OK;
}
static void run_links_end(bgr_graph* g, bool ok) {   // the aligners' tables, one behind the other: sorted, equal keys summed
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
static const bool g_run_links_registered = (bgr::g_run_links = bgr::RunLinks{run_links_wanted, run_links_begin, run_links_enable, run_links_collect, run_links_end}, true);

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

int bgr_align_device(bgr_aligner* a, const bgr_params* p, const void* d_reads, const void* d_read_offsets, uint64_t n_reads,
                     uint64_t total_bases, uint32_t max_read_len) {
    return align_device_impl(a, p, d_reads, d_read_offsets, n_reads, total_bases, max_read_len, false);
}

uint64_t bgr_packed_plane_words(uint64_t n_reads, uint64_t total_bases) { return bgr::packed_plane_words(n_reads, total_bases); }

int bgr_pack_reads(const char* reads, const uint64_t* read_offsets, uint64_t n, uint64_t* fw3, uint32_t* hasn, uint32_t* nm_index, uint64_t* nm_value,
                   uint64_t nm_cap, uint64_t* nm_count, uint32_t* max_read_len) {
    if (!read_offsets || !fw3 || !hasn || !nm_count || (n && !reads)) return fail(BGR_E_ARG, "bgr_pack_reads: null argument");
    const uint64_t base = read_offsets[0];
    memset(hasn, 0, ((n + 31) / 32) * 4);
    uint64_t cnt = 0;
    uint32_t longest = 0;
    std::vector<uint64_t> nm;
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t off = read_offsets[r] - base, len64 = read_offsets[r + 1] - read_offsets[r];
        if (len64 > 0x7FFFFFFFull) return fail(BGR_E_ARG, "bgr_pack_reads: read longer than 2^31 bases");
        const uint32_t len = (uint32_t)len64, words = (len + 31) >> 5;
        longest = std::max(longest, len);
        if (nm.size() < words) nm.resize(words);
        const uint64_t w0 = bgr::packed_word_offset(off, r);
        if (bgr::pack_read(reads + read_offsets[r], len, fw3 + w0, nm.data())) {
            hasn[r >> 5] |= 1u << (r & 31);
            if (cnt + words > nm_cap || !nm_index || !nm_value) return fail(BGR_E_CAPACITY, "bgr_pack_reads: N-mask list too small");
            for (uint32_t j = 0; j < words; ++j) { nm_index[cnt] = (uint32_t)(w0 + j); nm_value[cnt] = nm[j]; ++cnt; }
        }
    }
    *nm_count = cnt;
    if (max_read_len) *max_read_len = longest;
    return BGR_OK;
}

int bgr_align_batch_packed(bgr_aligner* a, const bgr_params* p, const bgr_packed_reads* pk, uint64_t n, int32_t* paths_out, uint64_t paths_cap,
                           uint64_t* path_offsets, uint8_t* status) {
    if (!a || !p || !pk || !path_offsets || (n && (!pk->read_offsets || !pk->fw3 || !pk->hasn || !status))) return fail(BGR_E_ARG, "bgr_align_batch_packed: null argument");
    if (pk->nm_count && (!pk->nm_index || !pk->nm_value)) return fail(BGR_E_ARG, "bgr_align_batch_packed: null N-mask list");
    path_offsets[0] = 0;
    a->last_n = 0;
    if (n == 0) return BGR_OK;
    if (pk->read_offsets[0] != 0) return fail(BGR_E_ARG, "bgr_align_batch_packed: read_offsets must start at 0 (they address the planes)");
    const uint64_t total = pk->read_offsets[n];
    if (n >= 0x7FFFFFFFull || 2 * (total + 16 * n) >= 0xFFFFFFFFull - (256ull << 20))
        return fail(BGR_E_ARG, "bgr_align_batch_packed: batch too large for one launch (2*(bases + 16*reads) must stay below 2^32 - 2^28); pack it in pieces");
    HIP_TRY(hipSetDevice(a->device));
    const uint64_t plane_words = bgr::packed_plane_words(n, total);
    HIP_TRY(a->in_offs.ensure((n + 1) * 8));
    HIP_TRY(a->pk_fw3.ensure(plane_words * 8));
    HIP_TRY(a->pk_nm.ensure(plane_words * 8));
    HIP_TRY(a->pk_hasn.ensure((n + 31) / 32 * 4 + 4));
    HIP_TRY(hipMemcpyAsync(a->in_offs.p, pk->read_offsets, (n + 1) * 8, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(a->pk_fw3.p, pk->fw3, ((total >> 5) + n + 1) * 8, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(a->pk_hasn.p, pk->hasn, (n + 31) / 32 * 4, hipMemcpyHostToDevice, a->stream));
    if (pk->nm_count) {  // the N-mask words of the few reads that hold an N: a sparse list, scattered into the plane on the device
        const uint64_t voff = (pk->nm_count * 4 + 7) & ~7ull;  // indices, then the values 8-byte aligned, in the ASCII staging buffer (unused here)
        HIP_TRY(a->in_reads.ensure(voff + pk->nm_count * 8));
        char* d = static_cast<char*>(a->in_reads.p);
        HIP_TRY(hipMemcpyAsync(d, pk->nm_index, pk->nm_count * 4, hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipMemcpyAsync(d + voff, pk->nm_value, pk->nm_count * 8, hipMemcpyHostToDevice, a->stream));
        hipError_t e = bgr::launch_scatter_words(reinterpret_cast<const uint32_t*>(d), reinterpret_cast<const uint64_t*>(d + voff), pk->nm_count,
                                                 static_cast<uint64_t*>(a->pk_nm.p), plane_words, a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("N-mask scatter launch: ") + hipGetErrorString(e));
    }
    uint32_t max_len = pk->max_read_len;
    if (!max_len) {
        for (uint64_t i = 0; i < n; ++i) max_len = std::max<uint32_t>(max_len, (uint32_t)std::min<uint64_t>(pk->read_offsets[i + 1] - pk->read_offsets[i], 0x7FFFFFFFull));
    }
    // (the host buffers may be reused once the copies are done: bgr_aligner_fetch below synchronises the stream)
    int rc = align_device_impl(a, p, nullptr, a->in_offs.p, n, total, max_len, true);
    if (rc != BGR_OK) return rc;
    return bgr_aligner_fetch(a, n, paths_out, paths_cap, path_offsets, status);
}

// ---- text form: FASTA bytes in, record bytes out (text_kernels.hip) -------------------------------------------------------------
static int fetch_text_impl(bgr_aligner* a, bgr_text_batch* b) {
    b->paths_bytes = a->tx_pbytes;
    b->notaligned_bytes = a->tx_nbytes;
    if (!b->want_output || a->tx_n_acc == 0) return BGR_OK;
    if (a->tx_pbytes > b->paths_cap || a->tx_nbytes > b->notaligned_cap || (a->tx_pbytes && !b->paths_out) || (a->tx_nbytes && !b->notaligned_out))
        return fail(BGR_E_CAPACITY, "bgr_align_fasta_text: output buffer too small (paths_bytes / notaligned_bytes say what is needed; bgr_aligner_fetch_text)");
    if (!a->tx_written) {   // (correction mode; streams larger than the buffers the format launch wrote into; a second fetch)
    HIP_TRY(a->tx_pout.ensure(a->tx_pbytes + 64));
    HIP_TRY(a->tx_nout.ensure(a->tx_nbytes + 64));
    hipError_t e = a->tx_want == 3
        ? bgr::launch_text_gaf_write(a->dg, a->tx_text, static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p), static_cast<const uint4*>(a->tx_rec.p),
                                     static_cast<const uint32_t*>(a->tx_accrec.p), (uint32_t)a->tx_n_acc, static_cast<const uint32_t*>(a->tx_poff.p),
                                     static_cast<const uint32_t*>(a->tx_noff.p), static_cast<const uint32_t*>(a->tx_psz.p), static_cast<const uint32_t*>(a->tx_idx.p),
                                     static_cast<const uint4*>(a->tx_gaf.p), static_cast<uint8_t*>(a->tx_pout.p), static_cast<uint8_t*>(a->tx_nout.p), a->stream)
        : a->tx_want == 2
        ? bgr::launch_text_correct_write(a->dg, a->tx_text, static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p), static_cast<const uint4*>(a->tx_rec.p),
                                         static_cast<const uint32_t*>(a->tx_accrec.p), (uint32_t)a->tx_n_acc, static_cast<const uint32_t*>(a->tx_poff.p),
                                         static_cast<const uint32_t*>(a->tx_noff.p), static_cast<const uint32_t*>(a->tx_idx.p), static_cast<uint8_t*>(a->tx_pout.p),
                                         static_cast<uint8_t*>(a->tx_nout.p), a->stream)
        : bgr::launch_text_write(a->tx_text, static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p),
                                 static_cast<const uint4*>(a->tx_rec.p), static_cast<const uint32_t*>(a->tx_accrec.p), (uint32_t)a->tx_n_acc,
                                 static_cast<const uint32_t*>(a->tx_poff.p), static_cast<const uint32_t*>(a->tx_noff.p), static_cast<uint8_t*>(a->tx_pout.p),
                                 static_cast<uint8_t*>(a->tx_nout.p), a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("text write launch: ") + hipGetErrorString(e));
    a->tx_written = true;
    }
    if (a->tx_pbytes) HIP_TRY(hipMemcpyAsync(b->paths_out, a->tx_pout.p, a->tx_pbytes, hipMemcpyDeviceToHost, a->stream));
    if (a->tx_nbytes) HIP_TRY(hipMemcpyAsync(b->notaligned_out, a->tx_nout.p, a->tx_nbytes, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    return BGR_OK;
}

int bgr_aligner_fetch_text(bgr_aligner* a, bgr_text_batch* b) {
    if (!a || !b) return fail(BGR_E_ARG, "bgr_aligner_fetch_text: null argument");
    if (b->struct_size != sizeof(bgr_text_batch)) return fail(BGR_E_ARG, "bgr_aligner_fetch_text: bgr_text_batch.struct_size is not this library's sizeof(bgr_text_batch)");
    HIP_TRY(hipSetDevice(a->device));
    return fetch_text_impl(a, b);
}

int bgr_text_stage_create(int device, bgr_text_stage** out) {
    if (!out) return fail(BGR_E_ARG, "bgr_text_stage_create: null argument");
    HIP_TRY(hipSetDevice(device));
    bgr_text_stage* s = new bgr_text_stage();
    s->device = device;
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    s->timing = bgr::opt("timing") != 0;
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev, s->timing ? hipEventDefault : hipEventDisableTiming);
    if (e == hipSuccess && s->timing) e = hipEventCreate(&s->ev0);
    if (e != hipSuccess) { bgr_text_stage_destroy(s); return fail(BGR_E_HIP, std::string("bgr_text_stage_create: ") + hipGetErrorString(e)); }
    *out = s;
    return BGR_OK;
}

void bgr_text_stage_destroy(bgr_text_stage* s) {
    if (!s) return;
    if (hipSetDevice(s->device) == hipSuccess) {
        if (s->stream) { (void)hipStreamSynchronize(s->stream); s->settle(); (void)hipStreamDestroy(s->stream); }
        if (s->timing && s->copy_ms > 0) fprintf(stderr, "bgreat: stage on device %d: %.0f MB up in %.3f s of copies = %.1f GB/s\n", s->device, s->copy_bytes / 1e6, s->copy_ms / 1e3, s->copy_bytes / s->copy_ms / 1e6);
        if (s->ev) (void)hipEventDestroy(s->ev);
        if (s->ev0) (void)hipEventDestroy(s->ev0);
        s->buf.release();
    }
    delete s;
}

int bgr_text_stage_device(const bgr_text_stage* s) { return s ? s->device : -1; }

int bgr_text_stage_upload(bgr_text_stage* s, const char* text, uint64_t bytes) {
    if (!s || (bytes && !text)) return fail(BGR_E_ARG, "bgr_text_stage_upload: null argument");
    if (bytes >= (1ull << 31)) return fail(BGR_E_ARG, "bgr_text_stage_upload: piece of 2 GiB or more; cut it");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));  // (a piece still on its way: the buffer may grow, i.e. move)
    s->settle();
    HIP_TRY(s->buf.ensure(bytes + 128));
    if (s->timing) { HIP_TRY(hipEventRecord(s->ev0, s->stream)); s->pending = true; }
    HIP_TRY(hipMemsetAsync(static_cast<char*>(s->buf.p) + (bytes & ~63ull), 0, 128, s->stream));   // (from an aligned address: one fill; the copies below lay the text over its start)
    if (bytes) HIP_TRY(hipMemcpyAsync(s->buf.p, text, bytes, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(s->ev, s->stream));
    s->bytes = bytes;
    return BGR_OK;
}

int bgr_text_stage_upload_parts(bgr_text_stage* s, uint32_t n_parts, const char* const* parts, const uint64_t* part_bytes) {
    if (!s || (n_parts && (!parts || !part_bytes))) return fail(BGR_E_ARG, "bgr_text_stage_upload_parts: null argument");
    uint64_t bytes = 0;
    for (uint32_t i = 0; i < n_parts; ++i) { if (part_bytes[i] && !parts[i]) return fail(BGR_E_ARG, "bgr_text_stage_upload_parts: null part"); bytes += part_bytes[i]; }
    if (bytes >= (1ull << 31)) return fail(BGR_E_ARG, "bgr_text_stage_upload_parts: piece of 2 GiB or more; cut it");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));  // (a piece still on its way: the buffer may grow, i.e. move)
    s->settle();
    HIP_TRY(s->buf.ensure(bytes + 128));
    if (s->timing) { HIP_TRY(hipEventRecord(s->ev0, s->stream)); s->pending = true; }
    HIP_TRY(hipMemsetAsync(static_cast<char*>(s->buf.p) + (bytes & ~63ull), 0, 128, s->stream));   // (from an aligned address: one fill; the copies below lay the text over its start)
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_parts; ++i) {
        if (part_bytes[i]) HIP_TRY(hipMemcpyAsync(static_cast<char*>(s->buf.p) + at, parts[i], part_bytes[i], hipMemcpyHostToDevice, s->stream));
        at += part_bytes[i];
    }
    HIP_TRY(hipEventRecord(s->ev, s->stream));
    s->bytes = bytes;
    return BGR_OK;
}

static double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int bgr_align_fasta_text(bgr_aligner* a, const bgr_params* p, bgr_text_batch* b) {
    if (!a || !p || !b) return fail(BGR_E_ARG, "bgr_align_fasta_text: null argument");
    if (b->struct_size != sizeof(bgr_text_batch)) return fail(BGR_E_ARG, "bgr_align_fasta_text: bgr_text_batch.struct_size is not this library's sizeof(bgr_text_batch): the caller was built against another header (zero the struct, set struct_size)");
    if (b->text_bytes && !b->text && !b->stage) return fail(BGR_E_ARG, "bgr_align_fasta_text: null argument");
    if (b->record_info_out && b->text_bytes >= (1ull << 30)) return fail(BGR_E_ARG, "bgr_align_fasta_text: record_info_out holds a read's length in 30 bits: pieces below 2^30 bytes");
    double tw = wall_now();
    auto lap = [&](int i) { const double t = wall_now(); a->tx_phase_s[i] += t - tw; tw = t; };
    if (b->text_bytes >= (1ull << 31)) return fail(BGR_E_ARG, "bgr_align_fasta_text: piece of 2 GiB or more; cut it");
    if (b->want_output > 3) return fail(BGR_E_ARG, "bgr_align_fasta_text: want_output must be 0, 1, 2 or 3");
    if (b->fastq > 2) return fail(BGR_E_ARG, "bgr_align_fasta_text: fastq must be 0, 1 (four-line records) or 2 (header and read lines only)");
    const uint32_t rec_lines = b->fastq == 2 ? 2u : b->fastq ? 4u : 0u;  // lines per record of a FASTQ piece (0: FASTA, records start at '>' lines)
    if (b->fastq && b->text_bytes && b->text && b->text[b->text_bytes - 1] != '\n' && !b->stage)
        return fail(BGR_E_ARG, "bgr_align_fasta_text: a FASTQ piece holds whole four-line records and ends with a newline");
    if (b->want_output == 2 && (a->graph->header.has_exc || p->mode == BGR_MODE_EXHAUSTIVE))
        return fail(BGR_E_ARG, "bgr_align_fasta_text: correction on the device needs a graph of ACGT-only unitigs and greedy mode (format such a run on the host)");
    if (b->want_output == 3 && (a->graph->header.has_exc || p->mode == BGR_MODE_EXHAUSTIVE))
        return fail(BGR_E_ARG, "bgr_align_fasta_text: GAF output needs a graph of ACGT-only unitigs (a path read backwards does not spell the reverse complement on one with other characters) and a greedy mode");
    if (b->record_info_out && (b->want_output >= 2 || b->record_info_cap < b->text_bytes / 24 + 1024))
        return fail(BGR_E_ARG, "bgr_align_fasta_text: record_info_out needs room for text_bytes / 24 + 1024 words and is not available in correction mode or with GAF output");
    a->tx_want = b->want_output;
    b->irregular = 0;
    b->n_records = b->n_accepted = b->paths_bytes = b->notaligned_bytes = 0;
    a->last_n = 0;
    a->tx_n_acc = a->tx_pbytes = a->tx_nbytes = 0;
    if (b->text_bytes == 0) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    const uint32_t nbytes = (uint32_t)b->text_bytes;
    const uint8_t* text = nullptr;
    // 1. the piece in HBM (zero padded): uploaded ahead of this call by a stage (bgr_text_stage_upload, a copy stream of its own), or copied now
    if (b->stage) {
        if (b->stage->device != a->device || b->stage->bytes != b->text_bytes) return fail(BGR_E_ARG, "bgr_align_fasta_text: the stage holds another piece / lives on another device");
        HIP_TRY(hipStreamWaitEvent(a->stream, b->stage->ev, 0));
        text = static_cast<const uint8_t*>(b->stage->buf.p);
    } else {
        if (!b->text) return fail(BGR_E_ARG, "bgr_align_fasta_text: null text");
        HIP_TRY(a->tx_in.ensure((uint64_t)nbytes + 128));
        text = static_cast<const uint8_t*>(a->tx_in.p);
        HIP_TRY(hipMemsetAsync(static_cast<char*>(a->tx_in.p) + (nbytes & ~63ull), 0, 128, a->stream));   // (64 zero bytes behind the piece at least; from an aligned address: ONE fill, and the copy below lays the text over its start)
        HIP_TRY(hipMemcpyAsync(a->tx_in.p, b->text, nbytes, hipMemcpyHostToDevice, a->stream));
    }
    a->tx_text = text;
    // 2. records: starts, extents, shape, accept test; accepted records compacted in input order.  Room for one record per 24 bytes of
    // text (a sequencing read with its header is several times that): a piece with more record starts goes to the host parser.
    const uint32_t R_cap = nbytes / 24 + 1024;
    // (tickets and chains of the two one-launch kernels, text_kernels.hip: never cleared between launches -- every launch gets a fresh epoch)
    {
        const uint64_t chain_words = std::max<uint64_t>(3ull * bgr::text_tiles(nbytes), 2ull * bgr::format_tiles(R_cap));
        const size_t had = a->tx_state.cap;
        HIP_TRY(a->tx_state.ensure(64 + chain_words * 8));
        if (a->tx_state.cap != had || a->tx_epoch + 2 > BGR_TEXT_EPOCH_MAX) {
            const bool fresh = a->tx_state.cap != had;
            HIP_TRY(hipMemsetAsync(a->tx_state.p, 0, a->tx_state.cap, a->stream));
            a->tx_epoch = fresh ? (uint32_t)bgr::opt("test.text_epoch") : 0u;   // (0 but for the test hook)
            a->tx_ticket[0] = a->tx_ticket[1] = 0;
        }
    }
    uint32_t* tickets = static_cast<uint32_t*>(a->tx_state.p);
    uint64_t* chains = reinterpret_cast<uint64_t*>(static_cast<char*>(a->tx_state.p) + 64);
    HIP_TRY(a->tx_sums.ensure((2ull * bgr::scan_tiles(R_cap) + 16) * 4));   // (correction mode's scans)
    for (DevBuf* d : {&a->tx_idx, &a->tx_accrec, &a->tx_accsrc, &a->tx_psz, &a->tx_nsz, &a->tx_poff, &a->tx_noff})
        HIP_TRY(d->ensure(((uint64_t)R_cap + 4) * 4));
    HIP_TRY(a->tx_rec.ensure(((uint64_t)R_cap + 1) * 16));
    HIP_TRY(a->tx_offs.ensure(((uint64_t)R_cap + 2) * 8));
    uint32_t* sums2 = static_cast<uint32_t*>(a->tx_sums.p);
    // TXT_INFO_WORDS u32 behind cursor / counters / CSR total -- two such blocks, taken in turn: a piece's parse launch clears the block of the NEXT piece (and the
    // mapping launch's cursor), so that no fill stands in front of either (the blocks start zero: bgr_aligner_create)
    a->tx_flip ^= 1u;   // (here, behind everything that can fail before the launch: a block is cleared by the launch in front of the one that uses it)
    uint32_t* info = reinterpret_cast<uint32_t*>(static_cast<char*>(a->small.p) + bgr::kSmallTextInfo + bgr::kSmallTextInfoBytes * a->tx_flip);
    uint32_t* info_next = reinterpret_cast<uint32_t*>(static_cast<char*>(a->small.p) + bgr::kSmallTextInfo + bgr::kSmallTextInfoBytes * (a->tx_flip ^ 1u));
    static_assert(TXT_INFO_WORDS * 4 == bgr::kSmallTextInfoBytes, "two info blocks at small + kSmallTextInfo");
    hipError_t e = bgr::launch_text_parse(text, nbytes, rec_lines, a->dg.k, tickets, a->tx_ticket[0], ++a->tx_epoch, chains, static_cast<uint4*>(a->tx_rec.p),
                                          static_cast<uint32_t*>(a->tx_idx.p), static_cast<uint32_t*>(a->tx_accrec.p), static_cast<uint32_t*>(a->tx_accsrc.p),
                                          static_cast<uint64_t*>(a->tx_offs.p), info, R_cap, static_cast<uint32_t*>(a->small.p), bgr::kCurWords, info_next, TXT_INFO_WORDS, a->stream);
    if (e == hipSuccess) a->tx_ticket[0] += bgr::text_tiles(nbytes);   // (as many tickets as workgroups will take)
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("text record launches: ") + hipGetErrorString(e));
    uint32_t h[TXT_INFO_WORDS];
    HIP_TRY(hipMemcpyAsync(h, info, sizeof(h), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    lap(0);
    const uint32_t R = h[TXT_INFO_N_REC];
    b->n_records = R;
    if (R == 0 || R > R_cap) { b->irregular = 1; return BGR_OK; }  // no record start in the bytes, or far more than a read file has: the host parser decides
    lap(1);
    if (h[TXT_INFO_IRREGULAR]) { b->irregular = 1; return BGR_OK; }
    const uint32_t n_acc = h[TXT_INFO_N_ACC], bases = h[TXT_INFO_BASES], max_len = h[TXT_INFO_MAX_LEN];
    b->n_accepted = n_acc;
    if (n_acc == 0) {
        if (b->record_info_out) memset(b->record_info_out, 0, (size_t)R * 4);  // (nothing kept: every record a dropped one)
        return BGR_OK;
    }
    // 3. the mapping launch, its reads where they lie in the text (planes by the pre-pass, or -- greedy mode -- staged by the mapping kernels themselves)
    int rc = align_device_impl(a, p, text, a->tx_offs.p, n_acc, bases, max_len, false, a->tx_accsrc.p, nbytes, true);
    if (rc != BGR_OK) return rc;
    a->last_n = 0;  // (bgr_aligner_fetch has no host read_offsets to pair its rows with: the text form hands out text)
    a->tx_n_acc = n_acc;
    // Everything behind the mapping launch reads its results.  In exhaustive mode those are final only once the launch is settled (reads the last pass
    // handed back for a larger table are mapped again: settle_launch) -- which hardly ever happens: so the kernels below are enqueued at once, the
    // cursor comes back with the wait this call makes anyway, and only a launch that did hand reads back is settled and the kernels enqueued AGAIN
    // (a wait between the mapping launch and them cost -b a fifth of its end-to-end rate)
    uint64_t pcap_dev = 0, ncap_dev = 0;
    a->tx_written = false;
    for (int again = 0; again < 2; ++again) {
    if (b->record_info_out) {  // what became of every record (the -b progress blocks of the caller), on its way to the host behind the mapping launch
        HIP_TRY(a->tx_info.ensure((uint64_t)R * 4));
        e = bgr::launch_text_record_info(static_cast<const uint4*>(a->tx_rec.p), static_cast<const uint32_t*>(a->tx_idx.p), static_cast<const uint2*>(a->results.p), R,
                                         static_cast<uint32_t*>(a->tx_info.p), a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("record info launch: ") + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(b->record_info_out, a->tx_info.p, (size_t)R * 4, hipMemcpyDeviceToHost, a->stream));
    }
    if (!b->want_output) {  // counters only: the launch still has to be settled (arena flag; exhaustive mode: reads the last pass handed back)
        uint32_t cur[bgr::kCurWords];
        HIP_TRY(hipMemcpyAsync(cur, a->small.p, sizeof(cur), hipMemcpyDeviceToHost, a->stream));
        HIP_TRY(wait_stream(a));
        const bool handed_back = a->deep.open && cur[bgr::list_word(bgr::List::kRetry)] != 0;
        rc = settle_launch(a, cur);
        if (rc != BGR_OK || !handed_back || !b->record_info_out) return rc;
        continue;  // (the record info was made from results that were not final)
    }
    // 4. sizes of the records, stream offsets, the bytes
    if (b->want_output == 3) {  // (tx_idx is free again behind the compaction: it takes the lengths of the names)
        HIP_TRY(a->tx_gaf.ensure(((uint64_t)n_acc + 1) * 16));
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(info + TXT_INFO_BUG), -1, 1, a->stream));
        e = bgr::launch_text_gaf_sizes(a->dg, text, static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p), static_cast<const uint4*>(a->tx_rec.p),
                                       static_cast<const uint32_t*>(a->tx_accrec.p), n_acc, static_cast<uint32_t*>(a->tx_psz.p), static_cast<uint32_t*>(a->tx_nsz.p),
                                       static_cast<uint32_t*>(a->tx_idx.p), static_cast<uint4*>(a->tx_gaf.p), info + TXT_INFO_BUG, a->stream);
    } else if (b->want_output == 2) {  // (tx_idx is free again behind the compaction: it takes the corrected reads' lengths)
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(info + TXT_INFO_BUG), -1, 1, a->stream));
        e = bgr::launch_text_correct_sizes(a->dg, static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p), static_cast<const uint4*>(a->tx_rec.p),
                                           static_cast<const uint32_t*>(a->tx_accrec.p), n_acc, static_cast<uint32_t*>(a->tx_psz.p), static_cast<uint32_t*>(a->tx_nsz.p),
                                           static_cast<uint32_t*>(a->tx_idx.p), info + TXT_INFO_BUG, a->stream);
    } else {
        // sizes, offsets and bytes in one launch, into device buffers of the caller's capacities (at most twice the piece + 1 MB each: a piece whose
        // streams need more -- paths of very many unitigs -- is written by bgr_text_write_kernel from the offsets once the totals are known)
        pcap_dev = b->paths_out ? std::min<uint64_t>(b->paths_cap, 2ull * nbytes + (1ull << 20)) : 0;
        ncap_dev = b->notaligned_out ? std::min<uint64_t>(b->notaligned_cap, 2ull * nbytes + (1ull << 20)) : 0;
        HIP_TRY(a->tx_pout.ensure(pcap_dev + 64));
        HIP_TRY(a->tx_nout.ensure(ncap_dev + 64));
        e = bgr::launch_text_format(text, static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p), static_cast<const uint4*>(a->tx_rec.p),
                                    static_cast<const uint32_t*>(a->tx_accrec.p), n_acc, tickets + 1, a->tx_ticket[1], ++a->tx_epoch, chains, static_cast<uint32_t*>(a->tx_poff.p),
                                    static_cast<uint32_t*>(a->tx_noff.p), static_cast<uint8_t*>(a->tx_pout.p), static_cast<uint8_t*>(a->tx_nout.p), pcap_dev, ncap_dev, info, a->stream);
        if (n_acc && e == hipSuccess) a->tx_ticket[1] += bgr::format_tiles(n_acc);   // (as many tickets as workgroups ran: launch_text_format launches nothing for zero reads)
    }
    if (e == hipSuccess && b->want_output >= 2) e = bgr::launch_scan2_u32(static_cast<const uint32_t*>(a->tx_psz.p), static_cast<const uint32_t*>(a->tx_nsz.p), static_cast<uint32_t*>(a->tx_poff.p),
                                                   static_cast<uint32_t*>(a->tx_noff.p), n_acc, nullptr, sums2, info + TXT_INFO_PBYTES, info + TXT_INFO_NBYTES, a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("text size launches: ") + hipGetErrorString(e));
    uint32_t all[bgr::kSmallBytes / 4], h2[bgr::kCurWords];   // the cursor block and the info block lie in the same `small` buffer: one copy
    HIP_TRY(hipMemcpyAsync(all, a->small.p, sizeof(all), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    memcpy(h2, all, sizeof(h2));
    memcpy(h, all + (info - static_cast<const uint32_t*>(a->small.p)), sizeof(h));
    lap(2);
    if (h2[bgr::kCurOverflow]) return fail(BGR_E_INTERNAL, "path arena overflow (internal sizing error)");
    if (a->deep.open) {
        const bool handed_back = h2[bgr::list_word(bgr::List::kRetry)] != 0;
        rc = settle_launch(a, h2);
        if (rc != BGR_OK) return rc;
        if (handed_back) continue;  // sizes and offsets once more, from the final results
    }
    break;
    }
    if (b->want_output >= 2 && h[TXT_INFO_BUG] != 0xFFFFFFFFu) {  // a path that does not spell a walk: the reference prints "bug compaction" and exits
        b->irregular = 2;                                          // (aligner.cpp:280-283); the caller reproduces that on the host
        a->tx_n_acc = 0;
        return BGR_OK;
    }
    a->tx_pbytes = h[TXT_INFO_PBYTES];
    a->tx_nbytes = h[TXT_INFO_NBYTES];
    a->tx_written = b->want_output == 1 && a->tx_pbytes <= pcap_dev && a->tx_nbytes <= ncap_dev;   // (every workgroup's stretch ended below the capacities)
    const int frc = fetch_text_impl(a, b);
    lap(3);
    a->tx_phase_s[4] += 1;
    return frc;
}

int bgr_aligner_sync(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_sync: null aligner");
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return settle_launch_sync(a);  // (exhaustive mode: reads the last pass handed back are mapped before the results count as final)
}

int bgr_aligner_device_results(bgr_aligner* a, void** d_results, void** d_arena, void** d_cursor) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_device_results: null aligner");
    if (d_results) *d_results = a->results.p;
    if (d_arena) *d_arena = a->arena.p;
    if (d_cursor) *d_cursor = a->small.p;
    return BGR_OK;
}

// results -> CSR on the device in two steps: the number of path ints of the launch (fetch_total), then the dense arrays and
// their copies into the caller's memory (fetch_copy: relative path_offsets[0..n], status[0..n), total ints at paths_out)
static int fetch_total(bgr_aligner* a, uint64_t n, uint64_t* total_out) {
    HIP_TRY(hipSetDevice(a->device));
    if (a->deep.open) { const int src = settle_launch_sync(a); if (src != BGR_OK) return src; }
    else HIP_TRY(wait_stream(a));
    const uint64_t nb = (n + 4095) / 4096;
    HIP_TRY(a->csr_sums.ensure(nb * 4 + 64));
    HIP_TRY(a->csr_poffs.ensure((n + 1) * 8));
    HIP_TRY(a->csr_status.ensure(n));
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(static_cast<char*>(a->small.p) + bgr::kSmallCsrTotal);
    hipError_t e = bgr::launch_csr(static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p), (uint32_t)n,
                                   static_cast<uint32_t*>(a->csr_sums.p), d_total, nullptr, nullptr, nullptr, 0, 0, a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("csr launch: ") + hipGetErrorString(e));
    uint64_t hs[bgr::kSmallCsrTotal / 8 + 1];  // the cursor block at the start, the path-int total at the end
    HIP_TRY(hipMemcpyAsync(hs, a->small.p, sizeof(hs), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    const uint32_t* cur = reinterpret_cast<const uint32_t*>(hs);
    if (cur[bgr::kCurOverflow]) return fail(BGR_E_INTERNAL, "path arena overflow (internal sizing error)");
    *total_out = hs[bgr::kSmallCsrTotal / 8];
    return BGR_OK;
}
static int fetch_copy(bgr_aligner* a, uint64_t n, uint64_t total, int32_t* paths_out, uint64_t* path_offsets, uint8_t* status, bool with_end = true) {
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(static_cast<char*>(a->small.p) + bgr::kSmallCsrTotal);
    HIP_TRY(a->csr_paths.ensure(total * 4 + 16));
    hipError_t e = bgr::launch_csr(static_cast<const uint2*>(a->results.p), static_cast<const int32_t*>(a->arena.p), (uint32_t)n,
                                   static_cast<uint32_t*>(a->csr_sums.p), d_total, static_cast<unsigned long long*>(a->csr_poffs.p),
                                   static_cast<int32_t*>(a->csr_paths.p), static_cast<uint8_t*>(a->csr_status.p), (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull), 1, a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("csr launch: ") + hipGetErrorString(e));
    // (with_end = false: entry n, the end of the last read, is left to the caller -- it is the first entry of the next piece)
    HIP_TRY(hipMemcpyAsync(path_offsets, a->csr_poffs.p, (n + (with_end ? 1 : 0)) * 8, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipMemcpyAsync(status, a->csr_status.p, n, hipMemcpyDeviceToHost, a->stream));
    if (total) HIP_TRY(hipMemcpyAsync(paths_out, a->csr_paths.p, total * 4, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    return BGR_OK;
}

int bgr_aligner_path_stats(bgr_aligner* a, const void* d_reads, const void* d_read_offsets, uint64_t n, bgr_path_stat* out) {
    if (!a || (n && (!d_reads || !d_read_offsets || !out))) return fail(BGR_E_ARG, "bgr_aligner_path_stats: null argument");
    if (a->graph->header.has_exc)
        return fail(BGR_E_ARG, "bgr_aligner_path_stats: needs a graph of ACGT-only unitigs (the walk is read from the 2-bit store)");
    if (n != a->last_n) return fail(BGR_E_ARG, "bgr_aligner_path_stats: n_reads differs from the last bgr_align_device call");
    if (a->last_mode == BGR_MODE_EXHAUSTIVE) return fail(BGR_E_ARG, "bgr_aligner_path_stats: the last launch was exhaustive; paths of the greedy modes only");
    if (n == 0) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    static_assert(sizeof(bgr_path_stat) == 24, "six words per read, as the kernel writes them");
    HIP_TRY(a->path_stats.ensure(n * sizeof(bgr_path_stat)));
    hipError_t e = bgr::launch_path_stats(a->dg, static_cast<const uint8_t*>(d_reads), static_cast<const uint64_t*>(d_read_offsets), static_cast<const uint2*>(a->results.p),
                                          static_cast<const int32_t*>(a->arena.p), (uint32_t)n, static_cast<uint32_t*>(a->path_stats.p), a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("path stats launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out, a->path_stats.p, n * sizeof(bgr_path_stat), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    return BGR_OK;
}

int bgr_aligner_fetch(bgr_aligner* a, uint64_t n, int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status) {
    if (!a || !path_offsets || !status || (paths_cap && !paths_out)) return fail(BGR_E_ARG, "bgr_aligner_fetch: null argument");
    if (n != a->last_n) return fail(BGR_E_ARG, "bgr_aligner_fetch: n_reads differs from the last bgr_align_device call");
    path_offsets[0] = 0;
    if (n == 0) return BGR_OK;
    uint64_t total = 0;
    int rc = fetch_total(a, n, &total);
    if (rc != BGR_OK) return rc;
    if (total > paths_cap) return fail(BGR_E_CAPACITY, "bgr_aligner_fetch: paths_out too small");
    return fetch_copy(a, n, total, paths_out, path_offsets, status);
}

// One piece of a batch up to (not including) the copies out: H2D of the characters and offsets, the mapping launch.
static int batch_piece_launch(bgr_aligner* a, const bgr_params* p, const char* reads, const uint64_t* read_offsets, uint64_t n) {
    HIP_TRY(hipSetDevice(a->device));
    const uint64_t base = read_offsets[0], total = read_offsets[n] - base;
    uint32_t max_len = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t l = read_offsets[i + 1] - read_offsets[i];
        if (l > 0x7FFFFFFFull) return fail(BGR_E_ARG, "bgr_align_batch: read longer than 2^31 bases");
        max_len = std::max<uint32_t>(max_len, (uint32_t)l);
    }
    HIP_TRY(a->in_reads.ensure(total + 16));
    HIP_TRY(a->in_offs.ensure((n + 1) * 8));
    HIP_TRY(hipMemcpyAsync(a->in_reads.p, reads + base, total, hipMemcpyHostToDevice, a->stream));
    if (base == 0) {
        HIP_TRY(hipMemcpyAsync(a->in_offs.p, read_offsets, (n + 1) * 8, hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipStreamSynchronize(a->stream));
    } else {
        std::vector<uint64_t> rel(n + 1);
        for (uint64_t i = 0; i <= n; ++i) rel[i] = read_offsets[i] - base;
        HIP_TRY(hipMemcpyAsync(a->in_offs.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipStreamSynchronize(a->stream));
    }
    return bgr_align_device(a, p, a->in_reads.p, a->in_offs.p, n, total, max_len);
}

// A large batch in pieces on several streams (this aligner's and its twins', one host thread each): the copies of one piece run under the
// kernels of the others, and -- with more streams than two -- the link never waits for a stream that is busy fetching its results (two
// streams kept it 2/3 busy: 243 Mreads/s per 5 M-read call; kOverlapStreams = 4: see DESIGN 9).  A piece's place in paths_out is known
// once the pieces in front of it have counted their path ints (fetch_total); results are those of one launch over the whole batch.
static const uint64_t kOverlapMinReads = 512 * 1024;
static const unsigned kOverlapMaxStreams = 4, kOverlapMaxPieces = 2 * kOverlapMaxStreams;
static int align_batch_overlapped(bgr_aligner* a, const bgr_params* p, const char* reads, const uint64_t* read_offsets, uint64_t n,
                                  int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status) {
    unsigned n_streams = kOverlapMaxStreams;
    n_streams = (unsigned)std::min<int64_t>((int64_t)kOverlapMaxStreams, std::max<int64_t>(2, bgr::opt("overlap_streams")));  // (option overlap_streams: A/B measurements)
    const unsigned n_pieces = 2 * n_streams;
    bgr_aligner* al[kOverlapMaxStreams] = {a, nullptr, nullptr, nullptr};
    for (unsigned t = 1; t < n_streams; ++t) {  // the twins: a chain a -> twin -> twin's twin ..., created on first use
        bgr_aligner* prev = al[t - 1];
        if (!prev->twin) {
            int rc = bgr_aligner_create(a->graph, a->device, &prev->twin);
            if (rc != BGR_OK) return rc;
            prev->twin->is_twin = true;
        }
        bgr_aligner* tw = prev->twin;
        tw->cfg_waves = a->cfg_waves; tw->cfg_blocks_per_cu = a->cfg_blocks_per_cu; tw->cfg_lds_mphf = a->cfg_lds_mphf;
        tw->knob_frame_cap = a->knob_frame_cap; tw->knob_search = a->knob_search; tw->knob_debug_stop = a->knob_debug_stop;
        tw->knob_greedy_fast = a->knob_greedy_fast; tw->knob_exh_fast = a->knob_exh_fast; tw->knob_anc_fast = a->knob_anc_fast; tw->knob_memo_cap = a->knob_memo_cap; tw->knob_prepass = a->knob_prepass; tw->knob_no_events = a->knob_no_events;
        tw->knob_abundance_form = a->knob_abundance_form;
        tw->knob_links_form = a->knob_links_form;
        tw->pileup_tab = a->pileup_tab; tw->pileup_base_offs = a->pileup_base_offs; tw->pileup_on = a->pileup_on;   // (likewise)
        tw->pileup_fwd_tab = a->pileup_fwd_tab; tw->strands_on = a->strands_on;
        tw->links_tab = a->links_tab; tw->links_cap = a->links_cap; tw->links_bound = a->links_bound; tw->links_on = a->links_on;   // (one table for the aligner and its twins: the atomics are device-scope)
        if (tw->abundance_on != a->abundance_on) { const int rc = abundance_set(tw, a->abundance_on); if (rc != BGR_OK) return rc; }
        al[t] = tw;
    }
    uint64_t cut[kOverlapMaxPieces + 1];
    for (unsigned k = 0; k <= n_pieces; ++k) cut[k] = n * k / n_pieces;
    std::mutex mu;
    std::condition_variable cv;
    uint64_t totals[kOverlapMaxPieces];
    bool known[kOverlapMaxPieces];
    for (unsigned k = 0; k < n_pieces; ++k) { totals[k] = 0; known[k] = false; }
    int first_rc = BGR_OK;
    std::string first_err;
    auto give_up = [&](int rc, const char* msg) {
        std::lock_guard<std::mutex> l(mu);
        if (first_rc == BGR_OK) { first_rc = rc; first_err = msg ? msg : ""; }
        cv.notify_all();
    };
    auto work = [&](unsigned t) {
        for (unsigned k = t; k < n_pieces; k += n_streams) {
            { std::lock_guard<std::mutex> l(mu); if (first_rc != BGR_OK) return; }
            const uint64_t i0 = cut[k], cnt = cut[k + 1] - cut[k];
            uint64_t tot = 0;
            int rc = cnt ? batch_piece_launch(al[t], p, reads, read_offsets + i0, cnt) : BGR_OK;
            if (rc == BGR_OK && cnt) rc = fetch_total(al[t], cnt, &tot);
            if (rc != BGR_OK) { give_up(rc, bgr_last_error()); return; }
            uint64_t before = 0;
            {
                std::unique_lock<std::mutex> l(mu);
                totals[k] = tot;
                known[k] = true;
                cv.notify_all();
                cv.wait(l, [&] { if (first_rc != BGR_OK) return true; for (unsigned j = 0; j < k; ++j) if (!known[j]) return false; return true; });
                if (first_rc != BGR_OK) return;
                for (unsigned j = 0; j < k; ++j) before += totals[j];
            }
            if (before + tot > paths_cap) { give_up(BGR_E_CAPACITY, "bgr_align_batch: paths_out too small"); return; }
            if (cnt) {
                rc = fetch_copy(al[t], cnt, tot, paths_out ? paths_out + before : nullptr, path_offsets + i0, status + i0, false);
                if (rc != BGR_OK) { give_up(rc, bgr_last_error()); return; }
                if (before) for (uint64_t i = i0; i < i0 + cnt; ++i) path_offsets[i] += before;  // (entry i0 + cnt belongs to the next piece / the end)
            }
        }
    };
    std::vector<std::thread> helpers;
    try {
        for (unsigned t = 1; t < n_streams; ++t) helpers.emplace_back(work, t);
        work(0u);
    } catch (...) {  // (bad_alloc in a piece, or no thread to be had: the helpers that run must still be joined)
        give_up(BGR_E_INTERNAL, "bgr_align_batch: out of memory");
    }
    for (auto& h : helpers) h.join();
    if (first_rc != BGR_OK) return fail(first_rc, first_err);
    uint64_t all = 0;
    for (unsigned k = 0; k < n_pieces; ++k) all += totals[k];
    path_offsets[n] = all;
    a->last_n = 0;  // several launches: bgr_aligner_fetch has nothing to re-read
    return BGR_OK;
}

int bgr_align_batch(bgr_aligner* a, const bgr_params* p, const char* reads, const uint64_t* read_offsets, uint64_t n,
                    int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status) {
    if (!a || !p || !path_offsets || (n && (!reads || !read_offsets || !status))) return fail(BGR_E_ARG, "bgr_align_batch: null argument");
    path_offsets[0] = 0;
    a->last_n = 0;
    if (n == 0) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    const uint64_t base = read_offsets[0], total = read_offsets[n] - base;
    // One launch addresses its path arena with 32 bits: a batch beyond that (~13 M reads of 150 bp) is mapped in pieces.
    // (BGR_KNOB_BATCH_SPLIT_LIMIT: tests lower the limit to walk this path with small inputs)
    const uint64_t lim = a->knob_split_limit ? std::max<uint64_t>(4096, a->knob_split_limit) : 0xFFFFFFFFull - (256ull << 20);
    if (n > 1 && (2 * (total + 16 * n) >= lim || n >= 0x7FFFFFFFull)) {
        uint64_t w = 0;
        for (uint64_t i0 = 0; i0 < n;) {
            uint64_t i1 = i0 + 1;  // longest piece below half the limit (at least one read)
            while (i1 < n && 2 * ((read_offsets[i1 + 1] - read_offsets[i0]) + 16 * (i1 + 1 - i0)) < lim / 2 && i1 + 1 - i0 < (1ull << 30)) ++i1;
            int rc = bgr_align_batch(a, p, reads, read_offsets + i0, i1 - i0, paths_out ? paths_out + w : nullptr, paths_cap - w, path_offsets + i0, status + i0);
            if (rc != BGR_OK) return rc;
            const uint64_t got = path_offsets[i1];
            for (uint64_t i = i0; i <= i1; ++i) path_offsets[i] += w;
            w += got;
            i0 = i1;
        }
        a->last_n = 0;  // several launches: bgr_aligner_fetch has nothing to re-read
        return BGR_OK;
    }
    // a large batch: in pieces on two streams, copies under kernels (BGR_KNOB_BATCH_OVERLAP = 1 turns it off)
    if (!a->is_twin && !a->knob_overlap && n >= kOverlapMinReads) return align_batch_overlapped(a, p, reads, read_offsets, n, paths_out, paths_cap, path_offsets, status);
    int rc = batch_piece_launch(a, p, reads, read_offsets, n);
    if (rc != BGR_OK) return rc;
    return bgr_aligner_fetch(a, n, paths_out, paths_cap, path_offsets, status);
}

// ---- asynchronous form over host buffers ---------------------------------------------------------------------------------------
int bgr_align_batch_begin(bgr_aligner* a, const bgr_params* p, const char* reads, const uint64_t* read_offsets, uint64_t n, bgr_ticket* ticket) {
    if (!a || !p || !ticket || (n && (!reads || !read_offsets))) return fail(BGR_E_ARG, "bgr_align_batch_begin: null argument");
    if (a->ticket_open) return fail(BGR_E_ARG, "bgr_align_batch_begin: this aligner still has a batch in flight (wait for its ticket first)");
    ticket->aligner = a;
    ticket->n_reads = n;
    ticket->serial = ++a->ticket_serial;
    a->last_n = 0;
    if (n == 0) { a->ticket_open = true; return BGR_OK; }
    HIP_TRY(hipSetDevice(a->device));
    const uint64_t base = read_offsets[0], total = read_offsets[n] - base;
    if (n >= 0x7FFFFFFFull || 2 * (total + 16 * n) >= 0xFFFFFFFFull - (256ull << 20))
        return fail(BGR_E_ARG, "bgr_align_batch_begin: batch too large for one launch (2 * (bases + 16 * reads) must stay below 2^32 - 2^28); bgr_align_batch cuts such a batch");
    uint32_t max_len = 0;
    a->ticket_offs.resize(n + 1);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t l = read_offsets[i + 1] - read_offsets[i];
        if (l > 0x7FFFFFFFull) return fail(BGR_E_ARG, "bgr_align_batch_begin: read longer than 2^31 bases");
        max_len = std::max<uint32_t>(max_len, (uint32_t)l);
        a->ticket_offs[i] = read_offsets[i] - base;
    }
    a->ticket_offs[n] = total;
    HIP_TRY(a->in_reads.ensure(total + 16));
    HIP_TRY(a->in_offs.ensure((n + 1) * 8));
    HIP_TRY(hipMemcpyAsync(a->in_reads.p, reads + base, total, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(a->in_offs.p, a->ticket_offs.data(), (n + 1) * 8, hipMemcpyHostToDevice, a->stream));
    const int rc = bgr_align_device(a, p, a->in_reads.p, a->in_offs.p, n, total, max_len);
    if (rc != BGR_OK) return rc;
    a->ticket_open = true;
    return BGR_OK;
}

int bgr_align_batch_test(const bgr_ticket* t) {
    if (!t || !t->aligner) return fail(BGR_E_ARG, "bgr_align_batch_test: null ticket");
    bgr_aligner* a = t->aligner;
    if (!a->ticket_open || t->serial != a->ticket_serial) return fail(BGR_E_ARG, "bgr_align_batch_test: stale ticket");
    if (hipSetDevice(a->device) != hipSuccess) return fail(BGR_E_HIP, "hipSetDevice failed");
    const hipError_t e = hipStreamQuery(a->stream);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    return fail(BGR_E_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(e));
}

int bgr_align_batch_wait(const bgr_ticket* t, int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status) {
    if (!t || !t->aligner || !path_offsets) return fail(BGR_E_ARG, "bgr_align_batch_wait: null argument");
    bgr_aligner* a = t->aligner;
    if (!a->ticket_open || t->serial != a->ticket_serial) return fail(BGR_E_ARG, "bgr_align_batch_wait: stale ticket (every begin is waited for once, in order)");
    path_offsets[0] = 0;
    if (t->n_reads == 0) { a->ticket_open = false; return BGR_OK; }
    const int rc = bgr_aligner_fetch(a, t->n_reads, paths_out, paths_cap, path_offsets, status);
    if (rc != BGR_E_CAPACITY) a->ticket_open = false;  // (too small a paths buffer: the results stay, wait again with a larger one)
    return rc;
}

int bgr_aligner_counters(bgr_aligner* a, uint64_t out[5]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_counters: null argument");
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    { const int src = settle_launch_sync(a); if (src != BGR_OK) return src; }  // (exhaustive mode: reads the last pass handed back are mapped -- and counted -- first)
    HIP_TRY(hipMemcpy(out, static_cast<char*>(a->small.p) + bgr::kSmallCounters, bgr::kCounters * 8, hipMemcpyDeviceToHost));
    for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) {  // the pieces of overlapped batches its other streams mapped
        uint64_t t[bgr::kCounters];
        HIP_TRY(hipStreamSynchronize(tw->stream));
        { const int src = settle_launch_sync(tw); if (src != BGR_OK) return src; }
        HIP_TRY(hipMemcpy(t, static_cast<char*>(tw->small.p) + bgr::kSmallCounters, sizeof(t), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < bgr::kCounters; ++i) out[i] += t[i];
    }
    return BGR_OK;
}

int bgr_aligner_reset_counters(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_reset_counters: null aligner");
    HIP_TRY(hipSetDevice(a->device));
    // (on the aligner's own stream: a fill on the null stream is not ordered with a non-blocking stream's kernels)
    HIP_TRY(hipMemsetAsync(static_cast<char*>(a->small.p) + bgr::kSmallCounters, 0, bgr::kCounters * 8, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) {
        HIP_TRY(hipMemsetAsync(static_cast<char*>(tw->small.p) + bgr::kSmallCounters, 0, bgr::kCounters * 8, tw->stream));
        HIP_TRY(hipStreamSynchronize(tw->stream));
    }
    return BGR_OK;
}

int bgr_aligner_kernel_time(bgr_aligner* a, uint64_t* launches, double* total_ms) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_kernel_time: null aligner");
    HIP_TRY(hipSetDevice(a->device));
    int rc = drain_timers(a);
    if (rc != BGR_OK) return rc;
    if (launches) *launches = a->t_launches;
    if (total_ms) *total_ms = a->t_ms;
    for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) {  // the pieces of overlapped batches its other streams mapped
        rc = drain_timers(tw);
        if (rc != BGR_OK) return rc;
        if (launches) *launches += tw->t_launches;
        if (total_ms) *total_ms += tw->t_ms;
    }
    return BGR_OK;
}

int bgr_aligner_kernel_times(bgr_aligner* a, uint64_t* launches, double slot_ms[8], const char* slot_names[8]) {
    if (!a || !slot_ms) return fail(BGR_E_ARG, "bgr_aligner_kernel_times: null argument");
    HIP_TRY(hipSetDevice(a->device));
    int rc = drain_timers(a);
    if (rc != BGR_OK) return rc;
    if (launches) *launches = a->t_launches;
    for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) {
        rc = drain_timers(tw);
        if (rc != BGR_OK) return rc;
        if (launches) *launches += tw->t_launches;
    }
    for (int j = 0; j < kTimerSlots; ++j) {
        slot_ms[j] = a->t_slot_ms[j];
        const char* name = a->t_slot_name[j];
        for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) {  // (all streams run the same launch sequence: slot j is the same kernel)
            if (tw->t_slot_ms[j] <= 0) continue;
            slot_ms[j] += tw->t_slot_ms[j];
            if (!name) name = tw->t_slot_name[j];
        }
        if (slot_names) slot_names[j] = slot_ms[j] > 0 ? name : nullptr;
    }
    return BGR_OK;
}

int bgr_aligner_reset_kernel_time(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_reset_kernel_time: null aligner");
    HIP_TRY(hipSetDevice(a->device));
    int rc = drain_timers(a);
    if (rc != BGR_OK) return rc;
    a->t_launches = 0;
    a->t_ms = 0;
    for (double& x : a->t_slot_ms) x = 0;
    if (a->twin) return bgr_aligner_reset_kernel_time(a->twin);
    return BGR_OK;
}

int bgr_aligner_launch_info(bgr_aligner* a, uint32_t out[4]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_launch_info: null argument");
    memcpy(out, a->last_launch, sizeof(a->last_launch));
    return BGR_OK;
}

#ifdef BGR_PHASE_TIMING
// diagnostic builds only (not part of include/bgreat_gpu.h): the last launch's per-wave time stamps, four u64 per wave (100 MHz ticks)
int bgr_debug_wave_times(bgr_aligner* a, uint64_t* out, uint64_t cap_waves, uint64_t* n_waves) {
    if (!a || !n_waves) return BGR_E_ARG;
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    *n_waves = a->wave_times_n;
    const uint64_t n = std::min(cap_waves, a->wave_times_n);
    if (n && out) HIP_TRY(hipMemcpy(out, a->wave_times.p, n * 32, hipMemcpyDeviceToHost));
    return BGR_OK;
}
// the greedy multi kernel's anchor-scan counts per wave of the last launch: {scan steps, items scanned, groups of items, 0}
int bgr_debug_scan_counts(bgr_aligner* a, uint64_t* out, uint64_t cap_waves, uint64_t* n_waves) {
    if (!a || !n_waves) return BGR_E_ARG;
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    *n_waves = a->wave_times_n;
    const uint64_t n = std::min(cap_waves, a->wave_times_n);
    if (n && out) HIP_TRY(hipMemcpy(out, static_cast<const char*>(a->wave_times.p) + a->wave_times_n * 32, n * 32, hipMemcpyDeviceToHost));
    return BGR_OK;
}
#endif

int bgr_aligner_last_pass_runs(const bgr_aligner* a, uint32_t* runs, uint32_t* memo_cap) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_last_pass_runs: null aligner");
    if (runs) *runs = a->deep.runs;
    if (memo_cap) *memo_cap = a->deep.memo_cap;
    return BGR_OK;
}

int bgr_aligner_pass_counts(bgr_aligner* a, uint32_t out[4]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_pass_counts: null argument");
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    uint32_t cur[bgr::kCurWords];
    HIP_TRY(hipMemcpy(cur, a->small.p, sizeof(cur), hipMemcpyDeviceToHost));
    static_assert(bgr::kCurFollowUps == bgr::list_word(bgr::List::kSearch), "out[0]: greedy mode's follow-up items, exhaustive mode's first list");
    out[0] = cur[bgr::kCurFollowUps]; out[1] = cur[bgr::list_word(bgr::List::kDepthFirst)];
    out[2] = cur[bgr::list_word(bgr::List::kFirst)]; out[3] = cur[bgr::list_word(bgr::List::kGeneral)];
    return BGR_OK;
}

int bgr_device_local_cpus(int device, char* cpulist_out, uint64_t cap) {
    if (!cpulist_out || cap < 2) return fail(BGR_E_ARG, "bgr_device_local_cpus: null argument");
    char bus[64];
    HIP_TRY(hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device));
    for (char* c = bus; *c; ++c) *c = (char)tolower(*c);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/local_cpulist";
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return fail(BGR_E_IO, "bgr_device_local_cpus: cannot read " + path);
    const size_t got = fread(cpulist_out, 1, (size_t)cap - 1, f);
    fclose(f);
    cpulist_out[got] = 0;
    for (size_t i = 0; i < got; ++i) if (cpulist_out[i] == '\n') cpulist_out[i] = 0;
    if (!cpulist_out[0]) return fail(BGR_E_IO, "bgr_device_local_cpus: empty cpulist");
    return BGR_OK;
}

int bgr_device_alloc(int device, uint64_t bytes, void** out) {
    if (!out) return fail(BGR_E_ARG, "bgr_device_alloc: null argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
    return BGR_OK;
}
int bgr_device_free(int device, void* p) {
    if (!p) return BGR_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(p));
    return BGR_OK;
}
int bgr_device_upload(int device, void* dst_device, const void* src_host, uint64_t bytes) {
    if (bytes && (!dst_device || !src_host)) return fail(BGR_E_ARG, "bgr_device_upload: null argument");
    HIP_TRY(hipSetDevice(device));
    if (bytes) { HIP_TRY(hipMemcpy(dst_device, src_host, bytes, hipMemcpyHostToDevice)); HIP_TRY(hipStreamSynchronize(nullptr)); }  // (the callers' kernels run on non-blocking streams)
    return BGR_OK;
}
int bgr_device_download(int device, void* dst_host, const void* src_device, uint64_t bytes) {
    if (bytes && (!dst_host || !src_device)) return fail(BGR_E_ARG, "bgr_device_download: null argument");
    HIP_TRY(hipSetDevice(device));
    if (bytes) HIP_TRY(hipMemcpy(dst_host, src_device, bytes, hipMemcpyDeviceToHost));
    return BGR_OK;
}

// Page-locked host memory.  hipHostMalloc pins 4 KB pages at ~4.4 GB/s on this platform, from any number of threads; an anonymous
// mapping with transparent huge pages asked for, touched once per 2 MB and then registered pins at ~26 GB/s (tools/ubench/pin_alloc.hip) --
// bgr_align_all takes ~0.7 GB of staging sets while its pipeline ramps up, 0.17 s of a 0.6 s run of 100 M reads.  Buffers of 2 MB and
// more go that way (hipHostMalloc when anything in it fails); the registry tells bgr_host_free how a pointer was obtained.
// (never destroyed: the pipeline's cache of staging sets frees its buffers from a static destructor of its own, in whatever order)
static std::mutex& g_host_m = *new std::mutex;
static std::map<void*, uint64_t>& g_host_mapped = *new std::map<void*, uint64_t>;  // registered anonymous mappings: pointer -> mapped bytes

int bgr_host_alloc(uint64_t bytes, void** out) {
    if (!out) return fail(BGR_E_ARG, "bgr_host_alloc: null argument");
    void* p = nullptr;
    if (bytes >= (2ull << 20) && bgr::opt("huge_pinned")) {
        const uint64_t len = (bytes + (2ull << 20) - 1) & ~((2ull << 20) - 1);
        void* m = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m != MAP_FAILED) {
            (void)madvise(m, len, MADV_HUGEPAGE);
            for (uint64_t o = 0; o < len; o += 2ull << 20) static_cast<volatile char*>(m)[o] = 0;  // fault the (huge) pages in before they are pinned
            if (hipHostRegister(m, len, hipHostRegisterDefault) == hipSuccess) {
                std::lock_guard<std::mutex> l(g_host_m);
                g_host_mapped[m] = len;
                *out = m;
                return BGR_OK;
            }
            (void)hipGetLastError();
            munmap(m, len);
        }
    }
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    *out = p;
    return BGR_OK;
}

int bgr_host_free(void* p) {
    if (!p) return BGR_OK;
    uint64_t len = 0;
    {
        std::lock_guard<std::mutex> l(g_host_m);
        auto it = g_host_mapped.find(p);
        if (it != g_host_mapped.end()) { len = it->second; g_host_mapped.erase(it); }
    }
    if (len) {
        hipError_t e = hipHostUnregister(p);
        munmap(p, len);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("hipHostUnregister: ") + hipGetErrorString(e));
        return BGR_OK;
    }
    hipError_t e = hipHostFree(p);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("hipHostFree: ") + hipGetErrorString(e));
    return BGR_OK;
}

// ---- read files / output records (host) ---------------------------------------------------------------
struct bgr_readset { bgr::ReadSet rs; };

int bgr_readset_load(const char* path, int fastq, uint32_t k, bgr_readset** out) {
    return bgr_readset_load_parallel(path, fastq, k, 1, 0, out);
}

int bgr_readset_load_parallel(const char* path, int fastq, uint32_t k, uint32_t threads, uint64_t chunk_bytes, bgr_readset** out) {
    if (!path || !out) return fail(BGR_E_ARG, "bgr_readset_load: null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(BGR_E_IO, std::string("cannot open read file ") + path);
    std::vector<char> buf;
    char tmp[1 << 16];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    fclose(f);
    bgr_readset* r = new bgr_readset();
    r->rs.clear();
    bgr::parse_reads_parallel(buf.data(), buf.size(), fastq != 0, k, threads ? threads : 1, chunk_bytes ? chunk_bytes : (8u << 20), r->rs);
    *out = r;
    return BGR_OK;
}
uint64_t bgr_readset_count(const bgr_readset* rs) { return rs ? rs->rs.count() : 0; }
int bgr_readset_view(const bgr_readset* rs, const char** reads, const uint64_t** read_offsets, const char** headers, const uint64_t** header_offsets) {
    if (!rs) return fail(BGR_E_ARG, "bgr_readset_view: null readset");
    if (reads) *reads = rs->rs.reads.data();
    if (read_offsets) *read_offsets = rs->rs.read_offs.data();
    if (headers) *headers = rs->rs.headers.data();
    if (header_offsets) *header_offsets = rs->rs.header_offs.data();
    return BGR_OK;
}
void bgr_readset_destroy(bgr_readset* rs) { delete rs; }

int bgr_write_records(void* paths_file, void* notaligned_file, uint64_t n, const char* headers, const uint64_t* hoffs,
                      const char* reads, const uint64_t* roffs, const int32_t* paths, const uint64_t* poffs) {
    if (!paths_file || !notaligned_file || (n && (!headers || !hoffs || !reads || !roffs || !poffs))) return fail(BGR_E_ARG, "bgr_write_records: null argument");
    FILE* pf = static_cast<FILE*>(paths_file);
    FILE* nf = static_cast<FILE*>(notaligned_file);
    std::string pbuf, nbuf;
    pbuf.reserve(1 << 20);
    nbuf.reserve(1 << 20);
    char num[16];
    for (uint64_t i = 0; i < n; ++i) {
        const char* h = headers + hoffs[i];
        size_t hn = hoffs[i + 1] - hoffs[i];
        if (poffs[i + 1] > poffs[i]) {  // alignerGreedy.cpp:406-411 + printPath aligner.cpp:600-609
            pbuf.append(h, hn);
            pbuf.push_back('\n');
            for (uint64_t j = poffs[i]; j < poffs[i + 1]; ++j) {
                int32_t v = paths[j];
                uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
                int len = 0;
                do { num[len++] = (char)('0' + u % 10); u /= 10; } while (u);
                if (v < 0) pbuf.push_back('-');
                while (len) pbuf.push_back(num[--len]);
                pbuf.push_back('.');
            }
            pbuf.push_back('\n');
            if (pbuf.size() > (1 << 20) - 4096) { if (fwrite(pbuf.data(), 1, pbuf.size(), pf) != pbuf.size()) return fail(BGR_E_IO, "write to paths file failed"); pbuf.clear(); }
        } else {  // alignerGreedy.cpp:421-427
            nbuf.append(h, hn);
            nbuf.push_back('\n');
            nbuf.append(reads + roffs[i], roffs[i + 1] - roffs[i]);
            nbuf.push_back('\n');
            if (nbuf.size() > (1 << 20) - 4096) { if (fwrite(nbuf.data(), 1, nbuf.size(), nf) != nbuf.size()) return fail(BGR_E_IO, "write to notAligned file failed"); nbuf.clear(); }
        }
    }
    if (!pbuf.empty() && fwrite(pbuf.data(), 1, pbuf.size(), pf) != pbuf.size()) return fail(BGR_E_IO, "write to paths file failed");
    if (!nbuf.empty() && fwrite(nbuf.data(), 1, nbuf.size(), nf) != nbuf.size()) return fail(BGR_E_IO, "write to notAligned file failed");
    return BGR_OK;
}

}  // extern "C"
