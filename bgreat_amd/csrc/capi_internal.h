// capi_internal.h -- what the units of the C-ABI share (capi.hip: index, distribution, mapping, text route, batches; capi_abundance.hip,
// capi_links.hip, capi_triples.hip, capi_bubbles.hip, capi_blocks.hip, capi_haplotypes.hip, capi_pileup.hip, capi_variants.hip: the counting features): the objects behind the opaque handles, the error channel, the
// waits, and the few functions that cross units.  Nothing in here is part of the interface (include/bgreat_gpu.h) or leaves the library.
#ifndef BGREAT_AMD_CAPI_INTERNAL_H
#define BGREAT_AMD_CAPI_INTERNAL_H

#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bgreat_gpu.h"
#include "abundance_kernels.h"
#include "align_kernels.h"
#include "graph_build.h"
#include "launch_plan.h"
#include "options.h"

namespace bgr {
int set_error(int code, const std::string& msg);  // capi.hip: the one definition, with the thread's message that bgr_last_error returns (pipeline.cpp calls it too)
}

#pragma GCC visibility push(hidden)

inline int fail(int code, const std::string& msg) { return bgr::set_error(code, msg); }
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(BGR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

const int kTimerRing = 64;   // launches between two drains of the timers
const int kTimerSlots = 8;   // kernels of one launch timed separately (pre-pass, passes)

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
    // bubbles (bgr_graph_bubbles_enable): the sticky switch with its threshold; the device of the first aligner a run collected (-1: none yet), where
    // the run's merged links are called when it ends; the records of the last successful run and the threshold they were called with
    bool bubbles_on = false, bubbles_valid = false;
    uint64_t bubbles_min_link = 1, bubbles_called = 0;
    int bubbles_device = -1;
    std::vector<bgr_bubble> bubbles;
    // triples (bgr_graph_triples_enable): as the links -- the sticky switch, the bound of distinct triples (from the host blob, the first time it is asked
    // for), the totals of the last bgr_align_all with the switch on: {k0, k1, count} as the aligners delivered them until the run ends, then merged and sorted
    struct TripleRow { uint64_t k0, k1, count; };
    bool triples_on = false, triples_valid = false, triples_bound_known = false;
    uint64_t triples_bound = 0;
    std::vector<TripleRow> triples;
    // phase (bgr_graph_phase_enable): the sticky switch with the threshold its bubbles are called with when the bubbles' own switch is off; the records
    // of the last successful run
    bool phase_on = false, phase_valid = false;
    uint64_t phase_min_link = 1;
    std::vector<bgr_phase> phase;
    // blocks (bgr_graph_blocks_enable): the sticky switch with the threshold of a decided link, and the threshold the run's bubbles are called with when
    // neither the bubbles' nor the phase's own switch is on; the entries of the last successful run
    bool blocks_on = false, blocks_valid = false;
    uint64_t blocks_min_link = 1, blocks_min_phase = 1;
    std::vector<bgr_block_entry> blocks;
    // haplotypes (bgr_graph_haplotypes_enable): the sticky switch with the smallest block that is spelled, and the thresholds the run's bubbles and blocks
    // are called with when no switch before it in the chain (bubbles, phase, blocks) is on; the records and characters of the last successful run
    bool haplotypes_on = false, haplotypes_valid = false;
    uint64_t haplotypes_min_link = 1, haplotypes_min_phase = 1, haplotypes_min_block = 1;
    std::vector<bgr_haplotype> haplotypes;
    std::vector<char> haplotypes_seq;
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
    uint64_t last_arena_cap = 0, last_total_bases = 0;   // its arena's ints and its reads' bases (the counting kernels behind bgr_aligner_path_stats: test.count_with_path_stats)
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
    uint32_t knob_no_jump = 0;      // BGR_KNOB_GREEDY_JUMP
    uint32_t knob_overlap = 0;      // BGR_KNOB_BATCH_OVERLAP
    uint32_t knob_abundance_form = 0;  // BGR_KNOB_ABUNDANCE_FORM
    bool abundance_on = false;      // bgr_aligner_abundance_enable: every greedy / anchors launch is followed by the abundance kernel
    DevBuf abundance;               // u64[n_unitigs + 1][3], allocated and zeroed on the first enable
    uint32_t knob_links_form = 0;   // BGR_KNOB_LINKS_FORM
    bool links_on = false;          // bgr_aligner_links_enable: every greedy / anchors launch is followed by the links kernel
    DevBuf links;                   // {u64 key, u64 count}[links_cap] + the tail words (links_kernels.h), allocated and zeroed on the first enable
    unsigned long long* links_tab = nullptr;   // the table this aligner's launches add to: its own, or (a twin) the one of the aligner it belongs to
    uint64_t links_cap = 0, links_bound = 0;
    bool triples_on = false;        // bgr_aligner_triples_enable: every greedy / anchors launch is followed by the triples kernel
    DevBuf triples;                 // {u64 k0, u64 k1, u64 count}[triples_cap] + the tail words (triples_kernels.h), allocated and zeroed on the first enable
    unsigned long long* triples_tab = nullptr;   // the table this aligner's launches add to: its own, or (a twin) the one of the aligner it belongs to
    uint64_t triples_cap = 0, triples_bound = 0;
    bool pileup_on = false;         // bgr_aligner_pileup_enable: every greedy / anchors launch is followed by the pileup kernel
    DevBuf pileup, pileup_offs;     // the table (pileup_kernels.h) and base_offs, allocated, zeroed / uploaded on the first enable
    uint32_t* pileup_tab = nullptr;             // the table this aligner's launches add to: its own, or (a twin) the one of the aligner it belongs to
    const uint64_t* pileup_base_offs = nullptr;
    bool strands_on = false;        // bgr_aligner_pileup_strands_enable: the pileup kernel also adds the forward observations to a second table
    DevBuf pileup_fwd;              // that table: the layout of `pileup`, its tail stays 0
    uint32_t* pileup_fwd_tab = nullptr;   // as pileup_tab: its own, or (a twin) the one of the aligner it belongs to
    DevBuf var_scratch, var_out, var_stage;   // bgr_aligner_pileup_sites: the passes' tile arrays and the records; bgr_aligner_pileup_add: the staging piece
    double var_ms[5] = {0, 0, 0, 0, 0};       // the last call's five launches
    double bub_ms[4] = {0, 0, 0, 0};          // bgr_aligner_bubbles: the last call's four launches
    bgr_aligner* twin = nullptr;    // second stream + buffers: the overlapped form of bgr_align_batch, un-waited consecutive bgr_align_device launches (created on first use)
    bool is_twin = false;
    uint32_t knob_device_overlap = 0;   // BGR_KNOB_DEVICE_OVERLAP
    bgr_aligner* holder = nullptr;  // who took this aligner's last mapping launch: null = itself, else its twin (launch_taker.h); "the last launch" is read there
    int num_cus = 0;
    size_t lds_per_cu = 0;
    hipEvent_t ev[kTimerRing][kTimerSlots + 1];  // ev[i][0] = start of launch i, ev[i][j] = behind its j-th kernel
    int ev_marks[kTimerRing];                    // kernels timed in launch i
    int ev_used = 0;
    uint64_t t_launches = 0;
    double t_ms = 0, t_slot_ms[kTimerSlots] = {0, 0, 0, 0, 0, 0, 0, 0};
    const char* t_slot_name[kTimerSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

// Wait for the aligner's stream.  By default hipStreamSynchronize (the runtime spins: lowest latency, one busy CPU per waiting thread);
// with BGREAT_BLOCKING_SYNC=1 an event made with hipEventBlockingSync is recorded and waited for instead: the thread sleeps until the
// interrupt, so more stream workers per device than CPUs to spare can overlap their calls (bgr_align_all's text route).
inline hipError_t wait_stream(bgr_aligner* a) {
    if (!a->blocking_sync) return hipStreamSynchronize(a->stream);
    hipError_t e = hipEventRecord(a->ev_wait, a->stream);
    return e == hipSuccess ? hipEventSynchronize(a->ev_wait) : e;
}
// Wait for every stream that adds to the aligner's tables: its own and its twins'.
inline int sync_all(bgr_aligner* a) {
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) HIP_TRY(hipStreamSynchronize(x->stream));
    return BGR_OK;
}

// The aligner whose buffers hold the last mapping launch: the aligner itself, or its twin when that took it (bgr_align_device, launch_taker.h).
inline bgr_aligner* holder_of(bgr_aligner* a) { return a->holder ? a->holder : a; }
inline const bgr_aligner* holder_of(const bgr_aligner* a) { return a->holder ? a->holder : a; }

// ---- the functions that cross units --------------------------------------------------------------------------------------------
// capi_abundance.hip
int abundance_set(bgr_aligner* a, bool on);   // this one aligner's (or twin's) switch; the table is allocated and zeroed the first time
bgr::AbundancePlan abundance_plan_of(const bgr_aligner* a, uint64_t n_reads, uint64_t total_bases);   // geometry and form of the abundance kernel behind a launch of this size
// capi_links.hip
void links_share(bgr_aligner* a);   // the twins add to the aligner's table of links: its fields copied to each of them
int links_tail(bgr_aligner* a, const char* who, uint64_t* tail);   // the three words behind the aligner's table, every stream that adds to it waited for; BGR_E_ARG when links were never enabled, BGR_E_CAPACITY when the table has overflowed
void run_links_begin(bgr_graph* g);                   // a whole run (run_counts.h): the totals of the run before are gone,
int run_links_collect(bgr_graph* g, bgr_aligner* a);  // ... an aligner's table joins the run's,
void run_links_end(bgr_graph* g, bool ok);            // ... sorted and merged; totals only of a run that ended well
// capi_triples.hip
void triples_share(bgr_aligner* a);   // the twins add to the aligner's table of triples: its fields copied to each of them
void run_triples_begin(bgr_graph* g);                   // a whole run (run_counts.h), as the links';
int run_triples_collect(bgr_graph* g, bgr_aligner* a);  // ... an aligner's table joins the run's,
void run_triples_end(bgr_graph* g, bool ok);            // ... sorted and merged; totals only of a run that ended well
void run_phase_begin(bgr_graph* g);
int run_phase_end(bgr_graph* g, bool ok);               // ... behind the bubbles' and the triples' end: the run's bubbles joined with its triples on the host
// capi_blocks.hip
void run_blocks_begin(bgr_graph* g);
int run_blocks_end(bgr_graph* g, bool ok);              // ... behind the phase's end: the run's bubbles and phase records uploaded once, chained on the device, the entries kept
// capi_haplotypes.hip
void run_haplotypes_begin(bgr_graph* g);
int run_haplotypes_end(bgr_graph* g, bool ok);          // ... behind the blocks' end: the run's bubbles and entries uploaded once, spelled from the resident graph, records and bytes kept
// capi_bubbles.hip
void run_bubbles_begin(bgr_graph* g);                   // a whole run (run_counts.h), as the links';
void run_bubbles_collect(bgr_graph* g, bgr_aligner* a); // ... the first aligner's device is where the run's links will be called,
int run_bubbles_end(bgr_graph* g, bool ok);             // ... behind the links' end: the merged links uploaded once, the four passes, the records kept
// capi_pileup.hip
void pileup_share(bgr_aligner* a);   // the twins add to the aligner's pileup tables: its fields copied to each of them
int pileup_guard(const bgr_unitig_abundance* rows, uint64_t n, const char* who);   // BGR_E_CAPACITY when a reads column reached 2^32: a depth may have wrapped
int guarded_sync(bgr_aligner* a, const char* who);   // the aligner's abundance snapshot through pileup_guard, then sync_all
int graph_base_offs(bgr_graph* g, const char* who);  // g->base_offs (prefix sums of the unitig lengths) made, once per graph
int pileup_refusal(const bgr_graph* g, const char* who);   // BGR_E_ARG on a graph whose unitigs are not ACGT only
void run_pileup_begin(bgr_graph* g);                   // a whole run (run_counts.h), as the links';
int run_pileup_collect(bgr_graph* g, bgr_aligner* a);  // ... the pileup switch gathers on the host, the variants switch on a device
int run_pileup_end(bgr_graph* g, bool ok);             // ... behind the abundance's end: BGR_E_CAPACITY when a depth may have wrapped
// capi_variants.hip
int variants_collect(bgr_graph* g, bgr_aligner* a);   // a run's aligner: the first one's tables become the run's (g->variants_run), the others' are added
int variants_end(bgr_graph* g, bool ok);              // the run's end: the sites called once from the run's table, which is freed whatever happens
void variants_run_free(bgr_graph* g);                 // g->variants_run and its device memory released

#pragma GCC visibility pop

#endif
