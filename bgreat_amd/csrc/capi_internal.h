// capi_internal.h -- what the units of the C-ABI share (capi.hip: index, distribution, mapping, batches; capi_text.hip: the text route; the counting features:
// capi_abundance.hip with the table of a run's stages, capi_links.hip with the count tables of links and triples, capi_triples.hip with the phase,
// capi_bubbles.hip, capi_blocks.hip, capi_haplotypes.hip, capi_haplotag.hip, capi_pileup.hip, capi_variants.hip): the objects behind the opaque handles, the error
// channel, the waits, the helpers the counting features are written with (delivering rows, the chain's switches and thresholds, a file of lines,
// a call's stream and buffers), and the few functions that cross units.  Nothing in here is part of the interface (include/bgreat_gpu.h) or
// leaves the library.
#ifndef BGREAT_AMD_CAPI_INTERNAL_H
#define BGREAT_AMD_CAPI_INTERNAL_H

#include <hip/hip_runtime.h>

#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bgreat_gpu.h"
#include "abundance_kernels.h"
#include "align_kernels.h"
#include "pileup_kernels.h"
#include "graph_build.h"
#include "inside_index.h"
#include "launch_plan.h"
#include "options.h"
#include "text_epochs.h"

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

// What a counting feature keeps in the graph object: the rows of the last successful run.
template <class Row>
struct RunRows {
    bool valid = false;
    std::vector<Row> rows;
    void forget() { std::vector<Row>().swap(rows); valid = false; }   // (nothing stays allocated)
};
// ... of a count table (links: W = 2, triples: W = 3): the key words, then the count
template <size_t W>
struct CountRows : RunRows<std::array<uint64_t, W>> {
    bool on = false, bound_known = false;
    uint64_t bound = 0;
};
// ... and the sticky switch of a feature of the chain bubbles -> phase -> blocks -> haplotypes with the thresholds it was given (1 where it takes none)
struct ChainMins { uint64_t link = 1, phase = 1, block = 1; };
struct ChainSwitch {
    bool on = false;
    ChainMins min;
    void set(uint32_t on_, const ChainMins& given) { if (on_) min = given; on = on_ != 0; }
};

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
    // The counting features whose rows a run leaves here (RunRows above): `on` is the sticky switch, `rows` with `valid` those of the last successful
    // bgr_align_all with the feature counted.  Every access is under abundance_m.
    // links and triples (bgr_graph_links_enable, bgr_graph_triples_enable): {key, count} and {k0, k1, count} as the aligners delivered them until the run
    // ends, then merged and sorted; the bound of distinct keys is computed from the host blob the first time it is asked for
    CountRows<2> links;
    CountRows<3> triples;
    // bubbles, phase, blocks, haplotypes (bgr_graph_*_enable): each switch with the thresholds it was given (run_thresholds below says which of them a
    // run uses).  bubbles.device: the device of the first aligner a run collected (-1: none yet), where the run's merged links are called when it ends
    // and the later stages of the chain run; haplotypes.seq: the characters the records point into
    // haplotags (bgr_graph_haplotag_enable): the sticky switch and the graph's copy of the tag table, n_unitigs + 1 words
    bool haplotag_on = false;
    bool exhaustive_paths_on = false;   // bgr_graph_exhaustive_paths_enable: sticky -- a later bgr_align_all in exhaustive mode writes GAF lines and counts, every aligner of it with the switch
    bool gaf_cs_on = false;   // bgr_graph_gaf_cs_enable: sticky -- the GAF lines of every later bgr_align_all end in the cs:Z: field
    std::vector<uint32_t> haplotag;
    struct Bubbles : ChainSwitch, RunRows<bgr_bubble> { int device = -1; } bubbles;
    struct Phase : ChainSwitch, RunRows<bgr_phase> {} phase;
    struct Blocks : ChainSwitch, RunRows<bgr_block_entry> {} blocks;
    struct Haplotypes : ChainSwitch, RunRows<bgr_haplotype> {
        std::vector<char> seq;
        void forget() { RunRows<bgr_haplotype>::forget(); std::vector<char>().swap(seq); }
    } haplotypes;
    // the re-compaction (bgr_graph_recompact_enable): the sticky switch with its threshold, the device of the first aligner a run collected (-1: none yet), and
    // the chains of the last successful run: records, the walks' oriented ids, the characters
    struct Recompact : RunRows<bgr_chain> {
        bool on = false;
        uint64_t min_reads = 1;
        int device = -1;
        std::vector<int32_t> walk;
        std::vector<char> seq;
        void forget() { RunRows<bgr_chain>::forget(); std::vector<int32_t>().swap(walk); std::vector<char>().swap(seq); }
    } recompact;
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
    // the inside index (bgr_graph_inside_build; inside_index.h): a buffer of its own on the host and, uploaded once per device that an aligner with the
    // pass enabled lives on, in HBM (inside_dev, under abundance_m) -- never part of the blob.  inside_on: the sticky switch of whole runs,
    // inside_run: what the aligners of the last bgr_align_all mapped inside
    bgr::InsideIndex inside;
    std::map<int, void*> inside_dev;
    bool inside_on = false;
    uint64_t inside_run = 0;
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
    template <class T> T* as() const { return static_cast<T*>(p); }   // the buffer as an array of T
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

// The text route's state in an aligner (capi_text.hip: bgr_align_fasta_text, bgr_aligner_fetch_text): the piece, its records, the formatted streams
struct TextRoute {
    DevBuf in, sums, state, rec, idx, accrec, accsrc, offs, psz, nsz, poff, noff, pout, nout, info, gaf;
    DevBuf tags;                    // GAF output of an aligner with a tag table: the tags per accepted read, next to gaf
    DevBuf cs;                      // GAF output with the cs:Z: field (bgr_aligner_gaf_cs_enable): the bytes of its ops per accepted read, next to gaf
    DevBuf idx_kept;                // GAF output with record info (exhaustive launches): idx as the parse launch left it -- the GAF sizes launch reuses idx, and the record info may be made twice
    uint64_t n_acc = 0, pbytes = 0, nbytes = 0;
    const uint8_t* text = nullptr;  // where the last call's piece lies in HBM (in, or the caller's stage)
    bgr::TextEpochs epochs;         // the one-launch kernels' chains (epoch of the last launch, tickets earlier launches took) and which of the two info blocks a piece uses
    bool written = false;           // the streams lie in pout / nout (the format launch wrote them: every stretch ended below the capacities)
    uint32_t want = 0;              // the piece's want_output (2 = correction mode: mapped reads as spelled by their paths, 3 = GAF lines)
    bool tagged = false;            // the sizes launch of the piece in the buffers was a tagged one (the write launch follows it)
    bool with_cs = false;           // ... was one of the instances that carry the cs:Z: field (the same)
    bool view = false;              // ... read an exhaustive launch through its view, launch.rows_view (bgr_aligner_exhaustive_paths_enable; the same)
    double phase_s[5] = {0, 0, 0, 0, 0};  // BGREAT_TIMING: host wall seconds to the call's four waits (mark, records, mapping + sizes, streams) + calls
    void release() {
        for (DevBuf* b : {&in, &sums, &state, &rec, &idx, &accrec, &accsrc, &offs, &psz, &nsz, &poff, &noff, &pout, &nout, &info, &gaf, &tags, &cs, &idx_kept}) b->release();
    }
};

// What a launch reads and writes on the device: the batch as it came in, its 2-bit planes, the rows, the lists the passes leave each other
struct LaunchBufs {
    DevBuf in_reads, in_offs, pk_fw3, pk_nm, pk_hasn, results, arena, ovf, ovf2, lst, deepbuf, retry, retry2, small;  // small: kSmall* (align_kernels.h)
    DevBuf wave_times;            // diagnostic builds only (-DBGR_PHASE_TIMING)
    DevBuf rows_view;             // bgr_aligner_exhaustive_paths_enable: 8 bytes per read, the rows of an exhaustive launch without their end offset (exhaustive_rows_kernels.h); allocated once the switch is on
    void release() { for (DevBuf* b : {&in_reads, &in_offs, &pk_fw3, &pk_nm, &pk_hasn, &results, &arena, &ovf, &ovf2, &lst, &deepbuf, &retry, &retry2, &small, &wave_times, &rows_view}) b->release(); }
};
// What reads the rows of the last launch back: the dense arrays of a fetch, bgr_aligner_path_stats, bgr_aligner_path_diffs
struct FetchBufs {
    DevBuf csr_sums, csr_poffs, csr_status, csr_paths, path_stats;
    DevBuf path_diffs;            // counts and offsets (two arrays of n + 1 words each way), then the differences
    void release() { for (DevBuf* b : {&csr_sums, &csr_poffs, &csr_status, &csr_paths, &path_stats, &path_diffs}) b->release(); }
};
// haplotags (bgr_aligner_haplotag_enable): the tag table on the device (null: off), the tags of the last call of bgr_aligner_haplotags
struct HaplotagBufs { DevBuf table, out; void release() { table.release(); out.release(); } };
// bgr_aligner_pileup_sites: the passes' tile arrays and the records; bgr_aligner_pileup_add: the staging piece
struct VariantBufs { DevBuf scratch, out, stage; void release() { scratch.release(); out.release(); stage.release(); } };

// links and triples (bgr_aligner_links_enable, bgr_aligner_triples_enable): every greedy / anchors launch is followed by the kernel that adds to the
// table.  buf: {key words, u64 count}[cap] + the tail words (links_kernels.h, triples_kernels.h), allocated and zeroed on the first enable; tab: the
// table once it is zeroed
struct CountTable {
    bool on = false;
    DevBuf buf;
    unsigned long long* tab = nullptr;
    uint64_t cap = 0, bound = 0;
};
// the pileup (bgr_aligner_pileup_enable, bgr_aligner_pileup_strands_enable): every greedy / anchors launch is followed by the pileup kernel, which with
// strands also adds the forward observations to a second table
struct PileupTables {
    bool on = false, strands_on = false;
    DevBuf table, offs;                    // the table (pileup_kernels.h) and base_offs, allocated, zeroed / uploaded on the first enable
    DevBuf fwd;                            // the forward table: the layout of `table`, its tail stays 0
    uint32_t* tab = nullptr;               // the tables once they are ready (a run's variants take them away: capi_variants.hip)
    const uint64_t* base_offs = nullptr;
    uint32_t* fwd_tab = nullptr;
    void release() { table.release(); offs.release(); fwd.release(); }
};

// What an aligner and its twins (below) have in common: the tuning, the knobs, the switches of the counting features and the tables that every stream
// adds to (the atomics are device-scope).  The aligner allocates it and a twin points at its owner's, so a setting made on the aligner is the twin's
// at once; nothing writes it through a twin, and the threads of an overlapped batch only read it.
struct AlignerShared {
    uint32_t cfg_waves = 0, cfg_blocks_per_cu = 0, cfg_lds_mphf = 0;
    bool exh_filter = bgr::opt("exh_filter") != 0;  // exhaustive mode through the minimizer filter too (option exh_filter = 0: without)
    // bgr_aligner_set_knob (test / diagnostic hooks, read here instead of from the environment on every launch; the table of them is in capi.hip)
    uint64_t knob_frame_cap = 0, knob_search = 0, knob_split_limit = 0, knob_debug_stop = 0, knob_greedy_fast = 0, knob_exh_fast = 0, knob_anc_fast = 0, knob_memo_cap = 0, knob_prepass = 0;
    uint64_t knob_no_events = 0, knob_no_jump = 0;   // BGR_KNOB_KERNEL_EVENTS (kept inverted), BGR_KNOB_GREEDY_JUMP
    uint64_t knob_overlap = 0, knob_device_overlap = 0, knob_abundance_form = 0, knob_links_form = 0;   // BGR_KNOB_BATCH_OVERLAP, .._DEVICE_OVERLAP, .._ABUNDANCE_FORM, .._LINKS_FORM
    bool abundance_on = false;          // bgr_aligner_abundance_enable: every greedy / anchors launch is followed by the abundance kernel (the table is each stream's own)
    CountTable links, triples;
    PileupTables pileup;
    // the inside pass (bgr_aligner_inside_enable): every greedy / anchors launch is followed, in front of the counting kernels, by bgr_align_inside_kernel
    // over the graph's inside index on this device (inside_tab: null = off); what it mapped is counted at kSmallInside of each stream's `small`
    const BgrInsideEntry* inside_tab = nullptr;
    uint64_t inside_slots = 0;
    // bgr_aligner_exhaustive_paths_enable: the paths of exhaustive launches are output -- the counting kernels run behind such a launch once it is settled,
    // and whatever reads the rows of the last launch reads an exhaustive one through its view (launch.rows_view)
    bool exhaustive_paths = false;
    void release() { links.buf.release(); triples.buf.release(); pileup.release(); }
};

struct bgr_aligner {
    bgr_graph* graph = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    BgrDeviceGraph dg;
    AlignerShared* sh = nullptr;  // the aligner's own, or (a twin) that of the aligner it belongs to
    TextRoute text;
    LaunchBufs launch;
    FetchBufs fetch;
    HaplotagBufs tag;
    VariantBufs var;
    DevBuf abundance;             // u64[n_unitigs + 1][3], allocated and zeroed on the first enable: one per stream, summed when it is read
    bool gaf_cs = false;          // bgr_aligner_gaf_cs_enable: the GAF lines of bgr_align_fasta_text end in the cs:Z: field
    bool blocking_sync = bgr::opt("blocking_sync") != 0;
    hipEvent_t ev_wait = nullptr;
    struct DeepRun {  // the last pass of the exhaustive launch in flight, as enqueued: settle_launch runs it again for reads whose table filled up
        bool open = false;
        bgr::Pass pass;
        bgr::BatchIO io;
        bgr::KernelParams kp;
        BgrDeviceGraph dg;
        uint32_t per_wave_lds = 0, path_cap = 0, memo_cap = 0, runs = 0;
    } deep;
    struct DeepCount {  // the counting kernels of the exhaustive launch in flight (exhaustive_paths): what they are handed, kept until settle_launch has made the rows final and queues them
        bool open = false;
        uint64_t arena_cap = 0, n_reads = 0, total_bases = 0;
        const uint64_t* read_offs = nullptr;
        bgr::PileupReads reads;
        int ev_launch = -1;       // the launch's place in the timer ring (-1: not timed)
        int marks = 0;            // ... and the kernels timed in it so far
    } deep_count;
    bool view_ready = false;      // launch.rows_view holds the view of the last launch (an exhaustive one, settled)
    bgr::PlanDevice plan_dev;     // CUs, LDS, resident waves per kernel: asked once
    bool plan_dev_known = false;
    uint64_t last_n = 0;
    uint32_t last_mode = 0;       // mode of the last mapping launch (bgr_aligner_path_stats)
    uint64_t last_arena_cap = 0, last_total_bases = 0;   // its arena's ints and its reads' bases (the counting kernels behind bgr_aligner_path_stats: test.count_with_path_stats)
    uint64_t sized_n = 0;         // reads of the last launch that sized the buffers (forget_launch leaves it: option test.keep_rows asks for the same launch again)
    uint64_t wave_times_n = 0;    // diagnostic builds only (-DBGR_PHASE_TIMING)
    uint64_t ticket_serial = 0;       // bgr_align_batch_begin: tickets handed out; the batch of the last one is in flight until its wait
    bool ticket_open = false;
    std::vector<uint64_t> ticket_offs;  // that batch's offsets made relative (kept alive for the asynchronous copy)
    uint32_t last_launch[4] = {0, 0, 0, 0};
    double var_ms[5] = {0, 0, 0, 0, 0};       // bgr_aligner_pileup_sites: the last call's five launches
    double bub_ms[4] = {0, 0, 0, 0};          // bgr_aligner_bubbles: the last call's four launches
    bgr_aligner* twin = nullptr;    // second stream + buffers: the overlapped form of bgr_align_batch, un-waited consecutive bgr_align_device launches (created on first use)
    bool is_twin = false;
    bgr_aligner* holder = nullptr;  // who took this aligner's last mapping launch: null = itself, else its twin (launch_taker.h); "the last launch" is read there
    int num_cus = 0;
    size_t lds_per_cu = 0;
    hipEvent_t ev[kTimerRing][kTimerSlots + 1];  // ev[i][0] = start of launch i, ev[i][j] = behind its j-th kernel
    int ev_marks[kTimerRing];                    // kernels timed in launch i
    int ev_used = 0;
    uint64_t t_launches = 0;
    double t_ms = 0, t_slot_ms[kTimerSlots] = {0, 0, 0, 0, 0, 0, 0, 0};
    const char* t_slot_name[kTimerSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~bgr_aligner() { if (!is_twin) delete sh; }   // (its device memory: bgr_aligner_destroy)
};

// Wait for the aligner's stream.  By default hipStreamSynchronize (the runtime spins: lowest latency, one busy CPU per waiting thread);
// with BGREAT_BLOCKING_SYNC=1 an event made with hipEventBlockingSync is recorded and waited for instead: the thread sleeps until the
// interrupt, so more stream workers per device than CPUs to spare can overlap their calls (bgr_align_all's text route).
inline hipError_t wait_stream(bgr_aligner* a) {
    if (!a->blocking_sync) return hipStreamSynchronize(a->stream);
    hipError_t e = hipEventRecord(a->ev_wait, a->stream);
    return e == hipSuccess ? hipEventSynchronize(a->ev_wait) : e;
}
// capi.hip: an exhaustive launch still in flight on this one aligner (or twin) is settled -- reads its last pass handed back are mapped -- and, where its
// counting kernels waited for that (bgr_aligner_exhaustive_paths_enable), those are queued on its stream; nothing to do otherwise
extern "C" int settle_pending(bgr_aligner* a);
// Wait for every stream that adds to the aligner's tables: its own and its twins' (an exhaustive launch whose counting is still to come counts first).
inline int sync_all(bgr_aligner* a) {
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) {
        if (const int rc = settle_pending(x); rc != BGR_OK) return rc;
        HIP_TRY(hipStreamSynchronize(x->stream));
    }
    return BGR_OK;
}

// The aligner whose buffers hold the last mapping launch: the aligner itself, or its twin when that took it (bgr_align_device, launch_taker.h).
inline bgr_aligner* holder_of(bgr_aligner* a) { return a->holder ? a->holder : a; }
inline const bgr_aligner* holder_of(const bgr_aligner* a) { return a->holder ? a->holder : a; }

// ---- what the counting features' units share -----------------------------------------------------------------------------------------
// *n = have; BGR_E_CAPACITY when `cap` has no room for them (the first call of a caller that asks for the number)
inline int rows_refusal(uint64_t have, uint64_t cap, uint64_t* n, const char* who, const char* noun) {
    *n = have;
    if (have > cap) return fail(BGR_E_CAPACITY, std::string(who) + ": " + std::to_string(have) + " " + noun + ", room for " + std::to_string(cap));
    return BGR_OK;
}
// `rows` into `out` when cap has room, each through `conv` (a row of a count table is no record of the interface)
template <class Row, class Out, class Conv>
int deliver_rows(const std::vector<Row>& rows, Out* out, uint64_t cap, uint64_t* n, const char* who, const char* noun, Conv conv) {
    if (const int rc = rows_refusal(rows.size(), cap, n, who, noun); rc != BGR_OK) return rc;
    for (size_t i = 0; i < rows.size(); ++i) out[i] = conv(rows[i]);
    return BGR_OK;
}
template <class Row>
int deliver_rows(const std::vector<Row>& rows, Row* out, uint64_t cap, uint64_t* n, const char* who, const char* noun) {
    return deliver_rows(rows, out, cap, n, who, noun, [](const Row& r) { return r; });
}
// a bgr_graph_* getter: the rows the last successful run left in g->*f (`none`: what the message calls them when there are none)
template <class F, class Out, class... Conv>
int graph_rows(const bgr_graph* g, F bgr_graph::*f, Out* out, uint64_t cap, uint64_t* n, const char* who, const char* noun, const char* none, Conv... conv) {
    if (n) *n = 0;
    if (!g || !n || (cap && !out)) return fail(BGR_E_ARG, std::string(who) + ": null argument");
    if (!(g->*f).valid) return fail(BGR_E_ARG, std::string(who) + ": no " + none + " -- they are those of the last successful bgr_align_all with " + who + "_enable on");
    return deliver_rows((g->*f).rows, out, cap, n, who, noun, conv...);
}

// what bgr_graph_{bubbles,phase,blocks,haplotypes}_enable refuse: a null graph, and with `on` a threshold of 0, a graph without its host blob, one
// whose unitigs are not ACGT only (`blob`, `acgt`: the feature's own words for the last two)
inline int chain_refusal(const bgr_graph* g, const char* who, uint32_t on, const ChainMins& given, const char* blob, const char* acgt) {
    const std::string w = who;
    if (!g) return fail(BGR_E_ARG, w + ": null graph");
    if (!on) return BGR_OK;
    if (given.link == 0) return fail(BGR_E_ARG, w + ": min_link is at least 1");
    if (given.phase == 0) return fail(BGR_E_ARG, w + ": min_phase is at least 1");
    if (given.block == 0) return fail(BGR_E_ARG, w + ": min_block is at least 1");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, w + ": the graph has no host blob (" + blob + ")");
    if (g->header.has_exc) return fail(BGR_E_ARG, w + ": " + acgt);
    return BGR_OK;
}
// The thresholds a run uses (under abundance_m).  link, what its bubbles are called with: that of the first switch that is on in the order bubbles,
// phase, blocks, haplotypes -- the others are on top of it -- and the bubbles' stored one when none is.  phase, what its blocks are chained with: the
// blocks' when their switch is on or the haplotypes' is off, else the haplotypes'.  block, the smallest block that is spelled: the haplotypes'.
inline ChainMins run_thresholds(const bgr_graph* g) {
    ChainMins m = {g->bubbles.min.link, g->blocks.on || !g->haplotypes.on ? g->blocks.min.phase : g->haplotypes.min.phase, g->haplotypes.min.block};
    const ChainSwitch* const chain[4] = {&g->haplotypes, &g->blocks, &g->phase, &g->bubbles};
    for (const ChainSwitch* s : chain) if (s->on) m.link = s->min.link;
    return m;
}

// a file of lines: the header, then line(i, &buf) for i < n, in pieces of a megabyte
template <class Line>
int write_lines(const char* who, const char* path, const char* header, uint64_t n, Line line) {
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string(who) + ": cannot open " + path);
    std::string buf = header;
    bool ok = true;
    for (uint64_t i = 0; i < n && ok; ++i) {
        line(i, &buf);
        if (buf.size() > (1u << 20)) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); }
    }
    if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string(who) + ": write to " + path + " failed");
    return BGR_OK;
}

// What one call needs on a device and nowhere after it: a stream (its own, made on the current device, or a borrowed one), events, buffers.  The
// destructor waits for the stream first -- an early return may leave a copy into the caller's locals in flight -- then frees: nothing stays allocated.
struct DeviceCall {
    hipStream_t s = nullptr;
    bool owned = false;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBuf buf[5];
    int rc = BGR_OK;   // what the last room() that returned false has set
    explicit DeviceCall(hipStream_t borrowed = nullptr) : s(borrowed) {}
    DeviceCall(const DeviceCall&) = delete;
    int own_stream() { HIP_TRY(hipStreamCreate(&s)); owned = true; return BGR_OK; }
    int events(int n) { for (int i = 0; i < n; ++i) HIP_TRY(hipEventCreate(&ev[i])); return BGR_OK; }
    bool room(DevBuf& b, uint64_t bytes, const std::string& what) {   // -> whether the device has `bytes` for b; else rc = BGR_E_NOMEM / BGR_E_HIP, "`what`: the runtime's words"
        const hipError_t e = b.ensure(bytes);
        if (e == hipSuccess) return true;
        (void)hipGetLastError();
        rc = fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, what + ": " + hipGetErrorString(e));
        return false;
    }
    ~DeviceCall() {
        if (s) (void)hipStreamSynchronize(s);
        for (DevBuf& b : buf) b.release();
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (owned) (void)hipStreamDestroy(s);
    }
};

// ---- the functions that cross units --------------------------------------------------------------------------------------------
// capi.hip, for the text route (capi_text.hip)
void forget_launch(bgr_aligner* a);   // no single launch whose results could be read again: bgr_aligner_fetch finds n = 0, on the aligner itself
extern "C" {   // (defined among the functions of the interface)
int align_device_impl(bgr_aligner* a, const bgr_params* p, const void* d_reads, const void* d_read_offsets, uint64_t n_reads, uint64_t total_bases, uint32_t max_read_len,
                      bool planes_ready, const void* d_src_off, uint64_t reads_bytes, bool cursor_is_zero);   // the mapping launch of one batch (see there)
int settle_launch(bgr_aligner* a, uint32_t* cur);   // behind a mapping launch, its stream waited for and the cursor block in `cur`: the arena flag; exhaustive mode: reads handed back are mapped, then the counting kernels that waited for that are queued
// the rows of the last launch of `h` (the aligner that holds it) as a reader of greedy rows takes them: its results, or -- an exhaustive launch, which is
// settled first -- its view, made on h's stream if it is not there.  `who` refuses an exhaustive launch of an aligner without bgr_aligner_exhaustive_paths_enable
int last_rows(bgr_aligner* h, const std::string& who, const uint2** rows);
int view_launch(bgr_aligner* a, uint64_t n_reads, uint64_t arena_cap);   // the view of the rows in a->launch.results into a->launch.rows_view, queued on a->stream (the text route's GAF kernels read an exhaustive launch through it)
}
// capi_abundance.hip
int abundance_table(bgr_aligner* a);   // this one aligner's (or twin's) table, allocated and zeroed the first time it is asked for
bgr::AbundancePlan abundance_plan_of(const bgr_aligner* a, uint64_t n_reads, uint64_t total_bases);   // geometry and form of the abundance kernel behind a launch of this size
// capi_links.hip: the count tables, links and triples
int links_tail(bgr_aligner* a, const char* who, uint64_t* tail);   // the three words behind the aligner's table of links, every stream that adds to it waited for; BGR_E_ARG when links were never enabled, BGR_E_CAPACITY when the table has overflowed
void triples_records(const std::vector<std::array<uint64_t, 3>>& rows, bgr_triple* out);   // the rows of a table of triples as the interface's records
// A whole run (run_counts.h, through the table of stages in capi_abundance.hip).  begin: the totals of the run before are gone; collect: an aligner's
// table joins the run's; end: totals only of a run that ended well -- the tables sorted and merged, every stage of the chain called from the totals of
// the one it reads (all on bubbles.device), BGR_OK when ok is false
void run_links_begin(bgr_graph* g);
int run_links_collect(bgr_graph* g, bgr_aligner* a);
int run_links_end(bgr_graph* g, bool ok);
void run_triples_begin(bgr_graph* g);
int run_triples_collect(bgr_graph* g, bgr_aligner* a);
int run_triples_end(bgr_graph* g, bool ok);
void run_bubbles_begin(bgr_graph* g);                    // capi_bubbles.hip
int run_bubbles_collect(bgr_graph* g, bgr_aligner* a);   // ... the first aligner's device is where the run's links will be called
int run_bubbles_end(bgr_graph* g, bool ok);              // ... behind the links' end
void run_phase_begin(bgr_graph* g);                      // capi_triples.hip
int run_phase_end(bgr_graph* g, bool ok);                // ... behind the bubbles' and the triples' end: the two joined on the host
void run_blocks_begin(bgr_graph* g);                     // capi_blocks.hip
int run_blocks_end(bgr_graph* g, bool ok);               // ... behind the phase's end
void run_haplotypes_begin(bgr_graph* g);                 // capi_haplotypes.hip
int run_haplotypes_end(bgr_graph* g, bool ok);           // ... behind the blocks' end: spelled from the resident graph
void run_recompact_begin(bgr_graph* g);                  // capi_recompact.hip
int run_recompact_collect(bgr_graph* g, bgr_aligner* a); // ... the first aligner's device is where the run's kept unitigs will be compacted
int run_recompact_end(bgr_graph* g, bool ok);            // ... behind the abundance's end: keep = reads >= min_reads
// The end of a chain stage under abundance_m: what it kept is forgotten; with ok, `call` makes the new rows (BGR_OK, or what it refuses with) provided
// the stages it reads (`inputs_valid`, else BGR_E_INTERNAL with `missing`) have theirs and, where there is something to call from, an aligner was collected
template <class F, class Call>
int chain_stage_end(bgr_graph* g, F& f, bool ok, bool inputs_valid, const char* missing, bool anything, const char* uncollected, Call call) {
    f.forget();
    if (!ok) return BGR_OK;
    int rc = BGR_OK;
    if (!inputs_valid) rc = fail(BGR_E_INTERNAL, std::string("bgr_align_all: ") + missing);
    else if (anything) rc = g->bubbles.device < 0 ? fail(BGR_E_INTERNAL, std::string("bgr_align_all: ") + uncollected + ", but no aligner of the run was collected") : call();
    if (rc != BGR_OK) f.forget();
    f.valid = rc == BGR_OK;
    return rc;
}
// capi_haplotag.hip: the graph's tag table while its switch is on, else null (run_counts.h; where a run needs no more than a call of the interface, that is registered)
const uint32_t* run_haplotag_table(const bgr_graph* g, uint64_t* n_rows);
// capi_pileup.hip
int pileup_guard(const bgr_unitig_abundance* rows, uint64_t n, const char* who);   // BGR_E_CAPACITY when a reads column reached 2^32: a depth may have wrapped
int guarded_sync(bgr_aligner* a, const char* who);   // the aligner's abundance snapshot through pileup_guard, then sync_all
int graph_base_offs(bgr_graph* g, const char* who);  // g->base_offs (prefix sums of the unitig lengths) made, once per graph
int pileup_refusal(const bgr_graph* g, const char* who);   // BGR_E_ARG on a graph whose unitigs are not ACGT only
void run_pileup_begin(bgr_graph* g);                   // a whole run (run_counts.h), as the links';
int run_pileup_collect(bgr_graph* g, bgr_aligner* a);  // ... the pileup switch gathers on the host, the variants switch on a device
int run_pileup_end(bgr_graph* g, bool ok);             // ... behind the abundance's end: BGR_E_CAPACITY when a depth may have wrapped
// capi_inside.hip
void inside_free_devices(bgr_graph* g);                // the device copies of the graph's inside index released (bgr_graph_destroy)
void run_inside_begin(bgr_graph* g);                   // a new run (run_counts.h): its count starts at 0
int run_inside_collect(bgr_graph* g, bgr_aligner* a);  // ... the aligner's count (its streams waited for) joins the run's
// capi_variants.hip
int variants_collect(bgr_graph* g, bgr_aligner* a);   // a run's aligner: the first one's tables become the run's (g->variants_run), the others' are added
int variants_end(bgr_graph* g, bool ok);              // the run's end: the sites called once from the run's table, which is freed whatever happens
void variants_run_free(bgr_graph* g);                 // g->variants_run and its device memory released

#pragma GCC visibility pop

#endif
