// pipeline_stages.h -- part of the translation unit pipeline.cpp (included by it alone): the state of one pipeline and its stages.
//   RunShape       everything decided before a thread starts (plan_run), NodeAffinity, the output files and aligners
//   Run            what the threads share: pool, channels, failure state, timers
//   Producer       stage 1: the input files into batches, one feeder per kind of input (FASTQ / FASTA on the text / host route)
//   gather, stage_text, host_parse_piece, gather_batches      stage 1b: a batch into page-locked memory
//   map_text_piece, map_packed, map_batches                   stage 2: the stream workers
//   ProgressCounts, OrderedWriter, write_files                stage 3 + 4: format in input order, write
#pragma once
#include <sched.h>
#include <sys/stat.h>

#include <chrono>
#include <cstdio>
#include <iostream>
#include <map>
#include <string>

#include "fastx.h"
#include "file_image.h"
#include "options.h"
#include "pipeline_support.h"
#include "record_format.h"
#include "run_counts.h"

namespace bgr {
int set_error(int code, const std::string& msg);  // capi.hip
}

namespace {

using bgr::ParsedChunk;
using MappedFile = bgr::FileImage;  // mmap for regular files, read-until-EOF for FIFOs and other streams

// Something the reference prints to stdout between two reads of the input order: a file name (aligner.cpp:559,576) or, in
// exhaustive mode, the block its worker prints after every tenth getReads() call (alignerExhaustive.cpp:306-316).  A
// mark sits in front of read `pos` of its batch; the ordered writer prints it when it gets there.
struct Mark {
    uint64_t pos;
    int kind;          // 0 = progress block, 1 = line of text
    std::string text;
};

struct Batch {
    uint64_t index = 0;
    std::vector<Mark> marks;                              // ascending pos
    std::shared_ptr<MappedFile> file;                     // keeps header/sequence slices valid
    std::vector<std::unique_ptr<ParsedChunk>> chunks;
    std::shared_ptr<std::vector<std::unique_ptr<ParsedChunk>>> shared_chunks;  // a chunk group cut into several batches (base cap): its storage, shared
    uint64_t n = 0, bases = 0, path_cap = 0;
    std::unique_ptr<Pinned> pin;                          // attached by the gatherer, handed back by the formatter
    std::vector<RecSlice> recs;                           // flattened view of the records of this batch
    // text route: the batch is bytes [t_begin, t_end) of `file` (a piece that starts at a header line); once mapped as text,
    // dev_text is set and the record streams sit in pin->ptext / pin->ntext
    bool text_piece = false, dev_text = false, fastq_piece = false;
    uint64_t t_begin = 0, t_end = 0, p_bytes = 0, n_bytes = 0;
    // a FASTQ piece crosses PCIe without its '+' and quality lines: fq_parts = where the gatherer may cut it into independent parts
    // ({first byte, number of the line it lies in}, FastqPlan::piece_parts), t_gathered = bytes of header + read lines staged
    std::vector<std::pair<uint64_t, uint64_t>> fq_parts;
    std::vector<std::shared_ptr<const std::vector<uint32_t>>> fq_nl;  // per part: the newline offsets of the plan's chunk the part lies in (from that chunk's first byte), or null
    uint64_t fq_chunk_bytes = 0;
    uint64_t t_gathered = 0;
    // text route under -b with progress blocks: the batch is a piece [t_begin, t_end) of its file whatever route mapped it in the end; the
    // writer counts getReads() iterations (record attempts) itself.  n_attempts = iterations of the piece; the device's per-record words sit in
    // pin->info, a piece that fell back to the host parser lists the iteration of each of its reads in att_of_read
    bool text_origin = false, first_of_file = false, last_of_file = false;
    uint64_t n_attempts = 0;
    std::vector<uint64_t> att_of_read;
    unsigned dev = 0;                                     // which device of the run maps the batch (round robin in input order)
};
using BatchPtr = std::unique_ptr<Batch>;
using BatchChannel = Channel<BatchPtr>;

const uint64_t kRefBatch = 10000;  // records per getReads() call (alignerExhaustive.cpp:270)

// Where the reference's exhaustive worker prints its periodic block at -t 1: `iter` starts at 1 (aligner.h:103) and
// `iter++ % 10 == 0` is tested after every getReads() call, over all input files, so the block follows calls 10, 20, ...
// A call is 10000 loop iterations of getReads (record attempts, accepted or not); the parser counts them per chunk.
struct ProgressMarker {
    bool on = false;
    uint64_t calls_before = 0;  // calls made for earlier files
    uint64_t next_fc = 10;      // the next call of the current file (1-based) that is followed by a block
    void begin_file() { next_fc = 10 - calls_before % 10; }
    // Chunk `ch` holds iterations [base_iter, base_iter + ch.iters) of the file: indices (chunk-relative, ascending) of the
    // records in front of which a block is due; ch.recs.size() = behind its last record.
    void chunk(const ParsedChunk& ch, uint64_t base_iter, std::vector<uint64_t>& idx_out) {
        idx_out.clear();
        while (on && next_fc * kRefBatch < base_iter + ch.iters) {
            const uint64_t rel = next_fc * kRefBatch - base_iter;  // first iteration of the call after the block
            idx_out.push_back((uint64_t)(std::lower_bound(ch.rec_iter.begin(), ch.rec_iter.end(), rel) - ch.rec_iter.begin()));
            next_fc += 10;
        }
    }
    // End of a file of `total_iters` iterations (>= 1: even an empty file costs one call): blocks still due.
    unsigned end_file(uint64_t total_iters) {
        const uint64_t calls = (total_iters + kRefBatch - 1) / kRefBatch;
        unsigned due = 0;
        while (on && next_fc <= calls) { ++due; next_fc += 10; }
        calls_before += calls;
        return due;
    }
};

// Bytes [begin, end) of one input file (end beyond the file: to its end).  `mf`: the file's image when the caller has opened it already
// (the lanes of a split run share the images; a FIFO can be opened only once), else the producer opens it when it gets there.
struct InputSpan {
    std::string file;
    std::shared_ptr<MappedFile> mf;
    uint64_t begin = 0, end = ~0ull;
};

inline uint64_t now_us() { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- what a run is, decided before any thread starts --------------------------------------------------------------------------
inline bool run_progress_blocks(const bgr_params* prm, const bgr_run_options* opt) { return opt->echo_files && prm->mode == BGR_MODE_EXHAUSTIVE; }
inline bool run_correction(const bgr_params* prm, const bgr_run_options* opt) { return opt->correction && prm->mode != BGR_MODE_EXHAUSTIVE; }  // alignPartExhaustive ignores -c
// (option test.lanes_on_one_device, a test hook: every device of the run is the first one -- the N-device code path on a one-GPU box)
inline bool run_on_one_device() { return bgr::opt("test.lanes_on_one_device") != 0; }

// The threads of a run (and the page-locked memory they allocate) on the NUMA node of the devices they feed: a copy engine
// reading staging buffers across the socket link runs at about half its rate.  Only when all devices of the run share a node;
// the calling thread's affinity is restored at the end, and `threads`, the pool of host threads, is clamped to the CPUs of the restricted
// set (opt->numa = 1, or the option numa = 0, leaves the affinity alone).
struct NodeAffinity {
    unsigned threads;
    explicit NodeAffinity(const bgr_run_options* opt) : threads(std::max<uint32_t>(1, opt->threads)) {
        if (opt->numa || bgr::opt("numa") == 0) return;
        const bool one_device = run_on_one_device();
        std::string first_list;
        for (unsigned g = 0; g < std::max<uint32_t>(1, opt->n_gpus); ++g) {
            char list[512];
            if (bgr_device_local_cpus((int)(one_device ? opt->first_device : opt->first_device + g), list, sizeof(list)) != BGR_OK) return;
            if (g == 0) first_list = list; else if (first_list != list) return;
        }
        if (first_list.empty() || sched_getaffinity(0, sizeof(old_), &old_) != 0) return;
        cpu_set_t want;
        CPU_ZERO(&want);
        int n_set = 0;
        const char* c = first_list.c_str();
        while (*c) {  // "a-b,c,d-e"
            char* e = nullptr;
            long a = strtol(c, &e, 10), b = a;
            if (e == c) break;
            if (*e == '-') { c = e + 1; b = strtol(c, &e, 10); }
            for (long i = a; i <= b && i < CPU_SETSIZE; ++i) if (CPU_ISSET(i, &old_)) { CPU_SET(i, &want); ++n_set; }
            c = *e == ',' ? e + 1 : e;
            if (*e != ',' && *e != 0) break;
        }
        if (n_set > 0 && sched_setaffinity(0, sizeof(want), &want) == 0) {
            changed_ = true;
            threads = std::min<unsigned>(threads, (unsigned)n_set);  // (a pool larger than the CPU set it may run on only oversubscribes it)
        }
    }
    ~NodeAffinity() { if (changed_) sched_setaffinity(0, sizeof(cpu_set_t), &old_); }
    NodeAffinity(const NodeAffinity&) = delete;
    NodeAffinity& operator=(const NodeAffinity&) = delete;
private:
    cpu_set_t old_;
    bool changed_ = false;
};

struct RunShape {
    unsigned n_gpus = 1, first_device = 0, threads = 1;
    bool one_device = false, fastq = false, echo_files = false;
    bool writes = false, correction = false, gaf = false, split_no_overlap = false, extended = false;  // extended: format_range_ext writes the records
    bool progress_blocks = false, text_route = false, text_progress = false, fastq_gather = false, timing = false;
    // text route: bytes of a batch.  At most kTextPieceMax: the device addresses the two formatted streams with 32 bits, and a piece of B
    // bytes gives at most 12 B + (its own bytes) of records (--batch beyond ~1.9 M reads of 150 bp is cut to that)
    static constexpr uint64_t kTextPieceMax = 320ull << 20;
    uint64_t batch_reads = 0, piece_bytes = 0, batch_bases_cap = 1ull << 30, chunk_bytes = 0, out_div = 4;
    unsigned per_dev = 2;
    size_t n_aligners = 0, extra_sets = 0, max_batches = 0, n_pins = 0;
    uint32_t k = 0;
    Unitigs unitigs;                     // -c and --gaf: the host formatter spells walks
    const uint32_t* tag_table = nullptr; // haplotags (bgr_graph_haplotag_enable; bgr_align_all has refused a run without gaf): the graph's table goes onto every
    uint64_t tag_rows = 0;               // aligner's device, and the host formatter tags from the same words
    bool gaf_cs = false;                 // the cs:Z: field (bgr_graph_gaf_cs_enable; the same refusal): every aligner's switch is set, the host formatter writes it too
    bool inside = false;                 // the inside pass (bgr_graph_inside_enable; bgr_align_all has refused it in exhaustive mode): every aligner's switch is set
    bool exhaustive_paths = false;       // an exhaustive run with bgr_graph_exhaustive_paths_enable: every aligner's switch is set, the host formatter reads the rows without their end offset
    int device_of(unsigned g) const { return (int)(one_device ? first_device : first_device + g); }
};

int plan_run(bgr_graph* graph, const bgr_params* prm, const bgr_run_options* opt, unsigned threads, RunShape& s) {
    bgr_graph_info_t gi;
    if (bgr_graph_info(graph, &gi) != BGR_OK) return BGR_E_ARG;
    s.k = gi.k;
    s.n_gpus = std::max<uint32_t>(1, opt->n_gpus);
    s.first_device = opt->first_device;
    s.one_device = run_on_one_device();
    s.threads = threads;
    s.fastq = opt->fastq != 0;
    s.echo_files = opt->echo_files != 0;
    s.exhaustive_paths = prm->mode == BGR_MODE_EXHAUSTIVE && bgr::g_run_counts.exhaustive_paths_wanted && bgr::g_run_counts.exhaustive_paths_wanted(graph) != 0;
    s.writes = prm->mode != BGR_MODE_EXHAUSTIVE || opt->write_exhaustive || (s.exhaustive_paths && opt->gaf);   // (GAF lines of an exhaustive run: the two files as --write-exhaustive fills them)
    s.correction = run_correction(prm, opt);
    s.gaf = opt->gaf != 0;  // (bgr_align_all has refused it in exhaustive mode without bgr_graph_exhaustive_paths_enable, with -c and on a graph with exception planes)
    s.split_no_overlap = opt->no_overlap_file != nullptr;
    s.extended = s.correction || s.gaf || s.split_no_overlap;
    s.progress_blocks = run_progress_blocks(prm, opt);
    // Text route: the device parses, packs, maps and formats (bgr_align_fasta_text); the host only moves bytes.  FASTA or FASTQ, the
    // reference's two output files.  Correction mode too (the device spells the reads from its 2-bit unitig store) unless the graph has
    // non-ACGT unitig characters.  -b WITH its progress blocks too, for FASTA -- the device says what became of every record
    // (bgr_text_batch.record_info_out) and the ordered writer counts getReads() calls from that; FASTQ with progress blocks stays on the host route.
    s.text_route = opt->route == 0 && !(s.correction && gi.has_exceptions) && !s.split_no_overlap && !(s.progress_blocks && s.fastq);
    s.text_progress = s.text_route && s.progress_blocks;
    // Defaults: 128k reads per batch keeps the page-locked staging small (it costs ~0.2 s per GB to allocate) and the
    // pipeline fine-grained; the parser chunk is a thread's share of a batch.
    // (one launch addresses its path arena with 32 bits: a batch stays below 4 M reads and ~1 G bases)
    s.batch_reads = std::min<uint64_t>(opt->batch_reads ? opt->batch_reads : (s.text_route ? 1ull << 18 : 1ull << 17), 4ull << 20);
    s.piece_bytes = std::min<uint64_t>(std::max<uint64_t>(s.batch_reads * 170, 4096), RunShape::kTextPieceMax - (16ull << 20));
    if (const int64_t cap = bgr::opt("test.bases_cap")) s.batch_bases_cap = (uint64_t)cap;  // (test hook: walk the cut with small inputs)
    s.chunk_bytes = opt->chunk_bytes ? opt->chunk_bytes : std::min<uint64_t>(8ull << 20, std::max<uint64_t>(256ull << 10, s.batch_reads * 170 / threads));
    if (s.correction || s.gaf) {
        if (bgr_graph_unitigs(graph, &s.unitigs.seqs, &s.unitigs.offs, &s.unitigs.n) != BGR_OK) return BGR_E_ARG;
        s.unitigs.k = gi.k;
    }
    if (s.gaf && bgr::g_run_counts.haplotag_table) s.tag_table = bgr::g_run_counts.haplotag_table(graph, &s.tag_rows);
    if (s.gaf && bgr::g_run_counts.gaf_cs_wanted) s.gaf_cs = bgr::g_run_counts.gaf_cs_wanted(graph) != 0;
    if (bgr::g_run_counts.inside_wanted) s.inside = bgr::g_run_counts.inside_wanted(graph) != 0;
    // two aligners (streams) per device so that consecutive batches overlap copy and compute (text route: the piece is already on its
    // way to the device when a worker takes the batch; measured 185 / 163 / 149 Mreads/s end to end with 2 / 3 / 4 workers per device)
    if (const int64_t w = bgr::opt("workers_per_device")) s.per_dev = (unsigned)w;  // (tuning / experiments)
    s.n_aligners = (size_t)s.n_gpus * s.per_dev;
    // A fixed pool of batch objects circulates producer -> GPU workers -> writer -> producer, so the pinned
    // buffers are allocated once and the number of batches in flight is bounded.
    s.extra_sets = s.text_route ? 3 : 0;  // text route: a set is held from the read of its piece until its streams are written
    if (bgr::opt("extra_sets") >= 0) s.extra_sets = (size_t)bgr::opt("extra_sets");
    s.max_batches = s.n_aligners * 2 + 2 + s.extra_sets;
    s.n_pins = s.n_aligners * 2 + 1 + s.extra_sets;
    // text route: room for a piece's two record streams.  A mapped 150 bp read leaves ~27 bytes of its 165 in `paths`, an unmapped one all
    // of them in the other file: a quarter of the piece each to start with (page-locked memory costs ~0.2 s per GB: less of it, and a fresh
    // process reaches its rate sooner); a stream that does not fit comes back as BGR_E_CAPACITY and the set's buffer grows once (-c, whose
    // paths stream is header + read, starts at the full size)
    s.out_div = s.correction ? 1 : s.gaf ? 2 : 4;   // (a GAF line is about half a 150 bp record)
    // FASTQ on the text route: only the header and read lines of a piece go to the device (option fastq_gather = 0: the four-line records as they are)
    s.fastq_gather = bgr::opt("fastq_gather") != 0;
    s.timing = bgr::opt("timing") != 0;
    return BGR_OK;
}

struct FileClose { void operator()(FILE* f) const { fclose(f); } };
using OutFile = std::unique_ptr<FILE, FileClose>;
struct Outputs { OutFile paths, notaligned, no_overlap; };
int open_outputs(const bgr_run_options* opt, const char* paths_file, const char* notaligned_file, Outputs& out) {
    if (opt->no_overlap_file) {
        out.no_overlap.reset(fopen(opt->no_overlap_file, "wb"));
        if (!out.no_overlap) return bgr::set_error(BGR_E_IO, "bgr_align_all: cannot open the no-overlap file");
    }
    out.paths.reset(fopen(paths_file, "wb"));            // aligner.h:85
    out.notaligned.reset(fopen(notaligned_file, "wb"));  // aligner.h:86
    if (!out.paths || !out.notaligned) return bgr::set_error(BGR_E_IO, "bgr_align_all: cannot open the output files");
    return BGR_OK;
}

struct AlignerDestroy { void operator()(bgr_aligner* a) const { bgr_aligner_destroy(a); } };
using AlignerPtr = std::unique_ptr<bgr_aligner, AlignerDestroy>;
// per_dev aligners for every device of the run, device by device; `counts`: what the run counts (run_counts.h)
int make_aligners(bgr_graph* graph, const RunShape& s, uint32_t counts, std::vector<AlignerPtr>& out) {
    for (unsigned g = 0; g < s.n_gpus; ++g) {
        for (unsigned j = 0; j < s.per_dev; ++j) {
            bgr_aligner* a = nullptr;
            int rc = bgr_aligner_create(graph, s.device_of(g), &a);
            if (rc != BGR_OK) return rc;
            out.emplace_back(a);
            // (nobody reads bgr_aligner_kernel_times here: no events around the kernels -- they cost a 262 144-read piece's mapping launch a tenth of its time)
            (void)bgr_aligner_set_knob(a, BGR_KNOB_KERNEL_EVENTS, 0);
            if (counts) rc = bgr::g_run_counts.enable(a, counts);  // every launch of the run is followed by the kernels of what it counts (bgr_align_all has checked the table)
            if (rc == BGR_OK && s.tag_table) rc = bgr::g_run_counts.haplotag_enable(a, s.tag_table, s.tag_rows);
            if (rc == BGR_OK && s.gaf_cs) rc = bgr::g_run_counts.gaf_cs_enable(a, 1);
            if (rc == BGR_OK && s.inside) rc = bgr::g_run_counts.inside_enable(a, 1);
            if (rc == BGR_OK && s.exhaustive_paths) rc = bgr::g_run_counts.exhaustive_paths_enable(a, 1);
            if (rc != BGR_OK) return rc;
        }
    }
    return BGR_OK;
}

// ---- what the threads of a run share ------------------------------------------------------------------------------------------
struct OutBufs { std::vector<std::string> pb, nb, ob; };
// what the writer hands to the I/O thread: formatted buffers (host route) or the batch itself, whose page-locked buffers hold the
// two record streams as the device wrote them (text route; the batch is recycled once they are on their way to the files)
struct IoItem { std::unique_ptr<OutBufs> bufs; BatchPtr batch; };

struct Run {
    const RunShape& s;
    const bgr_params* const prm;
    const std::vector<InputSpan>& inputs;
    Outputs out;
    std::vector<AlignerPtr> aligners;
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    WorkerPool pool;
    BatchChannel to_gather, to_out, free_batches;
    std::vector<std::unique_ptr<BatchChannel>> to_gpu;  // one queue per device: its workers and its share of the batches
    Channel<IoItem> to_io{2};
    Channel<std::unique_ptr<OutBufs>> free_bufs{4};
    PinChannel free_pins;
    std::atomic<size_t> created{0};
    std::atomic<unsigned> live_workers;
    std::atomic<uint64_t> us_parse{0}, us_gather{0}, us_gpu{0}, us_format{0}, us_write{0}, us_alloc{0};
    // the first failure wins; `failed` is shared with the other lanes of a split run (`cancel`): a lane that fails stops them all
    std::atomic<bool> failed_here{false};
    std::atomic<bool>& failed;
    bool failed_first = false;  // this pipeline recorded the failure (first_rc / first_err are its own)
    std::mutex err_m;
    std::string first_err;
    int first_rc = BGR_OK;

    Run(const RunShape& shape, const bgr_params* p, const std::vector<InputSpan>& in, Outputs&& o, std::vector<AlignerPtr>&& al, std::atomic<bool>* cancel)
        : s(shape), prm(p), inputs(in), out(std::move(o)), aligners(std::move(al)), pool(shape.threads + 2),  // + 2: the stage threads mostly wait inside run()
          to_gather(shape.max_batches), to_out(shape.max_batches), free_batches(shape.max_batches), free_pins(shape.n_pins + 1),
          live_workers((unsigned)shape.n_aligners), failed(cancel ? *cancel : failed_here) {
        pool.timing = s.timing;
        for (unsigned g = 0; g < s.n_gpus; ++g) to_gpu.push_back(std::make_unique<BatchChannel>(s.max_batches));
        for (int i = 0; i < 3; ++i) {
            auto ob = std::make_unique<OutBufs>();
            ob->pb.resize(s.threads); ob->nb.resize(s.threads); ob->ob.resize(s.threads);
            free_bufs.push(std::move(ob));
        }
    }
    void fail(int rc, const std::string& msg) {
        std::lock_guard<std::mutex> l(err_m);
        if (!failed.exchange(true)) { first_rc = rc; first_err = msg; failed_first = true; }
    }
    bool take_batch(BatchPtr& b) {  // reuse a finished batch; create one only while below the cap
        if (free_batches.try_pop(b)) return true;
        if (created.fetch_add(1) < s.max_batches) { b = std::make_unique<Batch>(); return true; }
        created.fetch_sub(1);
        return free_batches.pop(b);
    }
    void recycle(BatchPtr& b) {  // hand the batch (and its pinned buffers) back to the producer
        if (!b) return;
        if (b->pin) free_pins.push(std::move(b->pin));
        b->recs.clear(); b->marks.clear(); b->chunks.clear(); b->shared_chunks.reset(); b->file.reset(); b->fq_nl.clear();
        free_batches.push(std::move(b));
    }
};

// The pin-allocator thread: the sets of the run, sized from the input (pipeline_support.h: fill_pin_pool).
void allocate_pins(Run& r) {
    const RunShape& s = r.s;
    const uint64_t ta0 = now_us();
    uint64_t total_in = 0, max_file = 0;
    for (const InputSpan& in : r.inputs) {
        uint64_t sz = 0;
        struct stat st;
        if (in.mf) sz = in.mf->size;
        else if (stat(in.file.c_str(), &st) == 0) sz = (uint64_t)st.st_size;
        sz = std::min(sz, in.end) - std::min(sz, in.begin);
        total_in += sz;
        max_file = std::max(max_file, sz);
    }
    PinPlan pl;
    pl.text_route = s.text_route;
    pl.n_sets = s.n_pins;
    const uint64_t group0 = std::max<uint64_t>(s.threads, (s.batch_reads * 170) / s.chunk_bytes);
    pl.bytes = std::min<uint64_t>(max_file, s.fastq ? s.batch_reads * 160 : group0 * s.chunk_bytes);
    pl.reads = std::min<uint64_t>(s.batch_reads + s.batch_reads / 4, pl.bytes / 16 + 1);
    pl.piece = std::min<uint64_t>(max_file, s.fastq ? s.batch_reads * 330 : s.piece_bytes + s.piece_bytes / 16);
    pl.stream = pl.piece / s.out_div + 4096;
    const uint64_t per_set = s.text_route ? pl.piece : pl.bytes;  // (what one set takes of the input)
    pl.n_sized = per_set ? (size_t)std::min<uint64_t>(s.n_pins, (total_in + per_set - 1) / per_set + 1) : 1;
    fill_pin_pool(r.free_pins, pl);
    r.us_alloc += now_us() - ta0;
}

// ---- stage 1: parse ----------------------------------------------------------------------------------------------------------
struct Producer {
    Run& r;
    const RunShape& s;
    uint64_t next_index = 0;
    ProgressMarker marker;
    std::vector<Mark> pending;      // marks waiting for the next batch (they go in front of its first read)
    std::vector<uint64_t> mark_idx;
    bool ok = true;
    // the span of a file this pipeline maps: all of it, or -- a lane of a split run -- from one record start to another
    struct Span { std::shared_ptr<MappedFile> mf; uint64_t begin, size; const char* data() const { return mf->data + begin; } };

    explicit Producer(Run& run) : r(run), s(run.s) { marker.on = s.progress_blocks; }
    bool go() const { return ok && !r.failed; }

    bool open_batch(BatchPtr& b, const std::shared_ptr<MappedFile>& mf) {
        if (!r.take_batch(b)) return false;
        b->file = mf;
        b->bases = 0;
        b->text_piece = b->dev_text = b->fastq_piece = false;
        b->fq_parts.clear();
        b->fq_nl.clear();
        b->t_gathered = 0;
        b->text_origin = b->first_of_file = b->last_of_file = false;
        b->n_attempts = 0;
        b->att_of_read.clear();
        b->marks.clear();
        for (auto& m : pending) { m.pos = 0; b->marks.push_back(std::move(m)); }
        pending.clear();
        return true;
    }
    bool emit(BatchPtr b) {  // number the batch in input order and hand it to the gatherer
        b->index = next_index++;
        b->n = b->recs.size();
        return r.to_gather.push(std::move(b));
    }
    void drop(BatchPtr b) {  // an opened batch that got neither reads nor marks
        b->chunks.clear(); b->shared_chunks.reset(); b->file.reset(); b->recs.clear();
        r.free_batches.push(std::move(b));
    }
    void mark_behind(Batch* b) {  // a progress block due behind the last record so far: in the open batch, or in front of the next one
        if (b) b->marks.push_back({b->recs.size(), 0, ""}); else pending.push_back({0, 0, ""});
    }
    void finish(BatchPtr& b) {  // the open batch at the end of its file
        if (!b) return;
        if (ok && (!b->recs.empty() || !b->marks.empty())) ok = emit(std::move(b));
        else drop(std::move(b));
    }

    // FASTQ, text route: every record in front of the file's last getReads() call boundary is a plain four-line record -- pieces of
    // whole records go to the device as they are, cut while the newline counts of the chunks behind them are still being
    // taken (a boundary is final once the records counted so far reach beyond it); the rest of the file (the phantom record
    // at its end, truncated tails: aligner.cpp:51-68) goes through the sequential state machine on the host, behind them
    void fastq_text(const std::shared_ptr<MappedFile>& mf) {
        bgr::FastqPlan plan(mf->data, mf->size, s.chunk_bytes);
        if (s.fastq_gather) plan.keep_newlines();  // (the count pass keeps the newline positions: the gather does not scan again)
        const size_t nc = plan.chunks();
        const size_t wave = std::max<size_t>((size_t)s.threads * 8, 64);
        uint64_t r0 = 0, o0 = 0;
        for (size_t c_done = 0; go();) {
            const size_t c_end = std::min(nc, c_done + wave);
            uint64_t tp0 = now_us();
            if (c_end > c_done) r.pool.run(c_end - c_done, [&plan, c_done](size_t c) { plan.count_chunk(c_done + c); }, 1);
            plan.extend_counts(c_end);
            c_done = c_end;
            const bool last = c_done >= nc;
            if (last) plan.finish_counts();
            r.us_parse += now_us() - tp0;
            const uint64_t counted = plan.records_counted();
            const uint64_t limit = last ? plan.par_records() : (counted ? ((counted - 1) / 10000) * 10000 : 0);
            while (go() && r0 < limit && (last || r0 + s.batch_reads <= limit)) {
                uint64_t r1 = std::min<uint64_t>(limit, r0 + s.batch_reads), o1 = plan.record_offset(r1);
                while (o1 - o0 > (1ull << 30) && r1 > r0 + 1) {  // long reads: a piece stays under the 2 GiB of one call
                    r1 = r0 + (r1 - r0) / 2;
                    o1 = plan.record_offset(r1);
                }
                BatchPtr tb;
                if (!open_batch(tb, mf)) { ok = false; break; }
                tb->text_piece = o1 - o0 < (1ull << 31);  // (one record of 2 GiB: the host parser takes it)
                tb->fastq_piece = true;
                tb->t_begin = o0; tb->t_end = o1;
                if (s.fastq_gather) {
                    plan.piece_parts(o0, o1, r0, tb->fq_parts);
                    tb->fq_chunk_bytes = plan.chunk_bytes();
                    for (const auto& pt : tb->fq_parts) tb->fq_nl.push_back(plan.newlines_of((size_t)(pt.first / plan.chunk_bytes())));
                    plan.release_newlines((size_t)(o1 / plan.chunk_bytes()));  // (chunks wholly in front of the next piece)
                }
                if (!tb->text_piece) {
                    tb->chunks.clear();
                    tb->chunks.push_back(std::make_unique<ParsedChunk>());
                    bgr::parse_fastq_records(mf->data, o0, o1, *tb->chunks[0]);
                    tb->recs = tb->chunks[0]->recs;
                }
                ok = emit(std::move(tb));
                r0 = r1; o0 = o1;
            }
            if (last) break;
        }
        if (!go()) return;
        ParsedChunk tl;
        const uint64_t tp0 = now_us();
        bgr::parse_fastq_from(mf->data, o0, mf->size, tl);
        r.us_parse += now_us() - tp0;
        const std::vector<RecSlice>& rs = tl.recs;
        for (size_t lo = 0; lo < rs.size() && ok;) {
            BatchPtr hb;
            if (!open_batch(hb, mf)) { ok = false; break; }
            const size_t take = std::min<size_t>(rs.size() - lo, (size_t)s.batch_reads);
            hb->recs.assign(rs.begin() + lo, rs.begin() + lo + take);
            lo += take;
            ok = emit(std::move(hb));
        }
    }

    // the records of one parsed FASTQ chunk into the open batch `b` (slices point into the file image only: no joined storage)
    void feed_fastq(const ParsedChunk& ch, BatchPtr& b, const std::shared_ptr<MappedFile>& mf, uint64_t& file_iters) {
        const std::vector<RecSlice>& rs = ch.recs;
        marker.chunk(ch, file_iters, mark_idx);
        file_iters += ch.iters;
        size_t lo = 0, mi = 0;
        while (lo < rs.size() && ok) {
            if (!b && !open_batch(b, mf)) { ok = false; break; }
            size_t take = std::min<size_t>(rs.size() - lo, (size_t)s.batch_reads - b->recs.size());
            uint64_t acc = b->bases;
            for (size_t j = 0; j < take; ++j) {  // long reads: close the batch at ~1 G bases
                acc += rs[lo + j].sl;
                if (acc >= s.batch_bases_cap) { take = j + 1; break; }
            }
            b->bases = acc;
            for (; mi < mark_idx.size() && mark_idx[mi] < lo + take; ++mi) b->marks.push_back({b->recs.size() + (mark_idx[mi] - lo), 0, ""});
            b->recs.insert(b->recs.end(), rs.begin() + lo, rs.begin() + lo + take);
            lo += take;
            if (b->recs.size() >= s.batch_reads || b->bases >= s.batch_bases_cap) ok = emit(std::move(b));
        }
        for (; mi < mark_idx.size(); ++mi) mark_behind(b.get());  // due behind the chunk's last record
    }
    // FASTQ, host route: newline counts first (they fix which line of a record every chunk starts in), then the chunks
    // group by group, so that the later stages already work on the first batches while the rest is parsed
    void fastq_host(const std::shared_ptr<MappedFile>& mf) {
        bgr::FastqPlan plan(mf->data, mf->size, s.chunk_bytes);
        const size_t nc = plan.chunks();
        uint64_t tp0 = now_us();
        r.pool.run(nc, [&plan](size_t c) { plan.count_chunk(c); }, 1);
        plan.finish_counts();
        r.us_parse += now_us() - tp0;
        BatchPtr b;
        uint64_t file_iters = 0;  // getReads() iterations of this file handed on so far
        const size_t group = std::max<size_t>(s.threads, (size_t)((s.batch_reads * 330) / s.chunk_bytes));
        bool tail = plan.sequential_only();
        for (size_t c = 0; c < nc && !tail && go(); c += group) {
            const size_t c_end = std::min(nc, c + group);
            std::vector<ParsedChunk> fq(c_end - c);
            for (auto& ch : fq) ch.track_iters = marker.on;
            std::vector<char> done(c_end - c, 1);
            tp0 = now_us();
            r.pool.run(c_end - c, [&plan, &fq, &done, c](size_t j) { done[j] = plan.parse_chunk(c + j, fq[j]) ? 1 : 0; }, 1);
            r.us_parse += now_us() - tp0;
            for (size_t j = 0; j < fq.size() && ok; ++j) {
                feed_fastq(fq[j], b, mf, file_iters);
                if (!done[j]) { tail = true; break; }  // this chunk ran into the sequential tail: nothing after it is parsed here
            }
        }
        if (go()) {
            ParsedChunk tl;
            tl.track_iters = marker.on;
            tp0 = now_us();
            plan.parse_tail(tl);
            r.us_parse += now_us() - tp0;
            feed_fastq(tl, b, mf, file_iters);
        }
        for (unsigned d = marker.end_file(std::max<uint64_t>(1, file_iters)); d; --d) mark_behind(b.get());
        finish(b);
    }

    // FASTA, text route: pieces of the file as they are -- the device finds the records (the worker falls back per piece)
    void fasta_text(const Span& sp) {
        const std::vector<uint64_t> cuts = bgr::split_fasta(sp.data(), sp.size, s.piece_bytes);
        for (size_t c = 0; c < cuts.size() && go(); ++c) {
            BatchPtr b;
            if (!open_batch(b, sp.mf)) { ok = false; break; }
            b->text_piece = true;
            b->t_begin = sp.begin + cuts[c];
            b->t_end = sp.begin + (c + 1 < cuts.size() ? cuts[c + 1] : sp.size);
            b->text_origin = true;
            b->first_of_file = c == 0;
            b->last_of_file = c + 1 == cuts.size();
            ok = emit(std::move(b));
        }
    }

    // FASTA, host route: chunk-parallel parse, group by group
    void fasta_host(const Span& sp) {
        const std::vector<uint64_t> starts = bgr::split_fasta(sp.data(), sp.size, s.chunk_bytes);
        uint64_t file_iters = 0;  // getReads() iterations of this file handed on so far
        // as many chunks as it takes to reach ~batch_reads (estimated from bytes), at least `threads`
        const size_t group = std::max<size_t>(s.threads, (size_t)((s.batch_reads * 170) / s.chunk_bytes));
        for (size_t c = 0; c < starts.size() && go();) {
            const size_t c_end = std::min(starts.size(), c + group);
            BatchPtr b;
            if (!open_batch(b, sp.mf)) { ok = false; break; }
            // every batch cut from the group keeps the group's storage alive (the records point into it)
            auto keep = std::make_shared<std::vector<std::unique_ptr<ParsedChunk>>>(c_end - c);
            for (auto& ch : *keep) { ch = std::make_unique<ParsedChunk>(); ch->track_iters = marker.on; }
            const uint64_t tp0 = now_us();
            r.pool.run(c_end - c, [&sp, &starts, &keep, c, k = s.k](size_t j) {
                const uint64_t e = (c + j + 1 < starts.size()) ? starts[c + j + 1] : sp.size;
                bgr::parse_fasta_chunk(sp.data(), starts[c + j], e, k, *(*keep)[j]);
            }, 1);
            size_t total = 0;
            for (auto& ch : *keep) total += ch->recs.size();
            b->recs.reserve(total);
            // (one launch addresses its path arena with 32 bits: a group of chunks with very long records -- a large --chunk-bytes,
            // many threads -- is handed on in pieces of at most ~1 G bases, like the FASTQ feeder does)
            b->chunks.clear();
            b->shared_chunks = keep;
            for (auto& ch : *keep) {
                marker.chunk(*ch, file_iters, mark_idx);
                file_iters += ch->iters;
                size_t mi = 0;
                for (size_t ri = 0; ri <= ch->recs.size() && ok; ++ri) {
                    for (; mi < mark_idx.size() && mark_idx[mi] == ri; ++mi) mark_behind(b.get());
                    if (ri == ch->recs.size()) break;
                    b->recs.push_back(ch->recs[ri]);
                    b->bases += ch->recs[ri].sl;
                    if (b->bases >= s.batch_bases_cap) {  // hand this piece on, go on in a fresh batch
                        ok = emit(std::move(b));
                        if (!ok || !open_batch(b, sp.mf)) { ok = false; break; }
                        b->shared_chunks = keep;
                    }
                }
                if (!ok) break;
            }
            r.us_parse += now_us() - tp0;
            c = c_end;
            if (!ok) break;
            if (c >= starts.size())
                for (unsigned d = marker.end_file(std::max<uint64_t>(1, file_iters)); d; --d) mark_behind(b.get());
            finish(b);
        }
    }

    void run() {
        for (size_t fi = 0; fi < r.inputs.size() && go(); ++fi) {  // aligner.cpp:552-586: the files of the comma-separated list, in order
            const InputSpan& in = r.inputs[fi];
            if (s.echo_files) pending.push_back({0, 1, in.file});  // aligner.cpp:559,576  cout<<file<<endl
            std::shared_ptr<MappedFile> mf = in.mf;
            if (!mf) {
                mf = std::make_shared<MappedFile>();
                std::string err;
                if (!mf->open(in.file, err)) { r.fail(BGR_E_IO, "read file: " + err); break; }
            }
            const uint64_t s_begin = std::min(in.begin, mf->size), s_end = std::max(s_begin, std::min(in.end, mf->size));
            if (s.fastq && (s_begin != 0 || s_end != mf->size)) { r.fail(BGR_E_ARG, "bgr_align_all: a FASTQ file is mapped whole (its records are counted from its first line)"); break; }
            marker.begin_file();
            const Span sp{mf, s_begin, s_end - s_begin};
            if (s.fastq) { if (s.text_route) fastq_text(mf); else fastq_host(mf); }
            else if (s.text_route) fasta_text(sp);
            else fasta_host(sp);
        }
        if (go() && !pending.empty()) {  // what is printed after the last read: an empty batch carries it to the writer
            BatchPtr b;
            if (open_batch(b, nullptr)) emit(std::move(b));
        }
        r.to_gather.close();
    }
};
void produce(Run& r) { Producer(r).run(); }

// ---- stage 1b: a batch into (pooled) page-locked memory; called by the gatherer thread and, for a piece that falls back, by a worker ------
// Gathers the sequences of a batch as 2-bit planes.
// false = the batch could not be staged (the error is recorded); it still travels on, so that the writer sees every
// index and recycles every batch (a dropped batch would leave the producer waiting for a free one for ever)
bool gather(Run& r, Batch& b) {
    const unsigned threads = r.s.threads;
    uint64_t bases = 0;
    if (!b.pin && !r.free_pins.pop(b.pin)) { r.fail(BGR_E_INTERNAL, "pinned buffer pool closed"); return false; }
    const uint64_t tg0 = now_us();
    if (!b.pin->offs.ensure((b.n + 1) * 8)) { r.fail(BGR_E_HIP, bgr_last_error()); return false; }
    uint64_t* offs = static_cast<uint64_t*>(b.pin->offs.p);
    for (uint64_t i = 0; i < b.n; ++i) { offs[i] = bases; bases += b.recs[i].sl; }
    offs[b.n] = bases;
    b.bases = bases;
    // typical paths are a handful of ints; the worker fetches again with the full bound if not.  A batch large enough
    // for bgr_align_batch to map it in pieces gets the full bound at once (there is no single result to fetch again).
    b.path_cap = 2 * (bases + 8 * b.n) >= (1ull << 31) ? bases + 8 * b.n + 8 : 8 * b.n + 4096;
    if (!b.pin->fw3.ensure(bgr::packed_plane_words(b.n, bases) * 8) || !b.pin->hasn.ensure((b.n / 32 + 2) * 4) || !b.pin->paths.ensure(b.path_cap * 4) ||
        !b.pin->poffs.ensure((b.n + 1) * 8) || !b.pin->status.ensure(b.n + 1)) { r.fail(BGR_E_HIP, bgr_last_error()); return false; }
    uint64_t* fw3 = static_cast<uint64_t*>(b.pin->fw3.p);
    uint32_t* hasn = static_cast<uint32_t*>(b.pin->hasn.p);
    r.us_alloc += now_us() - tg0;
    const uint64_t tg1 = now_us();
    // pack (instead of copy) the sequences into the page-locked plane: every thread a range of whole bitmap words
    const uint64_t per = (((b.n + threads - 1) / threads) + 31) & ~31ull;
    struct Part { std::vector<uint32_t> idx; std::vector<uint64_t> val; uint32_t max_len = 0; };
    std::vector<Part> parts(threads);
    r.pool.run(threads, [&b, &parts, per, offs, fw3, hasn](size_t t) {
        const uint64_t lo = t * per, hi = std::min<uint64_t>(b.n, lo + per);
        if (lo >= hi) return;
        Part& pt = parts[t];
        std::vector<uint64_t> nm;
        memset(hasn + lo / 32, 0, ((hi - lo + 31) / 32) * 4);
        for (uint64_t i = lo; i < hi; ++i) {
            const uint32_t len = b.recs[i].sl, words = (len + 31) >> 5;
            if (nm.size() < words) nm.resize(words);
            const uint64_t w0 = bgr::packed_word_offset(offs[i], i);
            pt.max_len = std::max(pt.max_len, len);
            if (bgr::pack_read(b.recs[i].s, len, fw3 + w0, nm.data())) {
                hasn[i >> 5] |= 1u << (i & 31);
                for (uint32_t j = 0; j < words; ++j) { pt.idx.push_back((uint32_t)(w0 + j)); pt.val.push_back(nm[j]); }
            }
        }
    }, 2);
    uint64_t nmc = 0;
    b.pin->max_len = 0;
    for (const Part& pt : parts) { nmc += pt.idx.size(); b.pin->max_len = std::max(b.pin->max_len, pt.max_len); }
    b.pin->nm_count = nmc;
    if (nmc) {
        if (!b.pin->nm_idx.ensure(nmc * 4) || !b.pin->nm_val.ensure(nmc * 8)) { r.fail(BGR_E_HIP, bgr_last_error()); return false; }
        uint64_t at = 0;
        for (const Part& pt : parts) {
            if (pt.idx.empty()) continue;
            memcpy(static_cast<uint32_t*>(b.pin->nm_idx.p) + at, pt.idx.data(), pt.idx.size() * 4);
            memcpy(static_cast<uint64_t*>(b.pin->nm_val.p) + at, pt.val.data(), pt.val.size() * 8);
            at += pt.idx.size();
        }
    }
    r.us_gather += now_us() - tg1;
    return true;
}

// text route: the piece of the file into page-locked memory as it is (pread / memcpy in parallel), output buffers sized
bool stage_text(Run& r, Batch& b) {
    const RunShape& s = r.s;
    if (!b.pin && !r.free_pins.pop(b.pin)) { r.fail(BGR_E_INTERNAL, "pinned buffer pool closed"); return false; }
    const uint64_t tg0 = now_us();
    const uint64_t bytes = b.t_end - b.t_begin;
    if (!b.pin->text.ensure(bytes + 64) || !b.pin->ptext.ensure(bytes / s.out_div + 4096) || !b.pin->ntext.ensure(bytes / s.out_div + 4096)) { r.fail(BGR_E_HIP, bgr_last_error()); return false; }
    r.us_alloc += now_us() - tg0;
    const uint64_t tg1 = now_us();
    if (b.pin->stages.size() < s.n_gpus) b.pin->stages.resize(s.n_gpus, nullptr);
    bgr_text_stage*& st = b.pin->stages[b.dev];
    // (a set cached by an earlier run of the process may carry the stage of another device in this place: the index is relative to the run)
    if (st && bgr_text_stage_device(st) != s.device_of(b.dev)) { bgr_text_stage_destroy(st); st = nullptr; }
    if (!st && bgr_text_stage_create(s.device_of(b.dev), &st) != BGR_OK) { r.fail(BGR_E_HIP, bgr_last_error()); return false; }
    if (b.fastq_piece && !b.fq_parts.empty()) {
        // FASTQ: the header and read lines of every part, gathered where the part's bytes would have gone (never more than they are);
        // the parts travel one after the other and lie back to back on the device
        const size_t np = b.fq_parts.size();
        std::vector<const char*> ptrs(np);
        std::vector<uint64_t> lens(np);
        r.pool.run(np, [&b, &ptrs, &lens, np](size_t j) {
            const uint64_t lo = b.fq_parts[j].first, hi = j + 1 < np ? b.fq_parts[j + 1].first : b.t_end;
            char* dst = static_cast<char*>(b.pin->text.p) + (lo - b.t_begin);
            ptrs[j] = dst;
            const std::vector<uint32_t>* nl = j < b.fq_nl.size() ? b.fq_nl[j].get() : nullptr;
            lens[j] = nl ? bgr::fastq_gather_lines_at(b.file->data, lo, hi, b.fq_parts[j].second, dst, nl->data(), nl->size(), (lo / b.fq_chunk_bytes) * b.fq_chunk_bytes)
                         : bgr::fastq_gather_lines(b.file->data, lo, hi, b.fq_parts[j].second, dst);
        }, 2);
        r.us_gather += now_us() - tg1;
        b.t_gathered = 0;
        for (uint64_t l : lens) b.t_gathered += l;
        if (bgr_text_stage_upload_parts(st, (uint32_t)np, ptrs.data(), lens.data()) != BGR_OK) { r.fail(BGR_E_HIP, bgr_last_error()); return false; }
        return true;
    }
    const uint64_t part = 4ull << 20;
    const size_t parts = (size_t)((bytes + part - 1) / part);
    std::atomic<bool> okc{true};
    r.pool.run(parts, [&b, &okc, part, bytes](size_t j) {
        const uint64_t lo = j * part, len = std::min<uint64_t>(part, bytes - lo);
        if (!b.file->copy_out(static_cast<char*>(b.pin->text.p) + lo, b.t_begin + lo, len)) okc = false;
    }, 2);
    r.us_gather += now_us() - tg1;
    if (!okc) { r.fail(BGR_E_IO, "read error on the read file"); return false; }
    // ... and on towards its device at once, on the stage's own copy stream: the worker's call finds it there (or waits on the device)
    if (bgr_text_stage_upload(st, static_cast<const char*>(b.pin->text.p), bytes) != BGR_OK) { r.fail(BGR_E_HIP, bgr_last_error()); return false; }
    return true;
}

// a text piece through the host parser after all (the device found it irregular, or the file has shown to be): the exact
// getReads state machine, chunk-parallel, then the batch goes the host route (gather, bgr_align_batch_packed, host formatter)
void host_parse_piece(Run& r, Batch& b) {
    const RunShape& s = r.s;
    const uint64_t tp0 = now_us();
    const char* base = b.file->data + b.t_begin;
    const uint64_t bytes = b.t_end - b.t_begin;
    b.chunks.clear();
    b.text_piece = b.dev_text = false;
    if (b.fastq_piece) {  // whole four-line records
        b.chunks.push_back(std::make_unique<ParsedChunk>());
        bgr::parse_fastq_records(base, 0, bytes, *b.chunks[0]);
        b.recs = b.chunks[0]->recs;
    } else {
        const std::vector<uint64_t> starts = bgr::split_fasta(base, bytes, s.chunk_bytes);
        b.chunks.resize(starts.size());
        for (auto& ch : b.chunks) { ch = std::make_unique<ParsedChunk>(); ch->track_iters = s.text_progress; }
        r.pool.run(starts.size(), [&b, &starts, base, bytes, k = s.k](size_t j) {
            const uint64_t e = j + 1 < starts.size() ? starts[j + 1] : bytes;
            bgr::parse_fasta_chunk(base, starts[j], e, k, *b.chunks[j]);
        }, 1);
        b.recs.clear();
        b.att_of_read.clear();
        b.n_attempts = 0;
        for (auto& ch : b.chunks) {
            b.recs.insert(b.recs.end(), ch->recs.begin(), ch->recs.end());
            if (s.text_progress) for (uint32_t it : ch->rec_iter) b.att_of_read.push_back(b.n_attempts + it);  // (iterations of the piece: chunk after chunk)
            b.n_attempts += ch->iters;
        }
    }
    b.n = b.recs.size();
    r.us_parse += now_us() - tp0;
}

void gather_batches(Run& r) {  // the gatherer thread
    BatchPtr b;
    while (r.to_gather.pop(b)) {
        b->dev = (unsigned)(b->index % r.s.n_gpus);
        // this file is not of the device's shape: host route from here on.  So is a piece beyond what one text call takes: a piece is
        // cut at record starts, so a very long record can carry it past the 2 GiB of a call, or past kTextPieceMax bytes, the bound that
        // keeps the u32 offsets of the formatted streams exact (a path int is at most 12 characters and consumes at least one base)
        if (b->text_piece && !b->fastq_piece && (b->file->irregular_pieces.load() >= 2 || b->t_end - b->t_begin > RunShape::kTextPieceMax)) host_parse_piece(r, *b);
        if (r.failed || !(b->text_piece ? stage_text(r, *b) : gather(r, *b))) { if (!r.to_out.push(std::move(b))) break; continue; }
        const unsigned dv = b->dev;
        if (!r.to_gpu[dv]->push(std::move(b))) break;
    }
    r.to_gather.close();  // (after a failure: unblock the producer)
    for (auto& q : r.to_gpu) q->close();
}

// ---- stage 2: the stream workers ----------------------------------------------------------------------------------------------
// FASTA / FASTQ bytes in, record bytes out (bgr_align_fasta_text); an irregular piece goes through the host parser and stays a packed batch
void map_text_piece(Run& r, bgr_aligner* a, Batch& b) {
    const RunShape& s = r.s;
    const uint64_t tq0 = now_us();
    bgr_text_batch tb;
    memset(&tb, 0, sizeof(tb));
    tb.struct_size = sizeof(tb);
    tb.text = static_cast<const char*>(b.pin->text.p);
    tb.text_bytes = b.t_end - b.t_begin;
    tb.stage = b.pin->stages.size() > b.dev ? b.pin->stages[b.dev] : nullptr;
    tb.fastq = b.fastq_piece ? 1u : 0u;
    if (b.fastq_piece && !b.fq_parts.empty()) {  // gathered: header and read lines only, held by the stage (parts with gaps on the host)
        tb.text = nullptr;
        tb.text_bytes = b.t_gathered;
        tb.fastq = 2u;
    }
    tb.want_output = s.writes ? (s.gaf ? 3u : s.correction ? 2u : 1u) : 0u;
    auto point_at_streams = [&tb, &b]() {
        tb.paths_out = static_cast<char*>(b.pin->ptext.p); tb.paths_cap = b.pin->ptext.cap;
        tb.notaligned_out = static_cast<char*>(b.pin->ntext.p); tb.notaligned_cap = b.pin->ntext.cap;
    };
    point_at_streams();
    int rc = BGR_OK;
    if (s.text_progress) {  // what became of every record: the writer's progress blocks
        const uint64_t words = tb.text_bytes / 24 + 1024;
        if (!b.pin->info.ensure(words * 4)) rc = BGR_E_HIP;
        tb.record_info_out = static_cast<uint32_t*>(b.pin->info.p);
        tb.record_info_cap = words;
    }
    if (rc == BGR_OK) rc = bgr_align_fasta_text(a, r.prm, &tb);
    if (rc == BGR_E_CAPACITY) {  // unusually long records: the same device results into larger buffers
        if (!b.pin->ptext.ensure(tb.paths_bytes + 64) || !b.pin->ntext.ensure(tb.notaligned_bytes + 64)) rc = BGR_E_HIP;
        else { point_at_streams(); rc = bgr_aligner_fetch_text(a, &tb); }
    }
    if (rc != BGR_OK) r.fail(rc, bgr_last_error());
    else if (tb.irregular) {  // (2 = correction mode met a path that spells no walk: the host formatter reproduces the reference's exit)
        if (tb.irregular == 1) b.file->irregular_pieces.fetch_add(1);
        host_parse_piece(r, b);
        if (!gather(r, b)) return;  // (recorded as the run's failure: the batch travels on as it is)
    } else {
        b.dev_text = true;
        b.n = tb.n_accepted;
        b.n_attempts = tb.n_records;
        b.p_bytes = tb.paths_bytes;
        b.n_bytes = tb.notaligned_bytes;
    }
    r.us_gpu += now_us() - tq0;
}

void map_packed(Run& r, bgr_aligner* a, Batch& b) {
    const uint64_t tq0 = now_us();
    bgr_packed_reads pk;
    pk.read_offsets = static_cast<const uint64_t*>(b.pin->offs.p);
    pk.fw3 = static_cast<const uint64_t*>(b.pin->fw3.p);
    pk.hasn = static_cast<const uint32_t*>(b.pin->hasn.p);
    pk.nm_index = static_cast<const uint32_t*>(b.pin->nm_idx.p);
    pk.nm_value = static_cast<const uint64_t*>(b.pin->nm_val.p);
    pk.nm_count = b.pin->nm_count;
    pk.max_read_len = b.pin->max_len;
    int32_t* paths = static_cast<int32_t*>(b.pin->paths.p);
    uint64_t* poffs = static_cast<uint64_t*>(b.pin->poffs.p);
    uint8_t* status = static_cast<uint8_t*>(b.pin->status.p);
    int rc = bgr_align_batch_packed(a, r.prm, &pk, b.n, paths, b.path_cap, poffs, status);
    if (rc == BGR_E_CAPACITY) {  // unusually long paths: fetch the same device results again into a full-size buffer
        b.path_cap = b.bases + 8 * b.n + 8;
        if (!b.pin->paths.ensure(b.path_cap * 4)) rc = BGR_E_HIP;
        else rc = bgr_aligner_fetch(a, b.n, static_cast<int32_t*>(b.pin->paths.p), b.path_cap, poffs, status);
    }
    if (rc != BGR_OK) r.fail(rc, bgr_last_error());
    r.us_gpu += now_us() - tq0;
}

void map_batches(Run& r, size_t w) {  // stream worker w, on aligner w
    BatchPtr b;
    BatchChannel& my_q = *r.to_gpu[w / r.s.per_dev];  // (aligners are created device by device, per_dev each)
    while (my_q.pop(b)) {
        if (!r.failed && b->text_piece) map_text_piece(r, r.aligners[w].get(), *b);
        if (!r.failed && !b->text_piece) map_packed(r, r.aligners[w].get(), *b);
        if (!r.to_out.push(std::move(b))) break;
    }
    if (--r.live_workers == 0) r.to_out.close();
}

// ---- stage 3: format (range-parallel) in batch order, stage 4: one thread writes the formatted buffers ----------------------------
// What the reference's exhaustive worker has counted when it prints its block: aligner.h:68 counters as its single worker has them
// (atomic<uint>: 32-bit wrap-around).
struct ProgressCounts {
    uint32_t reads = 0, aligned = 0, failed = 0, noov = 0, overlaps = 0;
    uint32_t K1 = 0;
    std::chrono::steady_clock::time_point t_start;
    // text route under -b with progress blocks: the writer counts getReads() iterations itself.  A batch is a piece of its file; the
    // device reports what became of each of its records (pin->info: kept << 31 | mapped << 30 | length, record = iteration), a piece that
    // went through the host parser lists the iteration of each of its reads.  Same rule as ProgressMarker::chunk / end_file on the host route.
    ProgressMarker wmark;
    uint64_t w_file_iters = 0;

    void count(bool mapped, uint32_t L) {
        ++reads;
        if (mapped) ++aligned; else ++failed;
        overlaps += L >= K1 ? L - K1 + 1 : 1;  // overlaps += listOverlap.size(): every position (aligner.cpp:318-342)
    }
    void count_reads(const Batch& bt, uint64_t lo, uint64_t hi) {  // exhaustive mode: alignerExhaustive.cpp:35-58
        const uint8_t* st = static_cast<const uint8_t*>(bt.pin->status.p);
        for (uint64_t i = lo; i < hi; ++i) count((st[i] & BGR_ST_MASK) == BGR_ST_ALIGNED, bt.recs[i].sl);
    }
    void count_attempts(const Batch& bt, uint64_t lo, uint64_t hi, uint64_t& rd) {  // iterations [lo, hi) of the piece; rd: cursor into its reads (fallback form)
        if (bt.dev_text) {
            const uint32_t* info = static_cast<const uint32_t*>(bt.pin->info.p);
            for (uint64_t i = lo; i < hi; ++i)
                if (info[i] >> 31) count((info[i] & 0x40000000u) != 0, info[i] & 0x3FFFFFFFu);
        } else {
            uint64_t r1 = rd;
            while (r1 < bt.att_of_read.size() && bt.att_of_read[r1] < hi) ++r1;
            if (r1 > rd) count_reads(bt, rd, r1);
            rd = r1;
        }
    }
    void print_block() const {  // alignerExhaustive.cpp:306-316
        const uint32_t got = aligned + failed;
        std::cout << "Read : " << reads << std::endl;
        std::cout << "No Overlap : " << noov << " Percent : " << (100 * float(noov)) / reads << std::endl;
        std::cout << "Got Overlap : " << got << " Percent : " << (100 * float(got)) / reads << std::endl;
        std::cout << "Overlap and Aligned : " << aligned << " Percent : " << (100 * float(aligned)) / got << std::endl;
        std::cout << "Overlap but no aligne: " << failed << " Percent : " << (100 * float(failed)) / got << std::endl;
        const auto secs = std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - t_start).count();
        std::cout << "Reads/seconds : " << reads / (uint64_t)(secs + 1) << std::endl;
        // (the reference divides by zero here -- and dies -- when no read has been counted yet)
        std::cout << "Overlap per reads : " << (got ? overlaps / got : 0u) << std::endl;
        std::cout << std::endl;
    }
    void text_piece(const Batch& bt) {
        if (bt.first_of_file) { wmark.begin_file(); w_file_iters = 0; }
        uint64_t at = 0, rd = 0;
        while (wmark.next_fc * kRefBatch < w_file_iters + bt.n_attempts) {  // a block is due in front of iteration `rel` of this piece
            const uint64_t rel = wmark.next_fc * kRefBatch > w_file_iters ? wmark.next_fc * kRefBatch - w_file_iters : 0;
            count_attempts(bt, at, rel, rd);
            at = rel;
            print_block();
            wmark.next_fc += 10;
        }
        count_attempts(bt, at, bt.n_attempts, rd);
        w_file_iters += bt.n_attempts;
        if (bt.last_of_file)
            for (unsigned d = wmark.end_file(std::max<uint64_t>(1, w_file_iters)); d; --d) print_block();
    }
    // what the reference prints between the reads of a batch, in input order
    void between_reads(const RunShape& s, const Batch& cur) {
        uint64_t at = 0;
        const bool own_count = s.text_progress && cur.text_origin;  // (its marks are file names only; the iterations are counted in text_piece)
        for (const Mark& mk : cur.marks) {
            if (s.progress_blocks && !own_count) { count_reads(cur, at, mk.pos); at = mk.pos; }
            if (mk.kind == 1) std::cout << mk.text << std::endl; else print_block();
        }
        if (s.progress_blocks && !own_count) count_reads(cur, at, cur.n);
        if (own_count) text_piece(cur);
    }
};

struct OrderedWriter {
    Run& r;
    const RunShape& s;
    ProgressCounts progress;
    bool stop_writing_after_this = false, wrote_last = false;
    std::vector<char> okv;          // per formatter thread: its range spelled (they persist across batches: reset only after a compaction stop)
    std::vector<std::string> bugv;

    explicit OrderedWriter(Run& run) : r(run), s(run.s), okv(s.threads, 1), bugv(s.threads) {
        progress.K1 = s.k - 1;
        progress.t_start = r.t_start;
        progress.wmark.on = s.text_progress;
    }
    // The records of a batch into the buffers of `o`, a range per thread.  false = "bug compaction": like the reference, everything
    // before the offending read is written, nothing after it
    bool format(const Batch& cur, OutBufs& o) {
        const unsigned threads = s.threads;
        const uint64_t per = (cur.n + threads - 1) / threads;
        const int32_t* paths = static_cast<const int32_t*>(cur.pin->paths.p);
        const uint64_t* poffs = static_cast<const uint64_t*>(cur.pin->poffs.p);
        const uint8_t* status = static_cast<const uint8_t*>(cur.pin->status.p);
        r.pool.run(threads, [this, &cur, &o, per, paths, poffs, status](size_t t) {
            o.pb[t].clear(); o.nb[t].clear(); o.ob[t].clear();
            const uint64_t lo = t * per, hi = std::min<uint64_t>(cur.n, lo + per);
            if (lo >= hi) return;
            if (!s.extended) format_range(cur.recs.data(), paths, poffs, lo, hi, o.pb[t], o.nb[t]);
            else okv[t] = format_range_ext(cur.recs.data(), paths, poffs, status, lo, hi, (s.correction || s.gaf) ? &s.unitigs : nullptr, s.gaf, s.split_no_overlap, o.pb[t], o.nb[t],
                                           o.ob[t], bugv[t], s.tag_table, s.tag_rows, s.gaf_cs, s.exhaustive_paths && s.gaf) ? 1 : 0;
        }, 3);
        unsigned t_stop = threads;
        for (unsigned t = 0; t < threads; ++t)
            if (!okv[t]) { t_stop = t; break; }
        if (t_stop == threads) return true;
        r.fail(BGR_E_COMPACTION, "bug compaction\n" + bugv[t_stop]);
        for (unsigned t = t_stop + 1; t < threads; ++t) { o.pb[t].clear(); o.nb[t].clear(); o.ob[t].clear(); }
        for (auto& ok1 : okv) ok1 = 1;
        return false;
    }
    // The next batch of the input order.  `cur` is left in place for the caller to recycle unless the I/O thread takes it.
    void take(BatchPtr& cur) {
        if (!r.failed) progress.between_reads(s, *cur);
        if ((r.failed && !stop_writing_after_this) || !s.writes || wrote_last || cur->n == 0) return;
        IoItem item;
        if (cur->dev_text) {  // the record streams are ready as they are
            item.batch = std::move(cur);
            r.to_io.push(std::move(item));
            return;
        }
        if (!r.free_bufs.pop(item.bufs)) return;
        const uint64_t tf0 = now_us();
        if (!format(*cur, *item.bufs)) stop_writing_after_this = true;
        r.us_format += now_us() - tf0;
        r.to_io.push(std::move(item));  // the formatted records never point into the batch: it can be recycled now
        if (stop_writing_after_this) wrote_last = true;
    }
    void run() {
        std::map<uint64_t, BatchPtr> pending;
        uint64_t want = 0;
        BatchPtr b;
        while (r.to_out.pop(b)) {
            pending[b->index] = std::move(b);
            while (!pending.empty() && pending.begin()->first == want) {
                BatchPtr cur = std::move(pending.begin()->second);
                pending.erase(pending.begin());
                ++want;
                take(cur);
                r.recycle(cur);
            }
        }
        r.to_io.close();
    }
};
void write_in_order(Run& r) { OrderedWriter(r).run(); }

struct Bytes { const void* p; size_t n; };
void write_list(Run& r, FILE* f, const std::vector<Bytes>& list, const char* error) {
    for (const Bytes& b : list)
        if (b.n && fwrite(b.p, 1, b.n, f) != b.n) r.fail(BGR_E_IO, error);
}
void write_files(Run& r) {  // the I/O thread
    IoItem it;
    std::vector<Bytes> pl, nl, ol;
    while (r.to_io.pop(it)) {
        const uint64_t tw0 = now_us();
        pl.clear(); nl.clear(); ol.clear();
        if (it.batch) {
            pl.push_back({it.batch->pin->ptext.p, it.batch->p_bytes});
            nl.push_back({it.batch->pin->ntext.p, it.batch->n_bytes});
        } else {
            for (const std::string& x : it.bufs->pb) pl.push_back({x.data(), x.size()});
            for (const std::string& x : it.bufs->nb) nl.push_back({x.data(), x.size()});
            for (const std::string& x : it.bufs->ob) ol.push_back({x.data(), x.size()});
        }
        r.pool.run(2, [&r, &pl, &nl, &ol](size_t w) {  // the files are independent streams: one writer each
            if (w == 0) write_list(r, r.out.paths.get(), pl, "write to the paths file failed");
            else {
                write_list(r, r.out.notaligned.get(), nl, "write to the notAligned file failed");
                if (r.out.no_overlap) write_list(r, r.out.no_overlap.get(), ol, "write to the no-overlap file failed");
            }
        }, 4);
        r.us_write += now_us() - tw0;
        if (it.batch) r.recycle(it.batch);
        else r.free_bufs.push(std::move(it.bufs));
    }
}

}  // namespace
