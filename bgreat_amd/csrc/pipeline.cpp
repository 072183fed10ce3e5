// pipeline.cpp -- bgr_align_all: the batch form of Aligner::alignAll (aligner.cpp:550-597) as a host pipeline.
//
//   reference:  N threads, each: lock; getReads(10000); unlock; per read alignRead*; lock; fwrite; unlock
//   here     :  parse (chunk-parallel, exact getReads semantics, fastx.cpp)
//                 -> batches of reads gathered into pinned memory
//                 -> GPU workers (2 per device, each with its own bgr_aligner/stream: H2D, kernel, D2H of
//                    consecutive batches overlap)
//                 -> formatter (range-parallel printPath/record formatting) -> ONE writer, batches in input order
//
// so the bytes written are the reference's `-t 1` stream whatever the thread/GPU count.  Pure host C++: talks to
// the GPU only through the C-ABI (bgr_aligner_create, bgr_align_batch, bgr_host_alloc ...).
//
// One translation unit; its parts live in headers that only this file includes:
//   pipeline_support.h   WorkerPool, Channel, HostBuf, Pinned, the cache of page-locked sets between runs and the pin-allocator's body
//   record_format.h      the bytes of the records: put_int, recover_path (-c), gaf_line (--gaf), format_range / format_range_ext
//   pipeline_stages.h    RunShape (what a run is: plan_run), NodeAffinity, Run (what its threads share), and the stages: Producer (one feeder
//                        per kind of input), the stager (gather, stage_text, host_parse_piece), the stream workers (map_text_piece,
//                        map_packed), the ordered writer with the reference's progress blocks, the I/O thread
//   this file            align_all_impl (one pipeline: shape, resources, threads, totals), align_all_lanes (a split run), bgr_align_all
#include <array>
#include <thread>

#include "pipeline_stages.h"

namespace bgr {
RunCounts g_run_counts = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // run_counts.h: registered by the library's C-ABI units
}

extern "C" void bgr_host_cache_release(void) {
    std::lock_guard<std::mutex> l(g_pin_cache_m);
    g_pin_cache.clear();
}

namespace {

// One pipeline: the devices first_device .. first_device + n_gpus - 1 of `opt` map `inputs` in order into ONE pair of output files.
// `cancel` (optional): shared with the other lanes of a split run -- a lane that fails stops them all.  `counts`: what the run counts (run_counts.h).
int align_all_impl(bgr_graph* graph, const bgr_params* prm, const bgr_run_options* opt, uint32_t counts, const std::vector<InputSpan>& inputs,
                   const char* paths_file, const char* notaligned_file, uint64_t counters_out[5], double* mapping_seconds, std::atomic<bool>* cancel) {
    NodeAffinity affinity(opt);  // (restored when this call returns)
    RunShape shape;
    int rc = plan_run(graph, prm, opt, affinity.threads, shape);
    if (rc != BGR_OK) return rc;
    Outputs out;
    if ((rc = open_outputs(opt, paths_file, notaligned_file, out)) != BGR_OK) return rc;
    std::vector<AlignerPtr> aligners;
    if ((rc = make_aligners(graph, shape, counts, aligners)) != BGR_OK) return rc;
    Run r(shape, prm, inputs, std::move(out), std::move(aligners), cancel);

    std::thread pin_allocator(allocate_pins, std::ref(r));
    std::thread producer(produce, std::ref(r));        // stage 1: parse
    std::thread gatherer(gather_batches, std::ref(r)); // stage 1b: into page-locked memory, on towards the devices
    std::vector<std::thread> workers;                  // stage 2: one per aligner
    for (size_t w = 0; w < r.aligners.size(); ++w) workers.emplace_back(map_batches, std::ref(r), w);
    std::thread io_thread(write_files, std::ref(r));   // stage 4
    std::thread writer(write_in_order, std::ref(r));   // stage 3: format, in input order
    producer.join();
    gatherer.join();
    for (auto& t : workers) t.join();
    writer.join();
    io_thread.join();
    pin_allocator.join();
    park_pin_sets(r.free_pins);
    r.free_pins.close();
    r.free_batches.close();
    r.free_bufs.close();
    r.out = Outputs();  // (closes the files)

    uint64_t tot[5] = {0, 0, 0, 0, 0};
    for (AlignerPtr& a : r.aligners) {
        uint64_t c5[5];
        if (!r.failed && bgr_aligner_counters(a.get(), c5) == BGR_OK) for (int j = 0; j < 5; ++j) tot[j] += c5[j];
        if (!r.failed && counts) {  // likewise its tables of what the run counts: they join the run's totals in the graph
            const int crc = bgr::g_run_counts.collect(graph, a.get(), counts);
            if (crc != BGR_OK) r.fail(crc, bgr_last_error());
        }
        if (!r.failed && shape.inside) {  // and what it mapped inside
            const int irc = bgr::g_run_counts.inside_collect(graph, a.get());
            if (irc != BGR_OK) r.fail(irc, bgr_last_error());
        }
        a.reset();
    }
    if (counters_out) memcpy(counters_out, tot, sizeof(tot));
    if (mapping_seconds) *mapping_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - r.t_start).count();
    if (shape.timing)
        fprintf(stderr, "bgreat: stage busy time (s): parse %.3f  alloc %.3f  gather %.3f  gpu(sum over %zu workers) %.3f  format %.3f  write %.3f\n",
                r.us_parse / 1e6, r.us_alloc / 1e6, r.us_gather / 1e6, r.aligners.size(), r.us_gpu / 1e6, r.us_format / 1e6, r.us_write / 1e6);
    if (shape.timing)  // thread CPU seconds spent inside the pool's tasks, by stage
        fprintf(stderr, "bgreat: pool CPU time (s): parse %.3f  gather/pack %.3f  format %.3f  write %.3f  other %.3f\n", r.pool.cpu_us[1] / 1e6,
                r.pool.cpu_us[2] / 1e6, r.pool.cpu_us[3] / 1e6, r.pool.cpu_us[4] / 1e6, r.pool.cpu_us[0] / 1e6);
    if (r.failed_first) return bgr::set_error(r.first_rc, r.first_err);
    if (r.failed) return bgr::set_error(BGR_E_INTERNAL, "stopped: another lane of the run failed");
    return BGR_OK;
}

}  // namespace

// ---- split run: one pipeline per device (bgr_run_options.split_output) ---------------------------------------------------------
// The reference's N workers share ONE reader and ONE writer under a mutex each (alignerGreedy.cpp:372-377,407-411).  Here every
// device gets a lane of its own -- producer, gatherer, stream workers, ordered writer, output pair -- over a contiguous share of the
// input, so nothing is shared between devices but the graph and the page cache; `cat` of the pairs in device order is the -t 1 stream.
static int align_all_lanes(bgr_graph* graph, const bgr_params* prm, const bgr_run_options* opt, uint32_t counts, const std::vector<std::string>& files,
                           const char* paths_file, const char* notaligned_file, uint64_t counters_out[5], double* mapping_seconds) {
    const unsigned n = std::max<uint32_t>(1, opt->n_gpus);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::shared_ptr<MappedFile>> imgs;
    uint64_t total = 0;
    for (const std::string& f : files) {
        auto mf = std::make_shared<MappedFile>();
        std::string err;
        if (!mf->open(f, err)) return bgr::set_error(BGR_E_IO, "read file: " + err);
        if (opt->echo_files) std::cout << f << std::endl;  // aligner.cpp:559,576 (nothing else is printed while such a run maps)
        total += mf->size;
        imgs.push_back(std::move(mf));
    }
    // lane d: the bytes between cut d and cut d + 1 of the files taken together; a cut is the first record start at or behind d / n of
    // the bytes (fasta_cut_at: where an independent reader is in the sequential reader's state), so every lane parses its share exactly
    // as the one reader would
    struct Cut { size_t file; uint64_t off; };
    std::vector<Cut> cuts(n + 1);
    cuts[0] = {0, 0};
    cuts[n] = {files.size(), 0};
    for (unsigned d = 1; d < n; ++d) {
        const uint64_t target = (uint64_t)((unsigned __int128)total * d / n);
        uint64_t base = 0;
        Cut c = {files.size(), 0};
        for (size_t f = 0; f < imgs.size(); ++f) {
            const uint64_t sz = imgs[f]->size;
            if (target < base + sz) {
                const uint64_t at = target > base ? bgr::fasta_cut_at(imgs[f]->data, sz, target - base) : 0;
                c = at < sz ? Cut{f, at} : Cut{f + 1, 0};
                break;
            }
            base += sz;
        }
        if (c.file < cuts[d - 1].file || (c.file == cuts[d - 1].file && c.off < cuts[d - 1].off)) c = cuts[d - 1];
        cuts[d] = c;
    }
    // the graph on every device of the run before the lanes start: bgr_aligner_create would bring it there too, but the lanes run side by side
    // and the graph's table of resident copies is not made for concurrent writers (a run behind bgr_devices_init finds every copy in place)
    const bool one_device = run_on_one_device();
    for (unsigned d = 0; d < (one_device ? 1u : n); ++d) {
        const int rc = bgr_graph_upload(graph, (int)(opt->first_device + d));
        if (rc != BGR_OK) return rc;
    }
    std::atomic<bool> cancel{false};
    std::vector<int> rcs(n, BGR_OK);
    std::vector<std::string> errs(n);
    std::vector<std::array<uint64_t, 5>> cnt(n);
    std::vector<double> lane_end(n, 0.0), lane_secs(n, 0.0);
    std::vector<std::thread> lanes;
    for (unsigned d = 0; d < n; ++d) {
        lanes.emplace_back([&, d]() {
            std::vector<InputSpan> in;
            for (size_t f = cuts[d].file; f < files.size() && (f < cuts[d + 1].file || (f == cuts[d + 1].file && cuts[d + 1].off > 0)); ++f) {
                InputSpan sp;
                sp.file = files[f];
                sp.mf = imgs[f];
                sp.begin = f == cuts[d].file ? cuts[d].off : 0;
                sp.end = f == cuts[d + 1].file ? cuts[d + 1].off : ~0ull;
                if (std::min(sp.end, imgs[f]->size) > sp.begin || imgs[f]->size == 0) in.push_back(std::move(sp));
            }
            bgr_run_options o = *opt;
            o.n_gpus = 1;
            o.first_device = one_device ? opt->first_device : opt->first_device + d;
            o.threads = std::max<uint32_t>(1, opt->threads / n);
            o.echo_files = 0;
            o.split_output = 0;
            const std::string pf = std::string(paths_file) + "." + std::to_string(d), nf = std::string(notaligned_file) + "." + std::to_string(d);
            cnt[d].fill(0);
            double secs = 0;
            rcs[d] = align_all_impl(graph, prm, &o, counts, in, pf.c_str(), nf.c_str(), cnt[d].data(), &secs, &cancel);
            lane_end[d] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            lane_secs[d] = secs;
            if (bgr::opt("timing")) fprintf(stderr, "bgreat: lane %u (device %u): %llu reads in %.3f s, done %.3f s after the start of the run\n", d, o.first_device, (unsigned long long)cnt[d][0], secs, lane_end[d]);
            if (rcs[d] != BGR_OK) errs[d] = bgr_last_error();  // (the message is the lane thread's own)
        });
    }
    for (auto& t : lanes) t.join();
    if (mapping_seconds) {  // as for one pipeline: from the (first) pipeline's start -- output files open, aligners made -- to the (last) one's end
        double first = 1e300, last = 0;
        for (unsigned d = 0; d < n; ++d) { first = std::min(first, lane_end[d] - lane_secs[d]); last = std::max(last, lane_end[d]); }
        *mapping_seconds = std::max(0.0, last - first);
    }
    int rc = BGR_OK;
    std::string err;
    for (unsigned d = 0; d < n; ++d)   // the lane that failed, not the ones it stopped
        if (rcs[d] != BGR_OK && (rc == BGR_OK || (rc == BGR_E_INTERNAL && err.rfind("stopped:", 0) == 0))) { rc = rcs[d]; err = errs[d]; }
    if (rc != BGR_OK) return bgr::set_error(rc, err);
    if (counters_out) for (int j = 0; j < 5; ++j) { counters_out[j] = 0; for (unsigned d = 0; d < n; ++d) counters_out[j] += cnt[d][j]; }
    return BGR_OK;
}

extern "C" int bgr_align_all(bgr_graph* graph, const bgr_params* prm, const bgr_run_options* opt, const char* reads_csv,
                             const char* paths_file, const char* notaligned_file, uint64_t counters_out[5], double* mapping_seconds) {
    if (!graph || !prm || !opt || !reads_csv || !paths_file || !notaligned_file) return bgr::set_error(BGR_E_ARG, "bgr_align_all: null argument");
    if (opt->struct_size != sizeof(bgr_run_options))
        return bgr::set_error(BGR_E_ARG, "bgr_align_all: bgr_run_options.struct_size is not this library's sizeof(bgr_run_options): the caller was built against another header (zero the struct, set struct_size)");
    {   // (before any device work: a graph with k > 32 keeps two-word keys and maps in greedy mode only)
        bgr_graph_info_t gi;
        if (bgr_graph_info(graph, &gi) != BGR_OK) return BGR_E_ARG;
        if (gi.k > 32 && prm->mode != BGR_MODE_GREEDY)
            return bgr::set_error(BGR_E_ARG, "bgr_align_all: a graph with k > 32 (two-word keys) maps in greedy mode only; exhaustive mode (-b) needs k <= 32");
    }
    std::vector<std::string> files;  // aligner.cpp:552-586: comma-separated list
    {
        const std::string list(reads_csv);
        size_t last = 0;
        for (size_t i = 0; i <= list.size(); ++i) {
            if (i != list.size() && list[i] != ',') continue;
            files.push_back(list.substr(last, i - last));
            last = i + 1;
        }
    }
    const bool progress_blocks = run_progress_blocks(prm, opt), correction = run_correction(prm, opt);
    // bgr_graph_exhaustive_paths_enable: the paths of an exhaustive run are output -- GAF lines and everything that is counted read them without their end
    // offset.  What the definition leaves out is refused before any device work.
    const bool exhaustive_paths = bgr::g_run_counts.exhaustive_paths_wanted && bgr::g_run_counts.exhaustive_paths_wanted(graph) != 0;
    if (exhaustive_paths) {
        if (prm->mode != BGR_MODE_EXHAUSTIVE)
            return bgr::set_error(BGR_E_ARG, "bgr_align_all: the paths of exhaustive mode (--exhaustive-paths, bgr_graph_exhaustive_paths_enable) need exhaustive mode (-b)");
        if (prm->partial)
            return bgr::set_error(BGR_E_ARG, "bgr_align_all: the paths of exhaustive mode (--exhaustive-paths, bgr_graph_exhaustive_paths_enable) are not defined with partial paths (-i): such a row may lack its end offset");
        if (opt->gaf && opt->write_exhaustive)
            return bgr::set_error(BGR_E_ARG, "bgr_align_all: GAF output (--gaf) and --write-exhaustive both claim the paths file; choose one");
    }
    if (opt->gaf) {   // GAF output: what it cannot describe is refused before any device work
        bgr_graph_info_t gi;
        if (bgr_graph_info(graph, &gi) != BGR_OK) return BGR_E_ARG;
        if (prm->mode == BGR_MODE_EXHAUSTIVE && !exhaustive_paths)
            return bgr::set_error(BGR_E_ARG, "bgr_align_all: GAF output (--gaf) is for the greedy modes; exhaustive mode (-b) writes no paths");
        if (opt->correction)
            return bgr::set_error(BGR_E_ARG, "bgr_align_all: GAF output (--gaf) and correction (-c) both claim the paths file; choose one");
        if (gi.has_exceptions)
            return bgr::set_error(BGR_E_ARG, "bgr_align_all: GAF output (--gaf) needs a graph of ACGT-only unitigs: on one with other characters a path read backwards does not spell the reverse complement");
    }
    if (!opt->gaf && bgr::g_run_counts.haplotag_table) {   // tags are fields of GAF lines: a run with the switch on and no GAF output has nowhere to put them
        uint64_t tag_rows = 0;
        if (bgr::g_run_counts.haplotag_table(graph, &tag_rows))
            return bgr::set_error(BGR_E_ARG, "bgr_align_all: haplotags (--haplotag, bgr_graph_haplotag_enable) are fields of GAF lines; the run needs bgr_run_options.gaf (--gaf)");
    }
    if (!opt->gaf && bgr::g_run_counts.gaf_cs_wanted && bgr::g_run_counts.gaf_cs_wanted(graph))   // the same for the cs:Z: field
        return bgr::set_error(BGR_E_ARG, "bgr_align_all: the cs:Z: field (--cs, bgr_graph_gaf_cs_enable) is a field of GAF lines; the run needs bgr_run_options.gaf (--gaf)");
    const bool inside = bgr::g_run_counts.inside_wanted && bgr::g_run_counts.inside_wanted(graph);
    if (inside && prm->mode == BGR_MODE_EXHAUSTIVE)
        return bgr::set_error(BGR_E_ARG, "bgr_align_all: the inside pass (--inside, bgr_graph_inside_enable) writes rows of the greedy modes; exhaustive mode (-b) is refused");
    if (inside) bgr::g_run_counts.inside_begin(graph);
    if (opt->abundance > 1) return bgr::set_error(BGR_E_ARG, "bgr_align_all: bgr_run_options.abundance is 0 or 1");
    // what the run counts (run_counts.h): the graph's sticky switches, which imply unitig abundance whatever bgr_run_options.abundance says, and that option
    const uint32_t counts = (bgr::g_run_counts.wanted ? bgr::g_run_counts.wanted(graph) : 0) | (opt->abundance ? bgr::kCountAbundance : 0);
    // Everything that is counted is defined on the rows of the greedy modes, and refused before any device work: in the words of the most derived
    // feature that asks for it (the pileup's family first, then the links' chain from its end, then the features that stand alone).
    static const struct { uint32_t bit; const char* refusal; } kGreedyOnly[] = {
        {bgr::kCountVariants, "bgr_align_all: SNV sites (--vcf, bgr_graph_variants_enable) are called from the pileup, which is for the greedy modes; the rows of exhaustive mode (-b) have another layout"},
        {bgr::kCountPileup, "bgr_align_all: the pileup (--pileup, --depth, bgr_graph_pileup_enable) is for the greedy modes; the rows of exhaustive mode (-b) have another layout"},
        {bgr::kCountHaplotypes, "bgr_align_all: the haplotypes' sequences (--haplotypes, bgr_graph_haplotypes_enable) are spelled along phased bubbles, which are counted on the rows of the greedy modes; the rows of exhaustive mode (-b) have another layout"},
        {bgr::kCountBlocks, "bgr_align_all: haplotype blocks (--blocks, bgr_graph_blocks_enable) chain phased bubbles, which are counted on the rows of the greedy modes; the rows of exhaustive mode (-b) have another layout"},
        {bgr::kCountPhase, "bgr_align_all: phasing (--phase, bgr_graph_phase_enable) joins bubbles and triples, which are counted on the rows of the greedy modes; the rows of exhaustive mode (-b) have another layout"},
        {bgr::kCountBubbles, "bgr_align_all: bubbles (--bubbles, bgr_graph_bubbles_enable) are called from the link counts, which are for the greedy modes; the rows of exhaustive mode (-b) have another layout"},
        {bgr::kCountLinks, "bgr_align_all: link counting (--gfa, bgr_graph_links_enable) is for the greedy modes; the rows of exhaustive mode (-b) have another layout"},
        {bgr::kCountTriples, "bgr_align_all: triple counting (--triples, bgr_graph_triples_enable) is for the greedy modes; the rows of exhaustive mode (-b) have another layout"},
        {bgr::kCountAbundance, "bgr_align_all: unitig abundance (--abundance) is for the greedy modes; the rows of exhaustive mode (-b) have another layout"},
    };
    if (prm->mode == BGR_MODE_EXHAUSTIVE && !exhaustive_paths)   // (with the switch every one of them reads an exhaustive launch through its view)
        for (const auto& r : kGreedyOnly)
            if (counts & r.bit) return bgr::set_error(BGR_E_ARG, r.refusal);
    if (counts && !bgr::g_run_counts.begin) return bgr::set_error(BGR_E_ARG, "bgr_align_all: unitig abundance is not available in this build");
    if (counts) bgr::g_run_counts.begin(graph, counts);
    int run_rc;
    if (opt->split_output && opt->n_gpus > 1 && !opt->fastq && !progress_blocks && !correction && !opt->gaf && !opt->no_overlap_file)
        run_rc = align_all_lanes(graph, prm, opt, counts, files, paths_file, notaligned_file, counters_out, mapping_seconds);
    else {
        std::vector<InputSpan> inputs(files.size());
        for (size_t i = 0; i < files.size(); ++i) inputs[i].file = files[i];
        run_rc = align_all_impl(graph, prm, opt, counts, inputs, paths_file, notaligned_file, counters_out, mapping_seconds, nullptr);
    }
    if (counts) {   // (the message of a failed run stays; behind a good one the pileup's end refuses totals that may have wrapped)
        const int erc = bgr::g_run_counts.end(graph, counts, run_rc == BGR_OK);
        if (run_rc == BGR_OK) run_rc = erc;
    }
    return run_rc;
}
