// main.cpp -- `bgreat`: command-line twin of the reference driver (bgreat.cpp:54-130 + Aligner::alignAll,
// aligner.cpp:550-597) on top of the C-ABI of include/bgreat_gpu.h.  Same flags, same files, same stdout
// lines; the per-read work runs on the GPU(s).  Host code only -- no algorithm here.
//
//   bgreat -r reads.fa[,more.fa] -k 31 -g unitigs.fa -m 2 -t 8 [-e effort] [-f paths] [-a notAligned.fa] [-q] [-b] [-i]
//   extensions (opt-in, absent from the reference): --gpus N  (shard each batch over N devices, input order kept)
//                                                   --batch N (reads per device batch, default 128k)
//                                                   --write-exhaustive (-b normally writes nothing)
//                                                   --chunk-bytes N (parser chunk size; tests use tiny chunks)
//                                                   --no-overlap FILE (reads without any anchor go there instead of notAligned.fa)
//                                                   --split-output (with --gpus N: one pipeline per device, device d writes <paths>.<d> /
//                                                                   <notAligned>.<d>; `cat` in device order = the reference's files)
//                                                   --host-route (parse and format on the host always; default: FASTA goes through the
//                                                                 device as text when the run writes the reference's two files)
//                                                   --gaf (the paths file holds one GAF line per mapped read -- name, query interval, strand, the path's
//                                                          segments with their orientations, path interval, matches, NM:i -- instead of
//                                                          header + path ints; greedy modes, ACGT-only unitigs, not with -c: include/bgreat_gpu.h)
//                                                   --abundance FILE (per unitig: the reads, bases and k-mers mapped onto it, counted on the device while mapping; one
//                                                                     tab-separated line per unitig; greedy modes; the other outputs stay as they are)
//                                                   --gfa FILE (the graph the run's reads support, as GFA 1.0: every unitig as an S line under the 1-based ordinal the paths
//                                                               file and --gaf use, with its read and k-mer counts, and every link that a mapped read's path crosses
//                                                               as an L line with its count, counted on the device while mapping; greedy modes: include/bgreat_gpu.h)
//                                                   --pileup FILE, --depth FILE (per base of every unitig: how many reads cover it and, by read character, how many differ from it,
//                                                               counted on the device while mapping; --pileup writes one line per position with a count, --depth one
//                                                               bedGraph-like line per run of equal depth; greedy modes, ACGT-only unitigs: include/bgreat_gpu.h)
//                                                   --vcf FILE [--min-depth N] [--min-alt N] [--min-af F] (the SNV sites on the unitigs as VCF 4.2, CHROM the 1-based ordinal of the paths file: a base
//                                                               covered by at least N reads (2) where a letter other than the unitig's is read at least N times (2) and in
//                                                               at least the fraction F of the covering reads (0.2: a decimal with at most six places); called on the
//                                                               device from the pileup counted while mapping -- the table never crosses to the host; greedy modes, ACGT-only
//                                                               unitigs: include/bgreat_gpu.h)
//                                                   --strands [--min-alt-strand N] (with --pileup and / or --vcf: count the pileup per strand as well -- a read counts forward on a unitig when, as given
//                                                               in the input, it runs along the strand the unitig file spells; --pileup FILE gains the columns depth+ A+ C+ G+ T+ N+,
//                                                               --vcf FILE the INFO fields ADF / ADR, and an ALT must be read at least N times (0) on each strand;
//                                                               --min-alt-strand implies --strands and needs --vcf)
//                                                   --bubbles FILE [--min-link N] (the variants the graph already holds: a unitig that leaves through two links to two branch unitigs which
//                                                               both rejoin one unitig, called on the device from the run's link counts -- a link counts when at least
//                                                               N (1) mapped reads cross it; one tab-separated line per bubble with the four signed ids, the branches'
//                                                               lengths, the four link counts and how the branches differ (snv with pos:X>Y, mnv, indel); counts links
//                                                               and unitig abundance as --gfa does; greedy modes, ACGT-only unitigs: include/bgreat_gpu.h)
//                                                   --triples FILE (every three consecutive unitigs that a mapped read's path threads -- which way into a unitig goes with which way out of
//                                                               it -- with its count, counted on the device while mapping; one tab-separated line "from via to count" per
//                                                               canonical triple, signed ids as in the paths file; counts unitig abundance as --gfa does; greedy modes)
//                                                   --phase FILE [--min-link N] (read-backed phasing: every two bubbles of --bubbles that share a unitig, with the counts of the four
//                                                               in x out combinations of their branches that the reads thread, and cis / trans / . ; counts links and
//                                                               triples and calls the bubbles as --bubbles and --triples do; greedy modes, ACGT-only unitigs)
//                                                   --blocks FILE [--min-phase N] [--min-link N] (haplotype blocks: the pairs of --phase chained on the device -- which bubbles hang together, in what
//                                                               order, and which branch of each lies on the haplotype of the first bubble's first branch; a pair
//                                                               joins two bubbles when its cis and trans counts differ by at least N (1); one tab-separated line per
//                                                               bubble with its block, place, the block's size, the bubble's line in --bubbles, the ids as the block
//                                                               reads them and whether the block is a ring; counts and calls what --phase does: include/bgreat_gpu.h)
//                                                   --haplotypes FILE [--min-block N] [--min-phase N] [--min-link N] (the two sequences every block of --blocks stands for, spelled on
//                                                               the device from the graph's 2-bit store: per sequence a line ">block<b>_<A|B> bubbles= length= ring= walk=" and
//                                                               the sequence on one line; blocks of fewer than N (1) bubbles are left out; counts, calls and chains what
//                                                               --blocks does: include/bgreat_gpu.h)
//                                                   --recompact FILE [--min-reads N] (the unitigs that at least N (1; 0 keeps all) mapped reads' paths hold, merged into maximal
//                                                               non-branching chains on the device and written as a unitig file for the next run's -g: per chain a line
//                                                               ">ordinal LN:i: unitigs= ring= walk=" and the sequence on one line; counts what --abundance does:
//                                                               include/bgreat_gpu.h)
//                                                   --haplotag BLOCKS_FILE (with --gaf: tag every read with the haplotype it lies on -- BLOCKS_FILE is the --blocks file of an earlier run on the same
//                                                               unitig file, of these reads or of others; a line whose path crosses a branch of a block gains
//                                                               PS:i:<block> HP:i:<0|1|2> ha:i: hb:i: ho:i: (votes for haplotype A, for B, for other blocks), computed on the
//                                                               device where the line is formatted; not with -b: include/bgreat_gpu.h)
//                                                   --cs (with --gaf: every line ends in cs:Z:, minimap2's short difference string -- ":<n>" per run of equal characters, "*<path base><read
//                                                               base>" per difference, in the read's direction, behind NM:i: and the --haplotag fields; computed on the device
//                                                               where the line is formatted; runs with everything --gaf runs with: include/bgreat_gpu.h)
//                                                   --inside (greedy and -G: reads that lie wholly inside one unitig hold no overlap (k-1)-mer and stay unmapped; a pass behind the mapping
//                                                               looks up a sample of their k-mers in an exact index of the unitigs' k-mers and maps them as [offset, +-unitig], so
//                                                               they reach `paths` and every counting flag instead of notAligned.fa; one last line on stdout counts them; not with
//                                                               -b, k > 32 or non-ACGT unitig characters: include/bgreat_gpu.h)
//                                                   --exhaustive-paths (with -b: the paths exhaustive mode finds are output -- --gaf with --cs and --haplotag, --abundance, --gfa, --pileup / --depth,
//                                                               --vcf, --strands, --bubbles, --triples, --phase, --blocks and --haplotypes read them as they read the paths of
//                                                               the greedy modes, without the end offset an exhaustive row carries; with --gaf the two files are filled as
//                                                               --write-exhaustive fills them, GAF lines in `paths`; not without -b, with -i, --inside, or --gaf together
//                                                               with --write-exhaustive: include/bgreat_gpu.h)
//                                                   --set name=value (library option, bgr_set_option: INTEGRATION.md 5; e.g. --set timing=1)
#include <getopt.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bgreat_gpu.h"
#include "recompact_host.h"

static void die(const char* what) {
    fprintf(stderr, "bgreat: %s: %s\n", what, bgr_last_error());
    exit(2);
}

int main(int argc, char** argv) {
    std::string reads, unitigs("unitig.fa"), pathFile("paths"), notAlignedFile("notAligned.fa"), noOverlapFile, abundanceFile, gfaFile, pileupFile, depthFile, vcfFile, bubblesFile, triplesFile, phaseFile, blocksFile, haplotypesFile, haplotagFile, recompactFile;
    int errors = 2, threads = 1, ka = 30, effort = 2, gpus = 1;  // bgreat.cpp:56-66 defaults (k is 30, not 31)
    bgr_variant_params vprm = {2, 2, 200000};   // --min-depth, --min-alt, --min-af
    bool vprm_given = false, strands = false, strand_given = false;
    uint32_t min_alt_strand = 0;   // --min-alt-strand
    uint64_t min_link = 1;         // --min-link
    bool min_link_given = false;
    uint64_t min_phase = 1;        // --min-phase
    bool min_phase_given = false;
    uint64_t min_block = 1;        // --min-block
    bool min_block_given = false;
    uint64_t min_reads = 1;        // --min-reads
    bool min_reads_given = false;
    long batch = 0, chunk_bytes = 0;  // batch 0 = the pipeline's default per route
    bool brute = false, incomplete = false, fastq = false, correction = false, dog = false, write_exh = false, host_route = false, split_out = false, gaf = false, gaf_cs = false, inside = false, exh_paths = false;
    static option longopts[] = {{"gpus", required_argument, nullptr, 1000}, {"batch", required_argument, nullptr, 1001},
                                {"write-exhaustive", no_argument, nullptr, 1002}, {"chunk-bytes", required_argument, nullptr, 1003},
                                {"no-overlap", required_argument, nullptr, 1004}, {"host-route", no_argument, nullptr, 1005}, {"split-output", no_argument, nullptr, 1006},
                                {"set", required_argument, nullptr, 1007}, {"gaf", no_argument, nullptr, 1008}, {"abundance", required_argument, nullptr, 1009}, {"gfa", required_argument, nullptr, 1010},
                                {"pileup", required_argument, nullptr, 1011}, {"depth", required_argument, nullptr, 1012},
                                {"vcf", required_argument, nullptr, 1013}, {"min-depth", required_argument, nullptr, 1014}, {"min-alt", required_argument, nullptr, 1015},
                                {"min-af", required_argument, nullptr, 1016}, {"strands", no_argument, nullptr, 1017}, {"min-alt-strand", required_argument, nullptr, 1018},
                                {"bubbles", required_argument, nullptr, 1019}, {"min-link", required_argument, nullptr, 1020},
                                {"triples", required_argument, nullptr, 1021}, {"phase", required_argument, nullptr, 1022},
                                {"blocks", required_argument, nullptr, 1023}, {"min-phase", required_argument, nullptr, 1024},
                                {"haplotypes", required_argument, nullptr, 1025}, {"min-block", required_argument, nullptr, 1026},
                                {"haplotag", required_argument, nullptr, 1027}, {"cs", no_argument, nullptr, 1028}, {"inside", no_argument, nullptr, 1029},
                                {"exhaustive-paths", no_argument, nullptr, 1030},
                                {"recompact", required_argument, nullptr, 1031}, {"min-reads", required_argument, nullptr, 1032},
                                {nullptr, 0, nullptr, 0}};
    int c;
    while ((c = getopt_long(argc, argv, "r:k:g:m:t:e:f:o:a:biqpcG", longopts, nullptr)) != -1) {  // bgreat.cpp:67
        switch (c) {
            case 'r': reads = optarg; break;
            case 'k': ka = std::stoi(optarg); break;
            case 'g': unitigs = optarg; break;
            case 'm': errors = std::stoi(optarg); break;
            case 't': threads = std::stoi(optarg); break;
            case 'e': effort = std::stoi(optarg); break;
            case 'f': pathFile = optarg; break;
            case 'a': notAlignedFile = optarg; break;
            case 'b': brute = true; break;
            case 'i': incomplete = true; break;
            case 'q': fastq = true; break;
            case 'G': dog = true; break;
            case 'c': correction = true; break;
            case 1000: gpus = std::stoi(optarg); break;
            case 1001: batch = std::stol(optarg); break;
            case 1002: write_exh = true; break;
            case 1003: chunk_bytes = std::stol(optarg); break;
            case 1004: noOverlapFile = optarg; break;
            case 1005: host_route = true; break;
            case 1006: split_out = true; break;
            case 1007: {  // the environment is not read anywhere: options come in here
                const std::string kv = optarg;
                const size_t eq = kv.find('=');
                if (eq == std::string::npos || bgr_set_option(kv.substr(0, eq).c_str(), std::stoll(kv.substr(eq + 1))) != BGR_OK) die("--set name=value");
                break;
            }
            case 1008: gaf = true; break;
            case 1009: abundanceFile = optarg; break;
            case 1010: gfaFile = optarg; break;
            case 1011: pileupFile = optarg; break;
            case 1012: depthFile = optarg; break;
            case 1013: vcfFile = optarg; break;
            case 1014:
            case 1015: {   // a positive integer, digits only
                const std::string v = optarg;
                if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos || std::stol(v) < 1) {
                    fprintf(stderr, "bgreat: %s takes a positive integer, not '%s'\n", c == 1014 ? "--min-depth" : "--min-alt", optarg);
                    return 2;
                }
                (c == 1014 ? vprm.min_depth : vprm.min_alt) = (uint32_t)std::stol(v);
                vprm_given = true;
                break;
            }
            case 1016:
                if (bgr_parse_af_ppm(optarg, &vprm.min_af_ppm) != BGR_OK) die("--min-af");
                vprm_given = true;
                break;
            case 1017: strands = true; break;
            case 1018: {   // a non-negative integer, digits only
                if (bgr_parse_min_alt_strand(optarg, &min_alt_strand) != BGR_OK) {
                    fprintf(stderr, "bgreat: --min-alt-strand takes a non-negative integer of at most nine digits, not '%s'\n", optarg);
                    return 2;
                }
                strands = strand_given = true;
                break;
            }
            case 1019: bubblesFile = optarg; break;
            case 1020: {   // a positive integer, digits only
                const std::string v = optarg;
                if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos || std::stol(v) < 1) {
                    fprintf(stderr, "bgreat: --min-link takes a positive integer of at most nine digits, not '%s'\n", optarg);
                    return 2;
                }
                min_link = (uint64_t)std::stol(v);
                min_link_given = true;
                break;
            }
            case 1021: triplesFile = optarg; break;
            case 1022: phaseFile = optarg; break;
            case 1023: blocksFile = optarg; break;
            case 1024: {   // a positive integer, digits only
                const std::string v = optarg;
                if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos || std::stol(v) < 1) {
                    fprintf(stderr, "bgreat: --min-phase takes a positive integer of at most nine digits, not '%s'\n", optarg);
                    return 2;
                }
                min_phase = (uint64_t)std::stol(v);
                min_phase_given = true;
                break;
            }
            case 1025: haplotypesFile = optarg; break;
            case 1026: {   // a positive integer, digits only
                const std::string v = optarg;
                if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos || std::stol(v) < 1) {
                    fprintf(stderr, "bgreat: --min-block takes a positive integer of at most nine digits, not '%s'\n", optarg);
                    return 2;
                }
                min_block = (uint64_t)std::stol(v);
                min_block_given = true;
                break;
            }
            case 1027: haplotagFile = optarg; break;
            case 1028: gaf_cs = true; break;
            case 1029: inside = true; break;
            case 1030: exh_paths = true; break;
            case 1031: recompactFile = optarg; break;
            case 1032:   // a non-negative integer, digits only: 0 keeps every unitig
                if (!bgr::recompact_parse_min_reads(optarg, &min_reads)) {
                    fprintf(stderr, "bgreat: --min-reads takes a non-negative integer of at most nine digits, not '%s'\n", optarg);
                    return 2;
                }
                min_reads_given = true;
                break;
            default: break;  // -o and -p are accepted and ignored, as in the reference (no `case`)
        }
    }
    if (reads.empty()) {  // bgreat.cpp:117-127
        std::cout << "-r read_file" << std::endl << "-k k_value (30)" << std::endl << "-g unitig_file (unitig.dot)" << std::endl
                  << "-m n_missmatch (2)" << std::endl << "-t n_thread (1)" << std::endl << "-e effort put in mapping (2)" << std::endl
                  << "-f path_file (paths)" << std::endl << "-a not_aligned_file (notAligned.fa)" << std::endl
                  << "-p to align on paths instead of walks" << std::endl << "-q for fastq read file" << std::endl
                  << "-c to output corrected reads" << std::endl;
        return 0;
    }
    if (vprm_given && vcfFile.empty()) { fprintf(stderr, "bgreat: --min-depth, --min-alt and --min-af are thresholds of --vcf FILE\n"); return 2; }
    if (strand_given && vcfFile.empty()) { fprintf(stderr, "bgreat: --min-alt-strand is a threshold of --vcf FILE\n"); return 2; }
    if (strands && vcfFile.empty() && pileupFile.empty()) { fprintf(stderr, "bgreat: --strands adds the per-strand counts to --pileup FILE and / or --vcf FILE\n"); return 2; }
    if (min_link_given && bubblesFile.empty() && phaseFile.empty() && blocksFile.empty() && haplotypesFile.empty()) { fprintf(stderr, "bgreat: --min-link is the threshold of --bubbles FILE, --phase FILE, --blocks FILE and --haplotypes FILE\n"); return 2; }
    if (min_phase_given && blocksFile.empty() && haplotypesFile.empty()) { fprintf(stderr, "bgreat: --min-phase is the threshold of --blocks FILE and --haplotypes FILE\n"); return 2; }
    if (min_block_given && haplotypesFile.empty()) { fprintf(stderr, "bgreat: --min-block is the threshold of --haplotypes FILE\n"); return 2; }
    if (min_reads_given && recompactFile.empty()) { fprintf(stderr, "bgreat: --min-reads is the threshold of --recompact FILE\n"); return 2; }
    if (!haplotagFile.empty() && !gaf) { fprintf(stderr, "bgreat: --haplotag BLOCKS_FILE adds its fields to the lines of --gaf\n"); return 2; }
    if (exh_paths && !brute) { fprintf(stderr, "bgreat: --exhaustive-paths outputs the paths of exhaustive mode: it needs -b\n"); return 2; }
    if (exh_paths && incomplete) { fprintf(stderr, "bgreat: --exhaustive-paths is not defined with -i: a partial path of exhaustive mode may lack its end offset\n"); return 2; }
    if (exh_paths && inside) { fprintf(stderr, "bgreat: --exhaustive-paths and --inside: the inside pass writes rows of the greedy modes; exhaustive mode (-b) is refused\n"); return 2; }
    if (exh_paths && gaf && write_exh) { fprintf(stderr, "bgreat: --gaf and --write-exhaustive both claim the paths file; choose one\n"); return 2; }
    if (!haplotagFile.empty() && brute && !exh_paths) { fprintf(stderr, "bgreat: --haplotag tags GAF lines, which are for the greedy modes; exhaustive mode (-b) writes no paths\n"); return 2; }
    if (gaf_cs && !gaf) { fprintf(stderr, "bgreat: --cs adds the cs:Z: field to the lines of --gaf\n"); return 2; }
    if (inside && brute) { fprintf(stderr, "bgreat: --inside maps the reads greedy mode leaves without an anchor; exhaustive mode (-b) is refused\n"); return 2; }
    if (inside && ka > 32) { fprintf(stderr, "bgreat: --inside indexes one-word k-mers: k <= 32\n"); return 2; }
    if (gpus < 1 || batch < 0) { fprintf(stderr, "bgreat: --gpus and --batch must be positive\n"); return 2; }

    auto t0 = std::chrono::system_clock::now();
    bgr_graph* graph = nullptr;
    bgr_set_build_threads((uint32_t)std::max(1, threads));
    if (bgr_graph_build_from_fasta_ex(unitigs.c_str(), (uint32_t)ka, 0.0, dog ? BGR_BUILD_ANCHORS : 0u, &graph) != BGR_OK) die("index");
    if (!haplotagFile.empty()) {   // (before anything is mapped: a file that does not parse ends the run here, with the line named)
        bgr_graph_info_t gi;
        if (bgr_graph_info(graph, &gi) != BGR_OK) die("--haplotag");
        std::vector<uint32_t> table(gi.n_unitigs + 1);
        if (bgr_read_blocks_tags(haplotagFile.c_str(), gi.n_unitigs, table.data(), nullptr) != BGR_OK || bgr_graph_haplotag_enable(graph, table.data(), table.size()) != BGR_OK) die("--haplotag");
    }
    if (gaf_cs && bgr_graph_gaf_cs_enable(graph, 1) != BGR_OK) die("--cs");
    if (exh_paths && bgr_graph_exhaustive_paths_enable(graph, 1) != BGR_OK) die("--exhaustive-paths");
    if (inside && (bgr_graph_inside_build(graph) != BGR_OK || bgr_graph_inside_enable(graph, 1) != BGR_OK)) die("--inside");   // (k > 32, non-ACGT unitig characters: refused here, status 2)
    // one host -> device copy, then device to device over xGMI (RCCL broadcast, or peer copies): include/bgreat_gpu.h
    int64_t one_device = 0, timing = 0;  // (test hook: every lane on device 0)
    (void)bgr_get_option("test.lanes_on_one_device", &one_device);
    (void)bgr_get_option("timing", &timing);
    if (bgr_devices_init(graph, 0, one_device ? 1u : (uint32_t)gpus, BGR_FANOUT_AUTO) != BGR_OK) die("device setup");
    auto t1 = std::chrono::system_clock::now();
    std::cout << "Indexing in seconds : " << std::chrono::duration_cast<std::chrono::seconds>(t1 - t0).count() << std::endl;  // aligner.cpp:546

    // -b selects alignPartExhaustive, where -G has no effect (aligner.cpp:563-567, alignerGreedy.cpp:387)
    bgr_params prm = {brute ? (uint32_t)BGR_MODE_EXHAUSTIVE : (dog ? (uint32_t)BGR_MODE_ANCHORS : (uint32_t)BGR_MODE_GREEDY), (uint32_t)errors, (uint32_t)effort, incomplete ? 1u : 0u};
    bgr_run_options opt;
    memset(&opt, 0, sizeof(opt));
    opt.struct_size = sizeof(opt);
    opt.n_gpus = (uint32_t)gpus;
    opt.threads = (uint32_t)std::max(1, threads);   // -t: host threads of the pipeline (the reference: worker threads)
    opt.batch_reads = (uint64_t)batch;
    opt.chunk_bytes = (uint64_t)std::max(0L, chunk_bytes);
    opt.fastq = fastq ? 1 : 0;
    opt.write_exhaustive = write_exh ? 1 : 0;
    opt.echo_files = 1;
    opt.correction = correction ? 1 : 0;
    opt.no_overlap_file = noOverlapFile.empty() ? nullptr : noOverlapFile.c_str();
    opt.route = host_route ? 1u : 0u;
    opt.split_output = split_out ? 1u : 0u;
    opt.gaf = gaf ? 1u : 0u;
    opt.abundance = abundanceFile.empty() ? 0u : 1u;
    if (!gfaFile.empty() && bgr_graph_links_enable(graph, 1) != BGR_OK) die("gfa");   // the run counts unitig abundance and links (the switch is the graph's: bgr_run_options is full)
    if (!bubblesFile.empty() && bgr_graph_bubbles_enable(graph, 1, min_link) != BGR_OK) die("--bubbles");   // (likewise; it implies the counting of links)
    if (!triplesFile.empty() && bgr_graph_triples_enable(graph, 1) != BGR_OK) die("--triples");   // (likewise: unitig abundance and triples)
    if (!phaseFile.empty() && bgr_graph_phase_enable(graph, 1, min_link) != BGR_OK) die("--phase");   // (likewise; it implies links, triples and the bubbles)
    if (!blocksFile.empty() && bgr_graph_blocks_enable(graph, 1, min_link, min_phase) != BGR_OK) die("--blocks");   // (likewise; it implies what --phase does)
    if (!haplotypesFile.empty() && bgr_graph_haplotypes_enable(graph, 1, min_link, min_phase, min_block) != BGR_OK) die("--haplotypes");   // (likewise; it implies what --blocks does)
    if (!recompactFile.empty() && bgr_graph_recompact_enable(graph, 1, min_reads) != BGR_OK) die("--recompact");   // (likewise: unitig abundance, and the kept unitigs compacted when the run ends)
    const bool pileup = !pileupFile.empty() || !depthFile.empty();   // either file switches the counting on (the graph's switch, as --gfa's)
    if (pileup && bgr_graph_pileup_enable(graph, 1) != BGR_OK) die(pileupFile.empty() ? "--depth" : "--pileup");
    const bgr_variant_strand_params sprm = {vprm.min_depth, vprm.min_alt, vprm.min_af_ppm, min_alt_strand};
    if (strands && !pileupFile.empty() && bgr_graph_pileup_strands_enable(graph, 1) != BGR_OK) die("--strands");   // (the forward totals reach the host next to the totals)
    if (!vcfFile.empty() && strands) { if (bgr_graph_variants_strands_enable(graph, &sprm) != BGR_OK) die("--vcf"); }
    else if (!vcfFile.empty() && bgr_graph_variants_enable(graph, &vprm) != BGR_OK) die("--vcf");   // (likewise; it implies the counting of the pileup, whose tables then stay on the devices)
    auto start = std::chrono::system_clock::now();
    uint64_t tot[5] = {0, 0, 0, 0, 0};
    double map_secs = 0;
    const int arc = bgr_align_all(graph, &prm, &opt, reads.c_str(), pathFile.c_str(), notAlignedFile.c_str(), tot, &map_secs);
    if (arc == BGR_E_COMPACTION) {  // aligner.cpp:280-283: cout<<"bug compaction"<<endl; cout<<path<<" "<<unitig<<endl; exit(0);
        std::cout << bgr_last_error() << std::endl;
        bgr_host_cache_release();
        return 0;
    }
    if (arc != BGR_OK) die(vcfFile.empty() ? "mapping" : "mapping (--vcf)");
    if (!abundanceFile.empty()) {  // (behind a run that ended well: a run that stops with "bug compaction" leaves no totals)
        bgr_graph_info_t gi;
        if (bgr_graph_info(graph, &gi) != BGR_OK) die("abundance");
        std::vector<bgr_unitig_abundance> rows(gi.n_unitigs);
        if (bgr_graph_abundance(graph, rows.data(), gi.n_unitigs) != BGR_OK || bgr_write_abundance(abundanceFile.c_str(), graph, rows.data(), gi.n_unitigs) != BGR_OK) die("abundance");
    }
    // the two-call fetch of a run's records: the number first (BGR_E_CAPACITY with it), then the records
    auto fetch = [&](auto call, auto& rows, const char* what) {
        uint64_t n = 0;
        if (call(graph, nullptr, 0, &n) != BGR_OK && n == 0) die(what);
        rows.resize(n);
        if (n && call(graph, rows.data(), n, &n) != BGR_OK) die(what);
    };
    if (!gfaFile.empty()) {  // (likewise)
        bgr_graph_info_t gi;
        if (bgr_graph_info(graph, &gi) != BGR_OK) die("gfa");
        std::vector<bgr_unitig_abundance> rows(gi.n_unitigs);
        std::vector<bgr_link> links;
        if (bgr_graph_abundance(graph, rows.data(), gi.n_unitigs) != BGR_OK) die("gfa");
        fetch(bgr_graph_links, links, "gfa");
        if (bgr_write_gfa(gfaFile.c_str(), graph, rows.data(), gi.n_unitigs, links.data(), links.size()) != BGR_OK) die("gfa");
    }
    // the run's bubbles (called from its merged links) and block entries (chained from its phase records): fetched once, for the first file that names them
    std::vector<bgr_bubble> bubbles;
    std::vector<bgr_block_entry> entries;
    bool have_bubbles = false, have_entries = false;
    auto need_bubbles = [&](const char* what) { if (!have_bubbles) fetch(bgr_graph_bubbles, bubbles, what); have_bubbles = true; };
    auto need_entries = [&](const char* what) { need_bubbles(what); if (!have_entries) fetch(bgr_graph_blocks, entries, what); have_entries = true; };
    if (!bubblesFile.empty()) {
        need_bubbles("--bubbles");
        if (bgr_write_bubbles(bubblesFile.c_str(), graph, bubbles.data(), bubbles.size()) != BGR_OK) die("--bubbles");
    }
    if (!triplesFile.empty()) {  // (the run's aligners' tables, merged and sorted)
        std::vector<bgr_triple> triples;
        fetch(bgr_graph_triples, triples, "--triples");
        if (bgr_write_triples(triplesFile.c_str(), graph, triples.data(), triples.size()) != BGR_OK) die("--triples");
    }
    if (!phaseFile.empty()) {  // (the run has joined its bubbles with its triples)
        std::vector<bgr_phase> recs;
        fetch(bgr_graph_phase, recs, "--phase");
        if (bgr_write_phase(phaseFile.c_str(), graph, recs.data(), recs.size()) != BGR_OK) die("--phase");
    }
    if (!blocksFile.empty()) {  // (the lines name the run's bubbles)
        need_entries("--blocks");
        if (bgr_write_blocks(blocksFile.c_str(), graph, bubbles.data(), bubbles.size(), entries.data(), entries.size()) != BGR_OK) die("--blocks");
    }
    if (!haplotypesFile.empty()) {  // (the run has spelled its blocks; the header lines name the walks over the run's bubbles)
        need_entries("--haplotypes");
        uint64_t n_haps = 0, seq_bytes = 0;
        if (bgr_graph_haplotypes(graph, nullptr, 0, &n_haps, nullptr, 0, &seq_bytes) != BGR_OK && n_haps == 0) die("--haplotypes");
        std::vector<bgr_haplotype> haps(n_haps);
        std::vector<char> seq(seq_bytes);
        if (n_haps && bgr_graph_haplotypes(graph, haps.data(), n_haps, &n_haps, seq.data(), seq_bytes, &seq_bytes) != BGR_OK) die("--haplotypes");
        if (bgr_write_haplotypes(haplotypesFile.c_str(), graph, bubbles.data(), bubbles.size(), entries.data(), entries.size(), haps.data(), n_haps, seq.data(), seq_bytes) != BGR_OK) die("--haplotypes");
    }
    if (!recompactFile.empty()) {  // (the run has compacted the unitigs its reads support: a unitig file for the next run)
        uint64_t n_chains = 0, walk_n = 0, seq_bytes = 0;
        if (bgr_graph_recompact_result(graph, nullptr, 0, &n_chains, nullptr, 0, &walk_n, nullptr, 0, &seq_bytes) != BGR_OK && n_chains == 0) die("--recompact");
        std::vector<bgr_chain> chains(n_chains);
        std::vector<int32_t> walk(walk_n);
        std::vector<char> seq(seq_bytes);
        if (n_chains && bgr_graph_recompact_result(graph, chains.data(), n_chains, &n_chains, walk.data(), walk_n, &walk_n, seq.data(), seq_bytes, &seq_bytes) != BGR_OK) die("--recompact");
        if (bgr_write_recompact(recompactFile.c_str(), graph, chains.data(), n_chains, walk.data(), walk_n, seq.data(), seq_bytes) != BGR_OK) die("--recompact");
    }
    if (!pileupFile.empty() && (strands ? bgr_write_pileup_strands(pileupFile.c_str(), graph) : bgr_write_pileup(pileupFile.c_str(), graph)) != BGR_OK) die("--pileup");   // (likewise: straight from the graph's totals)
    if (!depthFile.empty() && bgr_write_depth(depthFile.c_str(), graph) != BGR_OK) die("--depth");
    if (!vcfFile.empty() && strands) {   // (the 64-byte records of a run that counted strands)
        std::vector<bgr_variant_strand_site> sites;
        fetch(bgr_graph_variant_strand_sites, sites, "--vcf");
        if (bgr_write_vcf_strands(vcfFile.c_str(), graph, &sprm, sites.data(), sites.size()) != BGR_OK) die("--vcf");
    } else if (!vcfFile.empty()) {   // (the run has called the sites: they, not the table, are what the graph keeps)
        std::vector<bgr_variant_site> sites;
        fetch(bgr_graph_variants, sites, "--vcf");
        if (bgr_write_vcf(vcfFile.c_str(), graph, &vprm, sites.data(), sites.size()) != BGR_OK) die("--vcf");
    }
    const uint64_t rn = tot[0], no = tot[1], ali = tot[2], na = tot[3];
    std::cout << "The End" << std::endl;  // aligner.cpp:588-596
    std::cout << "Reads : " << rn << std::endl;
    std::cout << "No overlap : " << no << " Percent : " << (100 * float(no)) / rn << std::endl;
    std::cout << "Got overlap : " << ali + na << " Percent : " << (100 * float(ali + na)) / rn << std::endl;
    std::cout << "Overlap and aligned : " << ali << " Percent : " << (100 * float(ali)) / (ali + na) << std::endl;
    std::cout << "Overlap but not aligned : " << na << " Percent : " << (100 * float(na)) / (ali + na) << std::endl;
    auto end = std::chrono::system_clock::now();
    auto secs = std::chrono::duration_cast<std::chrono::seconds>(end - start).count();
    std::cout << "Reads/seconds : " << rn / (uint64_t)(secs + 1) << std::endl;
    std::cout << "Mapping in seconds : " << secs << std::endl;
    if (inside) {   // (one more line, the last: the lines above are the reference's)
        uint64_t ni = 0;
        if (bgr_graph_inside_count(graph, &ni) != BGR_OK) die("--inside");
        std::cout << "Mapped inside a unitig : " << ni << std::endl;
    }
    if (timing) fprintf(stderr, "bgreat: mapping %.3f s, %.3f Mreads/s end to end\n", map_secs, map_secs > 0 ? rn / map_secs / 1e6 : 0.0);
    bgr_host_cache_release();  // the pipeline's page-locked staging sets (kept for a next run of the process): freed while the HIP runtime is up
    bgr_graph_destroy(graph);
    return 0;
}
