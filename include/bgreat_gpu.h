/* bgreat_gpu.h -- C-ABI of libbgreat_gpu.so: the MI355X (gfx950) implementation of BGREAT's per-read
 * de Bruijn-graph mapping path.  Plain pointers and sizes only; no C++/HIP/torch types cross this boundary.
 *
 * The reference (Malfoy/BGREAT) has no plugin/FFI interface.  Its in-process boundary for this path is the
 * worker body alignerGreedy.cpp:378-392 / alignerExhaustive.cpp:273-281, i.e. the member functions
 *
 *     vector<uNumber> Aligner::alignReadGreedy(const string& read, bool& overlapFound, uint errors, bool& rc)
 *                                                       (aligner.h:127, alignerGreedy.cpp:35-57)
 *     vector<uNumber> Aligner::alignReadExhaustive(const string& read, bool& overlapFound, uint errors)
 *                                                       (aligner.h:135, alignerExhaustive.cpp:35-58)
 *
 * called once per read on an immutable Aligner built by Aligner::Aligner + indexUnitigs()
 * (aligner.h:80-105, aligner.cpp:407-547), with side effects only on the counters of aligner.h:68.
 * One-read calls cannot feed a GPU, so every entry point below is the batch form of one of those; each
 * states the reference interface it replaces.  Results are bit-identical to the reference for the same
 * reads in the same order.
 *
 * Conventions: every function returns 0 on success, a negative BGR_E* code otherwise; bgr_last_error()
 * gives the text (thread-local).  Handles are opaque.  Nothing here falls back to a CPU implementation:
 * without a usable HIP device the device functions fail with BGR_E_HIP.
 */
#ifndef BGREAT_GPU_H
#define BGREAT_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGR_OK 0
#define BGR_E_ARG (-1)      /* invalid argument / limit exceeded */
#define BGR_E_HIP (-2)      /* HIP runtime or device failure */
#define BGR_E_IO (-3)       /* file could not be opened / read */
#define BGR_E_CAPACITY (-4) /* caller-provided output buffer too small */
#define BGR_E_INTERNAL (-5)
#define BGR_E_NOMEM (-7)    /* device memory exhausted (exhaustive mode on a unitig set that duplicates its own k-mers: the table of remembered
                               calls of one read's search outgrew what the device can hold -- see BGR_KNOB_EXH_MEMO_CAP) */
#define BGR_E_COMPACTION (-6) /* correction mode: a path does not spell a walk -- the reference's "bug compaction" exit
                                (aligner.cpp:280-283); bgr_last_error() = "bug compaction\n<walk> <unitig>", outputs hold the
                                records before the offending read, as the reference leaves them */

/* status byte of one read (alignReadGreedy's return + overlapFound + rc; alignerGreedy.cpp:35-57):
 *   low 2 bits: 0 = no anchor (noOverlapRead++), 1 = anchored, not aligned (notAligned++), 2 = aligned
 *   bit 2 (4) : the answer was produced on the reverse-complement retry (`rc` out-parameter)           */
#define BGR_ST_NOANCHOR 0
#define BGR_ST_FAILED 1
#define BGR_ST_ALIGNED 2
#define BGR_ST_MASK 3
#define BGR_ST_RC 4

#define BGR_MODE_GREEDY 0      /* alignAll(true, ...)  -> alignReadGreedy      (bgreat.cpp:115, default) */
#define BGR_MODE_EXHAUSTIVE 1  /* alignAll(false, ...) -> alignReadExhaustive  (bgreat.cpp -b)           */
#define BGR_MODE_ANCHORS 2     /* dogMode (bgreat.cpp -G) -> alignReadGreedyAnchors (alignerGreedy.cpp:60-164); the graph
                                  must have been built with BGR_BUILD_ANCHORS */

typedef struct bgr_graph bgr_graph;     /* immutable index: replaces the Aligner's unitigs/MPHF/indices members */
typedef struct bgr_aligner bgr_aligner; /* per-device mapping context: stream, workspaces, counters            */

typedef struct {
    uint32_t mode;         /* BGR_MODE_*                                            */
    uint32_t max_mismatch; /* -m  errorsMax  (bgreat.cpp:78-80, default 2)          */
    uint32_t effort;       /* -e  tryNumber  (bgreat.cpp:84-86, default 2)          */
    uint32_t partial;      /* -i  partial    (bgreat.cpp:96-98; exhaustive only)    */
} bgr_params;

typedef struct {
    uint32_t k, n_levels;  /* n_levels: buckets a key table lookup reads at most (2) */
    uint64_t n_unitigs, n_keys, n_left_keys, n_right_keys, n_fallback; /* n_keys: distinct overlap (k-1)-mers */
    uint64_t total_bases, blob_bytes, mphf_bytes, max_unitig_len;      /* mphf_bytes: size of the overlap key table */
    uint32_t has_exceptions, has_anchors; /* has_anchors: built with BGR_BUILD_ANCHORS (needed by BGR_MODE_ANCHORS) */
    double gamma;  /* key table slots per key */
    uint64_t jump_entries, jump_bytes; /* the jump index of the greedy anchor scan: entries placed, bytes of the section (0: the graph has none) */
    uint32_t jump_stride;              /* it samples every jump_stride-th (k-1)-mer of a unitig */
    uint32_t jump_absent;              /* why the graph has none: BGR_JUMP_* (0: it has one) */
    uint32_t jump_dropped_x1000, jump_reserved; /* 1000 x the share of the sampled (k-1)-mers that found no place in the table */
} bgr_graph_info_t;
#define BGR_JUMP_PRESENT 0u
#define BGR_JUMP_WIDE_KEYS 1u     /* two-word overlap keys (k > 32) */
#define BGR_JUMP_EXCEPTIONS 2u    /* unitig bases outside ACGT */
#define BGR_JUMP_NOT_STAGED 3u    /* the key table is too large to be staged in LDS: the kernel that jumps never runs */
#define BGR_JUMP_OVER_CAP 4u      /* the index would not stay resident in the last-level cache */
#define BGR_JUMP_NOT_COMPACTED 5u /* an interior (k-1)-mer of a unitig is an overlap key (or the index was built with build_jump = 0) */

const char* bgr_last_error(void);

/* Process-wide tuning / diagnostic options.  The library never reads the environment: a host sets what it wants changed here (the CLI:
 * --set name=value) before it creates the objects that look at it (graph build, aligners, bgr_align_all).  Names, defaults and what they
 * replace: INTEGRATION.md section 5; bgr_option_name(i, &what) enumerates them (nullptr behind the last).  Unknown name / value out of
 * range: BGR_E_ARG.  Options named test.* are test hooks. */
int bgr_set_option(const char* name, int64_t value);
int bgr_get_option(const char* name, int64_t* value);
const char* bgr_option_name(uint32_t index, const char** what);
int bgr_device_count(void); /* number of HIP devices visible, 0 if none / no driver */

/* ---- index ----------------------------------------------------------------------------------------
 * Replaces Aligner::Aligner + Aligner::indexUnitigs/indexUnitigsAux (aligner.h:80-105, aligner.cpp:407-547).
 * `seqs`/`offsets[n+1]`: the unitig sequences in file order (ids are 1-based ordinals, as in the reference).
 * Loading stops at the first sequence shorter than k (aligner.cpp:418-420).  gamma = slots per key of the overlap key
 * table that stands in for leftMPHF/rightMPHF + the key compare (1.03 .. 64; <= 0 selects the default: 1.07 when the table can be
 * staged in LDS, else 1.8).
 * The graph is built on the host; inputs are only read during the call.
 * Limits (narrower than the reference's int32 unitig ids, utils.h:26; a graph beyond them is refused with BGR_E_ARG and a message that
 * names the limit, never truncated): k <= 64.  k <= 32 as the reference (whose kmer is a uint64_t); 32 < k <= 64 keeps each (k-1)-mer as two
 * words (the reference's arithmetic on a 2(k-1)-bit integer) and maps in greedy mode only -- with -c, -q, both text routes and
 * several devices -- while exhaustive mode (-b) and the anchors index (-G, BGR_BUILD_ANCHORS) are refused with BGR_E_ARG; fewer than 2^30 unitigs (a slot's id field has 30 bits beside its two
 * orientation bits); fewer than 2^28 overlap keys and fewer than 2^27 - 8 filled neighbour slots (a handle is 28 bits, one of them the
 * "query is canonical" flag travelling with it); the packed sequence of both strands below 4 GiB = 2^34 bases (the kernels address it
 * with 32-bit byte offsets).  The BASELINE configs use 2 % / 0.4 % / 5 % of these (4 M unitigs, 2.6 M keys, 0.8 G bases at chr1 scale). */
/* Host threads of the index build (the reference: BooPHF's `coreNumber` threads, aligner.cpp:450,458); 0 = default
 * (all cores, at most 16).  The built graph does not depend on it.  Process-wide. */
void bgr_set_build_threads(uint32_t threads);
int bgr_graph_build(uint32_t k, uint64_t n_unitigs, const char* seqs, const uint64_t* offsets, double gamma, bgr_graph** out);
/* Same, reading the unitig FASTA exactly as aligner.cpp:415-417 does (2 lines per record, header ignored). */
int bgr_graph_build_from_fasta(const char* unitig_fasta_path, uint32_t k, double gamma, bgr_graph** out);
/* The same two with build flags.  BGR_BUILD_ANCHORS = the reference's dogMode index (`-G`, aligner.cpp:434-442,
 * 457-476): an MPHF over the canonical k-mers of all unitigs plus their (unitig, offset) table, the structure of
 * boomphf::mphf bit for bit because the reference consumes its answers for non-keys too (aligner.cpp:387-389).
 * Costs ~9.5 bytes per unitig base on the host and in HBM. */
#define BGR_BUILD_ANCHORS 1u
#define BGR_BUILD_NO_EVICTIONS 2u /* test hook: the key table is built without eviction walks, so a key that finds both of
                                      its buckets full goes to the sorted fallback list (normally empty); same results, slower */
int bgr_graph_build_ex(uint32_t k, uint64_t n_unitigs, const char* seqs, const uint64_t* offsets, double gamma, uint32_t flags, bgr_graph** out);
int bgr_graph_build_from_fasta_ex(const char* unitig_fasta_path, uint32_t k, double gamma, uint32_t flags, bgr_graph** out);
/* boomphf::mphf::lookup on the anchors index, host side (BooPHF.h:783-818): the index of a canonical k-mer, a false
 * index for many non-keys, UINT64_MAX otherwise; *position_out (may be NULL) = unitig id << 32 | offset stored
 * there.  Used by the CPU tests to pin the index against the oracle's. */
int bgr_graph_anchor_lookup(const bgr_graph* g, uint64_t kmer, uint64_t* index_out, uint64_t* position_out);
/* The overlap key table, host side: the membership test of aligner.cpp:158,219,353,361 ("is this canonical (k-1)-mer an
 * overlap of the graph") as the kernels make it.  *slot_out = the key's slot (its index into the blob's keys / records)
 * or UINT32_MAX for a non-member.  Used by the CPU tests. */
int bgr_graph_key_lookup(const bgr_graph* g, uint64_t canonical_k1mer, uint32_t* slot_out);  /* BGR_E_ARG on a graph with k > 32 */
/* The same for a (k-1)-mer of up to 126 bits given as two words: key_hi = its first k-1-32 bases, key_lo = its last min(k-1, 32)
 * (the integer's high and low 64 bits).  Works on any graph; on one with k <= 32 only key_hi == 0 can be a member. */
int bgr_graph_key_lookup_wide(const bgr_graph* g, uint64_t key_hi, uint64_t key_lo, uint32_t* slot_out);
/* The graph as one position-independent byte blob (what is copied to HBM / broadcast between GPUs). */
const void* bgr_graph_blob(const bgr_graph* g, uint64_t* bytes);
int bgr_graph_from_blob(const void* blob, uint64_t bytes, bgr_graph** out); /* copies the blob */
int bgr_graph_info(const bgr_graph* g, bgr_graph_info_t* out);
/* The jump index of a graph built here (graph_layout.h: buckets of two 8-byte entries), or NULL.  It is NOT part of bgr_graph_blob's bytes -- those
 * are what they always were -- but lies behind them in the graph's storage and in every device copy that bgr_graph_upload / bgr_devices_init make;
 * a graph made from a blob (bgr_graph_from_blob, bgr_graph_adopt_device_blob) has none unless the blob's header names one. */
const void* bgr_graph_jump_index(const bgr_graph* g, uint64_t* bytes);
/* The unitig characters as they were handed to bgr_graph_build (offsets[n+1]; unitig id i is row i-1), the
 * reference's `vector<string> unitigs` (aligner.h:70).  Only graphs built from sequences carry them (not blobs). */
int bgr_graph_unitigs(const bgr_graph* g, const char** seqs, const uint64_t** offsets, uint64_t* n);
void bgr_graph_destroy(bgr_graph* g);

/* Device residency.  upload: hipMalloc + H2D of the blob on `device` (idempotent per device).
 * adopt: the blob already sits in that device's HBM at `dev_blob` (e.g. it was received by an RCCL
 * broadcast from rank 0); the memory stays owned by the caller and must outlive the graph. */
int bgr_graph_upload(bgr_graph* g, int device);
const void* bgr_graph_device_blob(const bgr_graph* g, int device); /* NULL if not resident there */
/* Several GPUs in one process (replaces the thread fan-out of aligner.cpp:577-586 on the device side): makes the graph
 * resident on devices first_device .. first_device + n_devices - 1.  One host -> device copy to the first, then device to
 * device over xGMI: `how` = BGR_FANOUT_AUTO (one RCCL broadcast when librccl can be loaded at run time, else peer copies),
 * BGR_FANOUT_RCCL (ncclCommInitAll + ncclBroadcast, fail if unavailable), BGR_FANOUT_PEER (hipMemcpyPeerAsync in a doubling
 * schedule 1 -> 2 -> 4 -> 8 holders).  bgr_devices_method: what the last call used (0 = nothing to distribute). */
#define BGR_FANOUT_AUTO 0u
#define BGR_FANOUT_RCCL 1u
#define BGR_FANOUT_PEER 2u
int bgr_devices_init(bgr_graph* g, int first_device, uint32_t n_devices, uint32_t how);
uint32_t bgr_devices_method(const bgr_graph* g);
int bgr_graph_adopt_device_blob(int device, const void* dev_blob, uint64_t bytes, bgr_graph** out);

/* ---- mapping --------------------------------------------------------------------------------------
 * bgr_aligner_create replaces the per-thread worker state of alignPartGreedy/alignPartExhaustive
 * (alignerGreedy.cpp:367-371); it uploads the graph to `device` if needed and owns a HIP stream. */
int bgr_aligner_create(bgr_graph* g, int device, bgr_aligner** out);
void bgr_aligner_destroy(bgr_aligner* a);

/* Batch form of alignReadGreedy / alignReadExhaustive over host buffers (H2D, kernel, D2H; blocking).
 *   reads / read_offsets[n+1] : concatenated read sequences exactly as getReads (aligner.cpp:46-117) hands
 *                               them over (characters ACGTN), borrowed for the call.
 *   paths_out[paths_cap], path_offsets[n+1] : CSR of the returned vector<uNumber> per read, INPUT ORDER;
 *                               an empty row means "not mapped" (the reference's empty vector).
 *   status[n] : BGR_ST_* per read.
 * Counters of aligner.h:68 are accumulated in the aligner (bgr_aligner_counters).  Any batch size: one launch
 * addresses its path arena with 32 bits (about 13 M reads of 150 bp); a larger batch is mapped in pieces.     */
int bgr_align_batch(bgr_aligner* a, const bgr_params* p, const char* reads, const uint64_t* read_offsets, uint64_t n_reads,
                    int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status);

/* The same with the reads already packed on the host into the 2-bit planes the kernels read (what bgr_align_device's pre-pass
 * makes on the device): a batch then crosses PCIe at ~0.3 byte per base instead of 1.  Layout: str2num codes (utils.cpp:117-129:
 * A0 C1 G2, else 3), 32 bases per uint64, first base most significant, zero beyond a read's end; read r owns words
 * [(read_offsets[r] >> 5) + r, ... + ceil(len/32)) of `fw3` (bgr_packed_plane_words() words in all; read_offsets[0] must be 0).
 * Reads that hold an N have their bit set in `hasn` and one N-mask word (3 on every N) per word of theirs in the sparse list
 * nm_index[] (plane word index) / nm_value[].  bgr_pack_reads fills all of it from ASCII reads (single thread; ranges of a
 * batch can be packed concurrently with the helpers of bgreat_amd/csrc/read_pack.h, as the CLI's pipeline does). */
typedef struct {
    const uint64_t* read_offsets; /* n+1 base offsets, starting at 0 */
    const uint64_t* fw3;
    const uint32_t* hasn;         /* (n + 31) / 32 words */
    const uint32_t* nm_index;
    const uint64_t* nm_value;
    uint64_t nm_count;
    uint32_t max_read_len;        /* longest read of the batch (0 = have it computed) */
} bgr_packed_reads;
uint64_t bgr_packed_plane_words(uint64_t n_reads, uint64_t total_bases);
int bgr_pack_reads(const char* reads, const uint64_t* read_offsets, uint64_t n_reads, uint64_t* fw3, uint32_t* hasn, uint32_t* nm_index,
                   uint64_t* nm_value, uint64_t nm_cap, uint64_t* nm_count, uint32_t* max_read_len);
int bgr_align_batch_packed(bgr_aligner* a, const bgr_params* p, const bgr_packed_reads* reads, uint64_t n_reads, int32_t* paths_out,
                           uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status);

/* Asynchronous form over host buffers ("asynchronous variant with a stream/ticket for double-buffering"):
 * bgr_align_batch_begin starts the copy of the batch to the device and enqueues the mapping launch on the aligner's stream, then
 * returns a ticket WITHOUT waiting; bgr_align_batch_wait blocks until that launch has finished and delivers its results (same
 * output contract as bgr_align_batch); bgr_align_batch_test polls (1 = finished, 0 = still running).  One batch in flight per
 * aligner: one host thread double-buffers with two aligners -- begin(A, b0); begin(B, b1); wait(A); begin(A, b2); wait(B); ... --
 * where the blocking calls need two threads.  `reads` / `read_offsets` (page-locked memory recommended) must stay untouched until
 * the wait has returned.  The batch must fit one launch (2 * (bases + 16 * reads) < 2^32 - 2^28): larger ones go through
 * bgr_align_batch, which cuts them. */
typedef struct {
    bgr_aligner* aligner;
    uint64_t n_reads;
    uint64_t serial;      /* which begin of that aligner this ticket belongs to */
} bgr_ticket;
int bgr_align_batch_begin(bgr_aligner* a, const bgr_params* p, const char* reads, const uint64_t* read_offsets, uint64_t n_reads, bgr_ticket* ticket);
int bgr_align_batch_test(const bgr_ticket* ticket);
int bgr_align_batch_wait(const bgr_ticket* ticket, int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status);

/* Text form: one piece of a FASTA file in, the bytes to append to `paths` / `notAligned.fa` out -- the whole per-batch body of
 * Aligner::alignPartGreedy (alignerGreedy.cpp:367-431: getReads, alignReadGreedy per read, the fwrite of a record) on the device,
 * so a batch crosses PCIe as the file's own bytes (text_kernels.hip).  The piece must start at a header line and end behind the
 * newline of a sequence line (or at the end of the file).  The device takes the shape nearly every piece has (header line, ONE
 * sequence line, next header ...); for any other piece (multi-line sequences, blank lines, a last record without its newline;
 * records of fewer than 32 bytes on average over 32 KB of the piece -- reads of two dozen bases: more than the device's tables hold)
 * the call returns BGR_OK with `irregular` = 1 and NOTHING mapped: the caller then parses that piece on the host (the exact
 * getReads state machine) and uses bgr_align_batch*, so the records are the reference's either way.
 * BGR_E_CAPACITY: an output buffer is too small; paths_bytes / notaligned_bytes say what is needed, the mapping is done, and
 * bgr_aligner_fetch_text delivers the same bytes into larger buffers.  Blocking; page-locked buffers recommended. */
typedef struct bgr_text_stage bgr_text_stage;
typedef struct {
    uint64_t struct_size;         /* in: sizeof(bgr_text_batch) of the header the caller was built with.  The struct has grown over the rounds and will again: a
                                     caller built against another layout is refused (BGR_E_ARG) instead of having fields read past the end of its struct.
                                     Zero the whole struct, then set this first. */
    const char* text;             /* in: the piece (may be NULL when `stage` holds it) */
    uint64_t text_bytes;          /*     < 2^31 */
    uint32_t want_output;         /*     0 = map and count only (-b without --write-exhaustive writes nothing), 1 = the reference's records,
                                         2 = correction mode (-c, alignerGreedy.cpp:394-404): a mapped read's record is header + the read as
                                         spelled by its path (recoverPath, aligner.cpp:270-290); greedy modes, ACGT-only unitigs,
                                         3 = GAF (--gaf): a mapped read's record is one GAF line (below, bgr_run_options.gaf); greedy modes,
                                         ACGT-only unitigs; capacities, BGR_E_CAPACITY and bgr_aligner_fetch_text as with 2 */
    uint32_t irregular;           /* out: 1 = piece left to the host parser; 2 = (want_output 2, 3) a path of this piece does not spell a walk --
                                         the reference's "bug compaction" exit, which the caller reproduces on the host */
    char* paths_out;              /* in: where the records of mapped reads go */
    uint64_t paths_cap;
    char* notaligned_out;         /*     and those of the others (never more than text_bytes) */
    uint64_t notaligned_cap;
    uint64_t n_records, n_accepted, paths_bytes, notaligned_bytes;   /* out */
    bgr_text_stage* stage;        /* in, optional: the piece was sent ahead with bgr_text_stage_upload (same bytes, same device): the call
                                     waits for that copy on the device instead of making its own */
    uint32_t fastq;               /* in: 1 = the piece is FASTQ (-q): whole four-line records (record j = lines 4j .. 4j+3 whatever they hold,
                                     aligner.cpp:51-68), ending with a newline; the reference's end-of-file behaviour (its phantom record)
                                     stays with the caller: bgr_align_all maps the file's last getReads() call through the host parser.
                                     2 = the same records with their '+' and quality lines left out by the caller: record j = lines 2j, 2j+1
                                     (header line, read line) -- half the bytes over PCIe, the same records out */
    uint32_t reserved;
    uint32_t* record_info_out;    /* in, optional: one word per RECORD of the piece, in the piece's order -- bit 31: getReads keeps it, bit 30: it was mapped,
                                     bits 0..29: its read's length (0 unless kept) -- what the reference's -b progress blocks count between two getReads()
                                     calls (alignerExhaustive.cpp:306-316: a record, kept or dropped, is one iteration of the call).  Needs room for
                                     text_bytes / 24 + 1024 words (record_info_cap); n_records of them are written.  Not with want_output = 2 or 3. */
    uint64_t record_info_cap;
} bgr_text_batch;
/* A stage = a device buffer for one piece + a copy stream: bgr_text_stage_upload starts the host -> device copy and returns; the
 * bgr_align_fasta_text call that names the stage orders itself behind it (hipStreamWaitEvent), so the copy of the next piece runs
 * under the kernels of this one.  The host bytes must stay untouched until that call has returned, and the stage keeps the piece
 * (no new upload, no destroy) until the records have been fetched: after BGR_E_CAPACITY, bgr_aligner_fetch_text still cuts them from it. */
int bgr_text_stage_create(int device, bgr_text_stage** out);
void bgr_text_stage_destroy(bgr_text_stage* s);
int bgr_text_stage_upload(bgr_text_stage* s, const char* text, uint64_t text_bytes);
/* ... a piece that lies in several host ranges (the header and read lines gathered out of a FASTQ file part by part): the device receives
 * them back to back, in order; the piece's size is the sum. */
int bgr_text_stage_upload_parts(bgr_text_stage* s, uint32_t n_parts, const char* const* parts, const uint64_t* part_bytes);
int bgr_text_stage_device(const bgr_text_stage* s);  /* the device the stage was created on (-1: null) */
int bgr_align_fasta_text(bgr_aligner* a, const bgr_params* p, bgr_text_batch* b);
int bgr_aligner_fetch_text(bgr_aligner* a, bgr_text_batch* b);

/* Device-resident form: inputs already in this device's HBM (d_reads bytes, d_read_offsets uint64[n+1]);
 * results stay in aligner-owned device buffers (bgr_aligner_device_results).  Asynchronous on the
 * aligner's stream; max_read_len = longest read in the batch (< 2^24), total_bases = read_offsets[n].
 * Read characters must be from ACGTN (what getReads lets through).
 * Consecutive launches with no wait between them (bgr_aligner_sync, a fetch, counters ...) may run CONCURRENTLY and complete in either order: in
 * greedy and anchors mode a launch that finds the aligner's stream busy goes to a second stream with a second set of launch buffers (created on
 * first use), and further un-waited launches take turns between the two, each in order behind the launch that used its buffers before (at most
 * two in flight side by side; bgreat_amd/csrc/launch_taker.h has the rule).  A launch that finds the aligner idle always uses the aligner's own
 * stream and buffers, so a caller that waits between its launches sees no difference.  The input buffers of every launch in flight must stay
 * untouched until it is waited for.  An aligner used this way holds two sets of launch buffers: 4 bytes per arena int (bgr_plan_launch:
 * arena_ints, about 2 x (bases + 8 x reads) plus 16 ints per read), per read 8 bytes of results and 4 of the list for the second pass, plus the
 * follow-up rings -- at 5 M x 150 bp 1 661 966 080 arena ints = 6.65 GB, 6.71 GB in all, an eighth more as allocated.  Most of an arena is never
 * touched (a path has far fewer ints than its read has bases).  BGR_KNOB_DEVICE_OVERLAP 1 turns it off.
 * Exhaustive launches always stay on the aligner's own stream.  The counting features (abundance, links, triples, pileup) count every launch
 * once, whichever stream ran it. */
int bgr_align_device(bgr_aligner* a, const bgr_params* p, const void* d_reads, const void* d_read_offsets, uint64_t n_reads,
                     uint64_t total_bases, uint32_t max_read_len);
/* Waits for the aligner's stream, and for its second one when un-waited bgr_align_device launches went there: every launch has completed when it
 * returns.  In exhaustive mode it also SETTLES the launch: reads whose search outgrew the last pass's table of remembered calls
 * are mapped again with a larger one (BGR_KNOB_EXH_MEMO_CAP) before the results count as final -- every fetch / counters call does the same; a caller
 * that reads the device results below by itself calls this first. */
int bgr_aligner_sync(bgr_aligner* a);
/* Device pointers of the last bgr_align_device results: results uint32[n][2] = {path offset in the arena,
 * path length | status << 24}, arena int32[], cursor u32[2]: [0] = path ints handed out from the part of the arena behind the rows
 * the launch's several-reads-per-wave first pass owns by read or wave number (so not all the ints in use), [1] = 1 if the arena overflowed.
 * Row i of the result = arena[results[i][0] .. + (results[i][1] & 0xFFFFFF)].
 * The pointers are those of the LAST launch: behind un-waited consecutive launches (see bgr_align_device) they may differ from those of the launch
 * before, whose results lie in the other set of buffers until the next launch but one.  Like this call, bgr_aligner_fetch, bgr_aligner_path_stats,
 * bgr_aligner_arena_ints, bgr_aligner_pass_counts, bgr_aligner_launch_info and bgr_aligner_last_pass_runs describe the last launch.
 * A caller may write rows of its own there.  One rule for every reader: a row with results[i][0] + (results[i][1] & 0xFFFFFF) > the arena ints
 * of the launch (bgr_aligner_arena_ints; the sum taken in 64 bits) reads as an EMPTY row.  The counting kernels (abundance, links, triples,
 * pileup, haplotags) skip it -- the pileup does not count it as skipped --, bgr_aligner_path_stats reports zeros as for an unmapped read, and
 * bgr_aligner_fetch delivers an empty path with the status byte as stored. */
int bgr_aligner_device_results(bgr_aligner* a, void** d_results, void** d_arena, void** d_cursor);
/* Ints of that arena as the last launch planned it (0 before any launch): a row lies in the arena when results[i][0] + its ints is at most this,
 * and the counting kernels skip a row that does not. */
int bgr_aligner_arena_ints(bgr_aligner* a, uint64_t* ints);
/* What bgr_run_options.gaf writes per read, for a caller that keeps its own reads: over the results of the last bgr_align_device launch of this
 * aligner (greedy or anchors mode; the caller hands the same device reads again, the aligner keeps nothing alive), out[i] for read i: the size of the
 * walk its path spells, where the read starts on the path as GAF counts it (from the other end for a read mapped on its reverse complement), the
 * characters covered and how many of them differ from the read.  Zeros for an unmapped read; mismatches = BGR_PATH_STAT_NO_WALK for a path that
 * spells no walk (no error: the caller decides).  Blocking: one kernel on the aligner's stream and one copy.  BGR_E_ARG on a graph with non-ACGT
 * unitig characters, after an exhaustive launch, or when n_reads is not the launch's. */
typedef struct {
    uint64_t path_len, path_start;
    uint32_t aligned, mismatches;
} bgr_path_stat;
#define BGR_PATH_STAT_NO_WALK 0x80000000u
int bgr_aligner_path_stats(bgr_aligner* a, const void* d_reads, const void* d_read_offsets, uint64_t n_reads, bgr_path_stat* out);
/* WHICH characters differ, where bgr_path_stat says how many: the differences of read i at out[diff_offsets[i] .. diff_offsets[i + 1]), ascending
 * read_pos (a position of the read as the caller holds it), path_base = what the path spells there in the read's direction (for a read mapped on its
 * reverse complement: the complement), read_base = the read's character.  These are the "*" ops of the cs:Z: field below, as structs.  Nothing for an
 * unmapped read, for a row that does not lie wholly inside the arena and for a path that spells no walk -- so a read has as many entries as
 * bgr_path_stat.mismatches says, 0 where that is BGR_PATH_STAT_NO_WALK.  Three launches on the aligner's stream: count, a scan, fill; blocking.
 * diff_offsets has n_reads + 1 entries; *n = the differences of the launch.  BGR_E_CAPACITY, with *n and the offsets set and `out` untouched, when
 * cap < *n: call again with room.  The refusals are bgr_aligner_path_stats's, and BGR_E_ARG for a launch of 2^32 bases or more. */
typedef struct {
    uint32_t read_pos;
    uint8_t path_base;   /* 0..3 = ACGT, in the read's direction */
    uint8_t read_base;   /* 0..3 = ACGT, 4 = a character outside ACGT */
    uint16_t reserved;   /* 0 */
} bgr_path_diff;
int bgr_aligner_path_diffs(bgr_aligner* a, const void* d_reads, const void* d_read_offsets, uint64_t n_reads, uint64_t* diff_offsets, bgr_path_diff* out, uint64_t cap,
                           uint64_t* n);
/* The cs:Z: field of GAF lines (--cs): "\tcs:Z:<ops>" as the LAST field of every line, behind NM:i: and behind the haplotag fields of a line that has
 * them.  The ops are minimap2's short form with substitutions only (a path and its read have no gaps between them): over the aligned characters in
 * the read's direction, ":<n>" per maximal run of n equal characters and "*<path base><read base>" in lower case per difference, "n" for a read
 * character outside ACGT; no aligned character: the empty value.  So the number of "*" is NM, and the run lengths plus NM are column 11.
 * bgr_aligner_gaf_cs_enable(a, on): the GAF lines of bgr_align_fasta_text (want_output = 3) of this aligner end in the field; the sizes and write
 * kernels then launched are instances of their own (bgreat_amd/csrc/gaf_cs_device.h), an aligner with the switch off launches the kernels it always did
 * and writes the bytes it always did.  bgr_graph_gaf_cs_enable(g, on) is sticky, for whole runs: every later bgr_align_all with bgr_run_options.gaf
 * writes the field, on every route (the host formatter writes the same bytes); BGR_E_ARG from a bgr_align_all with the switch on and gaf off. */
int bgr_aligner_gaf_cs_enable(bgr_aligner* a, int on);
int bgr_graph_gaf_cs_enable(bgr_graph* g, int on);
int bgr_graph_gaf_cs_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
/* The paths of exhaustive launches as output (--exhaustive-paths).  Off by default: an aligner with the switch off refuses what it always refused
 * and launches the kernels it always did.
 * A row of exhaustive mode is [begin offset, +-u_1 .. +-u_n, end offset] (alignerExhaustive.cpp:96-104, 193-201, 249-257): a row of the greedy modes
 * with one more int behind it, |readLeft| + k - 1 in the last unitig or 0 when the read ends with the anchor.  With L the read's length and
 * e = row[0] + L - (the walk's length - the last unitig's length), that int is e -- or, only where e is the last unitig's length, 0: the same position,
 * the read's last character on the unitig's last, spelled two ways.  Dropping it loses no position.
 * The VIEW of an exhaustive launch is a second array of result words.  For the pair {off, w} of a read, n = w & 0xFFFFFF and st = w >> 24, its entry is
 * {off, (n - 1) | st << 24} when (st & BGR_ST_MASK) == BGR_ST_ALIGNED, n >= 3 and off + n <= the launch's arena ints (the sum in 64 bits), else
 * {off, st << 24}: an empty row with the status as stored -- the rule every reader applies to a row outside the arena.  The rows themselves and
 * the arena are untouched: bgr_aligner_fetch and bgr_aligner_device_results deliver the reference's rows with the end offset, as ever.
 * (tests/exhaustive_rows_ref.py is the rule in plain Python; the kernel, "bgr_exhaustive_rows_kernel" in bgr_aligner_kernel_times, is
 * bgreat_amd/csrc/exhaustive_rows_kernels.hip.)
 * bgr_aligner_exhaustive_paths_enable(a, on), refused on an internal twin.  While on:
 *  - an exhaustive launch of an aligner that counts abundance, links, triples or a pileup (with or without strands) is accepted, and counted through
 *    its view.  The inside pass is still refused.  An exhaustive launch is final only once it is SETTLED (bgr_aligner_sync above), so its view and
 *    counting kernels are queued behind that, exactly once per launch, by whichever comes first: a call that reads a counting table, a fetch, sync,
 *    counters or kernel-times call, or the next launch on the same aligner.  The read buffers of the launch must stay untouched until then -- longer
 *    than the rule for un-waited launches at bgr_align_device asks, which ends at the wait;
 *  - bgr_aligner_path_stats, bgr_aligner_path_diffs and bgr_aligner_haplotags accept an exhaustive last launch: they settle it and read its view
 *    (mismatches may exceed max_mismatch for a read that holds a character outside ACGT: exhaustive mode counts those as the reference does);
 *  - bgr_align_fasta_text accepts want_output = 3 in exhaustive mode -- its GAF kernels read the view, cs:Z: and haplotags included -- and
 *    record_info_out together with it; a call on a counting aligner returns once the counting kernels have run.
 * bgr_aligner_device_rows_view: the view of the last launch in the aligner's HBM, uint32[n][2], made and waited for (the launch is settled first);
 * valid until the next launch.  BGR_E_ARG when the last launch was not exhaustive or the switch is off.
 * bgr_graph_exhaustive_paths_enable(g, on) is sticky, for whole runs: a later bgr_align_all in exhaustive mode accepts gaf and every counting
 * output.  BGR_E_ARG from such a run that is not exhaustive, has partial (-i) set -- a row may then lack the end offset -- or has the graph's inside
 * switch on.  Correction (-c) stays ignored and k > 32 stays refused in exhaustive mode. */
int bgr_aligner_exhaustive_paths_enable(bgr_aligner* a, int on);
int bgr_aligner_device_rows_view(bgr_aligner* a, void** d_view);
int bgr_graph_exhaustive_paths_enable(bgr_graph* g, int on);
int bgr_graph_exhaustive_paths_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
/* Copy the last device results to the host in input order (same output contract as bgr_align_batch). */
int bgr_aligner_fetch(bgr_aligner* a, uint64_t n_reads, int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status);

/* Reads that lie inside one unitig (--inside).  Greedy mode anchors a read on overlap (k-1)-mers, which sit at unitig ends: a read that lies wholly
 * inside one unitig has none, gets BGR_ST_NOANCHOR and reaches no output.  The inside pass maps these reads in a pass of its own behind the mapping
 * passes.  The definition (tests/inside_ref.py restates it in plain Python):
 *   k-mer word: the 2k-bit word of the graph's 2-bit code, first base most significant, k <= 32; canonical = the smaller of the word and the word of
 *   its reverse complement; a k-mer equal to its own reverse complement is never indexed; a k-mer is SELECTED when the jump index's rule holds for the hash of
 *   its canonical form (bgr_jump_selects over bgr_mix64, bgreat_amd/csrc/graph_layout.h: one in four, a function of the k-mer alone).
 *   The inside index holds, for every unitig id and offset 0 <= j <= len - k whose k-mer is selected, canonical -> (id, j, whether the forward window
 *   is the canonical one); of a k-mer that occurs more than once the smallest (id, j).  It is exact: membership is decided by comparing the key.
 *   The pass, over a read R of L >= k characters whose status & BGR_ST_MASK is BGR_ST_NOANCHOR, for i = 0 .. L - k in order: the window R[i, i + k) is
 *   skipped if it holds a character outside ACGT, is not selected or is not in the index; else with its entry (id, j): if the window equals the
 *   unitig's at j the read lies forward on it from s = j - i, else on its reverse complement from s = (len - k - j) - i, counted there.  The candidate
 *   is valid when 0 <= s, s + L <= len and R differs from the oriented unitig's [s, s + L) in at most max_mismatch characters (a read character
 *   outside ACGT always differs).  The FIRST valid candidate decides: the row becomes [s, +id] or [s, -id] (two ints; the sign is the strand) and the
 *   status BGR_ST_ALIGNED without BGR_ST_RC.  No valid candidate: nothing about the read changes.  effort does not enter.  Reads shorter than k,
 *   BGR_ST_FAILED reads and reads that hang over a unitig's end stay as they are.  The result is a function of the read, the graph and max_mismatch
 *   alone, whatever the batching, route, stream or device.
 * bgr_graph_inside_build builds the index on the host (bgr_set_build_threads threads) from the graph's host blob; sticky, a second call does nothing.
 * BGR_E_ARG for k > 32, a graph with non-ACGT unitig characters and one without a host blob; BGR_E_NOMEM, with nothing left allocated, when the table
 * cannot be had.  The table -- open addressing, load at most 0.5, 16-byte entries: 32 bytes per selected k-mer, at most 8 bytes per graph base -- is NOT part of bgr_graph_blob's bytes: it
 * lives in a buffer of its own and is copied once to each device on which an aligner enables the pass.  bgr_graph_inside_info: its numbers (zeroes
 * before a build).  bgr_graph_inside_lookup (diagnostic, the CPU tests pin the table with it): the entry of a k-mer word given on either strand.
 * bgr_aligner_inside_enable(a, on): while on, every greedy / anchors launch of the aligner, through every entry point, is followed on its stream -- in
 * front of the counting kernels, the text formatter and everything else that reads rows -- by one kernel ("bgr_align_inside_kernel" in
 * bgr_aligner_kernel_times); the launch's arena is planned with 2 more ints per read.  BGR_E_ARG when the graph has no index; an exhaustive launch
 * of an enabled aligner, and one with a read beyond 32 000 characters, is refused with BGR_E_ARG.  bgr_aligner_inside_count: reads the pass has
 * mapped since the aligner was made or bgr_aligner_reset_counters; the five counters of bgr_aligner_counters keep their meaning -- no_overlap counts
 * the reads without an anchor, those mapped inside included.
 * bgr_graph_inside_enable(g, on) is sticky, for whole runs: every aligner of a later bgr_align_all runs the pass (both routes, every device, split
 * output); BGR_E_ARG from a run in exhaustive mode.  bgr_graph_inside_count: what the last such run mapped inside. */
typedef struct {
    uint64_t entries, slots, bytes;   /* distinct k-mers held, slots of the table, its bytes (16 per slot) */
    double build_seconds;
} bgr_inside_info;
int bgr_graph_inside_build(bgr_graph* g);
int bgr_graph_inside_info(const bgr_graph* g, bgr_inside_info* out);
int bgr_graph_inside_lookup(const bgr_graph* g, uint64_t kmer, uint32_t* unitig, uint32_t* offset, uint32_t* forward_canonical, uint32_t* found);
int bgr_aligner_inside_enable(bgr_aligner* a, int on);
int bgr_aligner_inside_count(bgr_aligner* a, uint64_t* n);
int bgr_graph_inside_enable(bgr_graph* g, int on);
int bgr_graph_inside_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_inside_count(const bgr_graph* g, uint64_t* n);

/* Per-unitig abundance, counted on the device behind every mapping launch (the definition: bgr_run_options.abundance below).  Off unless enabled;
 * while enabled every greedy / anchors launch of the aligner -- through bgr_align_device, bgr_align_batch and its split and overlapped forms, the
 * packed form, begin / wait, the text form -- is followed on its stream by one kernel ("bgr_abundance_kernel" in bgr_aligner_kernel_times) that adds
 * the launch's rows to a table in the aligner: exact 64-bit sums, whatever the batching.  An exhaustive launch on an enabled aligner is refused
 * (BGR_E_ARG: its rows end in an end offset, alignerExhaustive.cpp:96-104, 249-257).  Fetching the same results again (after BGR_E_CAPACITY)
 * counts nothing.  enable allocates and zeroes the table the first time; disabling keeps it.  bgr_aligner_abundance synchronises and delivers the
 * table (n_rows must be the graph's n_unitigs; row i = unitig id i + 1), with what the other streams of overlapped batches counted added in.
 * The kernel is queued with the launch: a launch that fails afterwards (BGR_E_INTERNAL, BGR_E_HIP) may have added part of its rows, and the table is
 * undefined until bgr_aligner_reset_abundance.
 * bgr_aligner_abundance_plan: the kernel a launch of n_reads reads and total_bases bases on this aligner is followed by, with its knob as it stands --
 * out = {form (1 = A, 2 = B), workgroups, threads per workgroup, bytes of LDS per workgroup}.  bgr_plan_abundance is the same choice from plain
 * numbers, without a device (num_cus / lds_per_cu 0 = the MI355X's); form B needs 12 x (n_unitigs + 1) bytes of LDS and k x total_bases < 2^32
 * (no 32-bit counter of the launch can wrap then), and a launch that misses either takes form A whatever BGR_KNOB_ABUNDANCE_FORM says. */
typedef struct { uint64_t reads, bases, kmers; } bgr_unitig_abundance;
int bgr_aligner_abundance_enable(bgr_aligner* a, uint32_t on);
int bgr_aligner_abundance(bgr_aligner* a, bgr_unitig_abundance* out, uint64_t n_rows);
int bgr_aligner_reset_abundance(bgr_aligner* a);
int bgr_aligner_abundance_plan(bgr_aligner* a, uint64_t n_reads, uint64_t total_bases, uint32_t out[4]);
int bgr_plan_abundance(uint64_t n_unitigs, uint32_t k, uint64_t n_reads, uint64_t total_bases, uint32_t num_cus, uint64_t lds_per_cu, uint32_t form_knob, uint32_t out[4]);

/* Links: which unitigs the mapped reads join, and how often.  A mapped read's row in the greedy modes is [off, id_1 .. id_n] with signed 1-based ids;
 * every consecutive pair (a, b) = (id_j, id_j+1), j = 1 .. n-1, is one traversal of a link.  (a, b) and (-b, -a) are the same link -- the same
 * junction read from the other strand: with key(x, y) = the tuple (|x|, x < 0, |y|, y < 0), the canonical form is whichever of (a, b) and (-b, -a)
 * has the smaller key, compared lexicographically ((a, -a) is its own mate), and count[canonical link] += 1 per traversal.  Neither the read's strand
 * (BGR_ST_RC) nor off enters; unmapped reads and one-unitig paths add nothing; ids that are 0 or beyond n_unitigs are skipped, as the abundance kernel
 * skips them.  The counts are exact 64-bit integers and do not depend on batching, routes, streams or devices.
 * Counted on the device as unitig abundance is: off unless enabled; while enabled every greedy / anchors launch of the aligner, through every entry
 * point, is followed on its stream by one kernel ("bgr_links_kernel" in bgr_aligner_kernel_times while a slot is free) that adds the launch's pairs to
 * an open-addressed hash table {u64 key, u64 count} in device memory.  The table is sized when counting is first enabled, from the graph (one with a
 * host blob): bgr_graph_links_bound counts, over the unitig ends and the slots of the half record each end's walk reads, how many distinct links any
 * rows on this graph can hold (bgreat_amd/csrc/links_kernels.h has the argument), and the capacity is the power of two that is at least twice that,
 * 16 bytes per slot -- so the table cannot fill.  Should an insert find no place all the same, it is counted in an overflow word, and
 * bgr_aligner_links / the run return BGR_E_CAPACITY with a message until bgr_aligner_reset_links.  The internal streams of overlapped batches add to
 * the same table.  An exhaustive launch on an enabled aligner is refused (BGR_E_ARG) and adds nothing; launches of an aligner that is not counting
 * add nothing; disabling keeps the table; a launch that fails afterwards may have added part of its rows.
 * bgr_aligner_links synchronises and delivers the canonical links with a count, sorted by key; *n = their number, BGR_E_CAPACITY (with *n set) when
 * cap is smaller -- the kernel counts the slots it claims, so the call that only asks for the number (cap 0) moves three words, not the table.
 * A delivery copies the whole table to the host (16 bytes per slot: 512 MiB on a chr1-scale graph) and picks and sorts the used slots on the calling
 * thread: a call per run or per batch of launches, not per launch.
 * bgr_aligner_links_info (diagnostic: tests and tools/links_rate.py read it): out = {slots of the table, the graph's bound, traversals that found no place, workgroups of form B whose
 * LDS table handed at least one traversal straight to the table in device memory}.
 * bgr_aligner_links_plan: the kernel behind a launch of n_reads reads on this aligner, with its knob as it stands -- out = {form (1 = A, 2 = B),
 * workgroups, threads per workgroup, bytes of LDS per workgroup}; bgr_plan_links is the same choice from plain numbers, without a device
 * (num_cus 0 = the MI355X's): form B by default exactly where links_bound is at most half of its LDS table's 2048 slots. */
typedef struct { int32_t from, to; uint64_t count; } bgr_link;
int bgr_aligner_links_enable(bgr_aligner* a, uint32_t on);
int bgr_aligner_links(bgr_aligner* a, bgr_link* out, uint64_t cap, uint64_t* n);
int bgr_aligner_reset_links(bgr_aligner* a);
int bgr_aligner_links_info(bgr_aligner* a, uint64_t out[4]);
int bgr_aligner_links_plan(bgr_aligner* a, uint64_t n_reads, uint32_t out[4]);
int bgr_plan_links(uint64_t links_bound, uint64_t n_reads, uint32_t num_cus, uint32_t form_knob, uint32_t out[4]);
int bgr_graph_links_bound(bgr_graph* g, uint64_t* bound);
/* Pileup: per base of every unitig, how many mapped reads cover it and how many of them differ from it, by read character.  Take a mapped row
 * (status, path = [off, id_1 .. id_n]) of a read R of L characters in the greedy modes; the path spells a walk in which unitig occurrence j is glued on
 * in its forward strand or its reverse complement (recoverPath / compactionEnd: the strand its sign names, or failing that the other) and has the
 * extent [s_j, e_j): s_1 = 0, e_j = s_j + len_j, s_(j+1) = e_j - (k-1) -- the k-1 characters two neighbours share belong to BOTH.  With
 * cl = min(L, walk size - off) and Q = R, or its reverse complement when status has BGR_ST_RC: for every i in [0, cl) and every occurrence j whose
 * extent holds p = off + i, x = p - s_j, pos = x on a forward occurrence and len - 1 - x on a reversed one, c = Q[i] resp. its complement (any character
 * outside ACGT is N, and stays N): depth[unitig][pos] += 1 and, if c is not the unitig's character there, the count of c at [unitig][pos] += 1.
 * Positions are 0-based on the strand the unitig file spells; a, c, g, t count only reads that DIFFER from the unitig's base (the word of the base's
 * own letter is always 0).  Unmapped reads add nothing; a path that spells no walk (bgr_path_stat's BGR_PATH_STAT_NO_WALK condition) adds nothing and is
 * counted in *skipped.  For every unitig the sum of its depths equals its `bases` of bgr_unitig_abundance.  Rows are flat in unitig order: base pos of
 * unitig i (1-based) has index sum(len_j, j < i) + pos; n_bases must be the sum of the unitig lengths (bgr_graph_info's total_bases / 2).
 * Counted on the device as unitig abundance is: off unless enabled; while enabled every greedy / anchors launch of the aligner, through every entry
 * point, is followed on its stream by one kernel ("bgr_pileup_kernel" in bgr_aligner_kernel_times while a slot is free) that walks each path with
 * sixteen lanes, adds +1 / -1 at the two ends of each occurrence's covered stretch to a difference array (the depth is its running sum, taken mod 2^32
 * when the table is read) and one 32-bit atomic per differing character.  The internal streams of overlapped batches add to the same table.  The table
 * takes 20 bytes per base of the graph and 4 per unitig in device memory, per aligner, allocated (with the buffers' usual slack of one eighth) when
 * counting is first enabled: 164 MiB on bench.py's default graph (8 587 555 bases in 98 866 unitigs), 7.3 GiB on the chr1-scale graph (389 965 388
 * bases in 3 966 085 unitigs); BGR_E_NOMEM, with nothing allocated, when the device does not have it.  A character outside ACGTN is an N where the kernel reads the read's
 * characters (bgr_align_batch, bgr_align_device and the text form in greedy mode); where it reads the 2-bit planes (bgr_align_batch_packed, and launches
 * that pack the reads in a pre-pass: anchors mode, BGR_KNOB_GREEDY_PREPASS) it sees what the packing made of it -- its str2num code, as the mapping
 * kernels do -- so such a character counts like the letter it packs to there.  The file parsers admit only ACGTN, so whole runs never meet one.
 * Enabling the pileup also enables unitig
 * abundance (as links do): its `reads` column is an exact upper bound on every depth on the unitig, and when any unitig's reads reach 2^32
 * bgr_aligner_pileup and the run return BGR_E_CAPACITY with a message instead of wrapped numbers.  Refused with BGR_E_ARG: an exhaustive launch on an
 * enabled aligner, and enabling on a graph with non-ACGT unitig characters (as GAF output) or without a host blob.  Disabling keeps the table; a launch
 * that fails afterwards may have added part of its rows, and the table is undefined until bgr_aligner_reset_pileup (which leaves the abundance table
 * alone).  bgr_aligner_pileup synchronises, copies the table to the host (20 bytes per base) and converts it on the calling thread: a call per run or
 * per batch of launches, not per launch. */
typedef struct { uint32_t depth, a, c, g, t, n; } bgr_pileup_base;
int bgr_aligner_pileup_enable(bgr_aligner* a, uint32_t on);
int bgr_aligner_pileup(bgr_aligner* a, bgr_pileup_base* out, uint64_t n_bases, uint64_t* skipped);
int bgr_aligner_reset_pileup(bgr_aligner* a);
/* SNV sites on the unitigs, called from the pileup table on the device.  For thresholds min_depth >= 1, min_alt >= 1 and min_af_ppm in 0 .. 1 000 000
 * a base (unitig, pos) is a SITE when its depth >= min_depth and at least one allele passes; allele X of A C G T, other than the unitig's own letter,
 * PASSES when its count c_X >= min_alt and c_X * 1 000 000 >= min_af_ppm * depth (64-bit integers: no floating point anywhere).  N is never an allele.
 * A site's record holds the numbers of bgr_pileup_base at that base, unitig the 1-based ordinal, pos 0-based; sites come in (unitig, pos) order.
 * bgr_aligner_pileup_sites calls the sites of this aligner's table where it lies: it synchronises (the aligner's stream and its internal ones), applies
 * the guard of bgr_aligner_pileup (BGR_E_CAPACITY when a unitig's reads reach 2^32), runs five launches on the aligner's stream -- per-tile sums of the
 * difference array, their scan, a classify pass that counts each tile's sites, the scan of the counts, and the same pass again writing every record at
 * its final place (tiles of BGR_VARIANTS_TILE words of the difference array; no sort, no atomics on the output, no workgroup waits for another) -- and
 * copies only the records: *n = their number, always; BGR_E_CAPACITY, with *n set and nothing copied, when cap is smaller.  The table itself never
 * leaves the device.  BGR_E_ARG: the pileup was never enabled on the aligner, or thresholds out of range.  bgr_aligner_pileup_sites_times: the
 * milliseconds of the last call's five launches (zeroes when none ran).
 * bgr_aligner_pileup_add adds src's pileup table into dst's (both enabled, same graph, neither an internal stream; mod 2^32, the skipped counter too;
 * the abundance tables are not touched -- a caller that relies on dst's guard adds those itself): one kernel when both are on one device, else in
 * pieces through a staging buffer on dst's device of at most 64 MiB (peer copy, then the kernel). */
#define BGR_VARIANTS_TILE 2048u
typedef struct { uint32_t unitig, pos, depth, a, c, g, t, n; } bgr_variant_site;
typedef struct { uint32_t min_depth, min_alt, min_af_ppm; } bgr_variant_params;
int bgr_aligner_pileup_sites(bgr_aligner* a, const bgr_variant_params* params, bgr_variant_site* out, uint64_t cap, uint64_t* n);
int bgr_aligner_pileup_sites_times(bgr_aligner* a, double ms[5]);
int bgr_aligner_pileup_add(bgr_aligner* dst, bgr_aligner* src);
/* Strands.  Occurrence j of a mapped read is a FORWARD OBSERVATION when the read as given in the input is collinear with the strand the unitig file
 * spells: the row's status has no BGR_ST_RC and the occurrence is glued on forward, or it has BGR_ST_RC and the occurrence is glued on reversed.  The
 * FORWARD PILEUP is bgr_pileup_base over the forward observations only -- same positions, same complementing, same N rule; the reverse part is the
 * total minus it, element by element, so 0 <= forward <= total everywhere, and for every unitig the forward depths sum to the bases its forward
 * occurrences cover.  Rows that spell no walk add to neither table: skipped is the total table's alone.
 * bgr_aligner_pileup_strands_enable(a, 1) enables the pileup as well (as the pileup enables abundance) and allocates a second table of the pileup's
 * layout, 20 more bytes per base: 328 MiB per aligner in total on bench.py's default graph, 14.6 GiB on the chr1-scale graph; BGR_E_NOMEM with nothing
 * allocated when the device does not have it.  While it is on, the pileup kernel of every launch is the instance that repeats the two delta atomics
 * and each alt atomic of a forward observation into that table ("bgr_pileup_kernel" in the times as before); the internal streams share it.
 * Switching off keeps the table (and leaves the pileup on); bgr_aligner_reset_pileup clears both tables; bgr_aligner_pileup_add adds the forward
 * tables too when both aligners have one (BGR_E_ARG when exactly one has); the 2^32 guard is the total table's, unchanged, and bgr_aligner_pileup /
 * bgr_aligner_pileup_sites deliver what they deliver without the switch.  bgr_aligner_pileup_forward: the forward table as bgr_aligner_pileup
 * delivers the total (BGR_E_ARG when strands were never enabled).
 * bgr_aligner_pileup_strand_sites: bgr_aligner_pileup_sites with the STRAND FILTER on top -- for min_alt_strand >= 0 allele X passes when it passes
 * the test above and forward.X >= min_alt_strand and total.X - forward.X >= min_alt_strand (0: exactly the sites of bgr_aligner_pileup_sites).
 * Still five launches: the tile sums and the scan take both difference arrays, the two classify passes rescan both and read the forward alt words of
 * a base that has a candidate allele.  A record is 64 bytes: the numbers of bgr_variant_site, then fdepth, fa .. fn of the forward table, then two
 * zero words.  Capacity protocol, guard and refusals as bgr_aligner_pileup_sites (BGR_E_ARG when strands were never enabled);
 * bgr_aligner_pileup_sites_times reads its launches too. */
typedef struct { uint32_t min_depth, min_alt, min_af_ppm, min_alt_strand; } bgr_variant_strand_params;
typedef struct { uint32_t unitig, pos, depth, a, c, g, t, n, fdepth, fa, fc, fg, ft, fn, reserved[2]; } bgr_variant_strand_site;   /* 64 bytes */
int bgr_aligner_pileup_strands_enable(bgr_aligner* a, uint32_t on);
int bgr_aligner_pileup_forward(bgr_aligner* a, bgr_pileup_base* out, uint64_t n_bases);
int bgr_aligner_pileup_strand_sites(bgr_aligner* a, const bgr_variant_strand_params* params, bgr_variant_strand_site* out, uint64_t cap, uint64_t* n);
/* Diagnostic (the host tests pin the kernel's canonicalisation through it): the canonical form of the link (a, b) as the kernel computes it (the same inline code, compiled for the host): out = {from, to, 0}, and, if key is
 * not NULL, the 64-bit integer the tables hold for it -- (|from| << 33) | (from < 0) << 32 | (|to| << 1) | (to < 0), whose order is the order of the keys. */
int bgr_link_canonical(int32_t a, int32_t b, bgr_link* out, uint64_t* key);

/* aligner.h:68 counters since creation/reset: out[0]=readNumber, [1]=noOverlapRead, [2]=alignedRead,
 * [3]=notAligned, [4]=overlaps (exhaustive only).  Synchronises the stream. */
int bgr_aligner_counters(bgr_aligner* a, uint64_t out[5]);
int bgr_aligner_reset_counters(bgr_aligner* a);

/* Kernel timing by HIP events recorded on the aligner's stream around every mapping-kernel launch since the
 * last reset: number of launches and their summed duration in milliseconds.  Synchronises the stream. */
int bgr_aligner_kernel_time(bgr_aligner* a, uint64_t* launches, double* total_ms);
int bgr_aligner_reset_kernel_time(bgr_aligner* a);
/* The same per kernel of a launch, in launch order (a mapping launch is a short sequence on one stream: the pre-pass that
 * packs the reads, then the passes of the mode): summed milliseconds per position and the kernel's name (static strings;
 * NULL behind the last).  Launches of different modes since the last reset share positions. */
int bgr_aligner_kernel_times(bgr_aligner* a, uint64_t* launches, double slot_ms[8], const char* slot_names[8]);
/* Launch geometry of the last mapping kernel (for logs): blocks, threads per block, dynamic LDS bytes, and flags:
 * bit 0 = the overlap key table was staged in LDS, bit 1 = exhaustive mode ran its level search (else depth-first),
 * bit 2 = the mode ran its several-reads-per-wave first pass (sixteen in greedy mode, eight or four in the others; the numbers then
 * describe that launch). */
int bgr_aligner_launch_info(bgr_aligner* a, uint32_t out[4]);
/* How the last mapping launch went through its passes.  Greedy mode: out[0] = follow-up items (the next anchors of a read, its
 * reverse complement) the sixteen-reads-per-wave kernel queued and worked off inside its launch, out[1] = out[2] = 0,
 * out[3] = reads it left to the general kernel.  Anchors mode: out[2] = reads the several-reads-per-wave pass left to the general
 * kernel.  Exhaustive mode: out[2] = reads the four-reads-per-wave pass left to the level / depth-first search, out[0] = reads that
 * search listed for its second pass, out[1] = for its third.  Synchronises the stream. */
int bgr_aligner_pass_counts(bgr_aligner* a, uint32_t out[4]);
/* Tuning knobs (0 keeps the default): waves per workgroup, workgroups per CU, LDS staging of the overlap
 * key table (0 auto, 1 off: probed in L2, 2 on -- where it can be had: anchors mode stages nothing, a table beyond a CU's LDS is probed in L2;
 * bgr_aligner_launch_info says what the launch did). */
int bgr_aligner_configure(bgr_aligner* a, uint32_t waves_per_block, uint32_t blocks_per_cu, uint32_t lds_mphf);

/* Test / diagnostic hooks, set once per aligner (they used to be environment variables read on every launch):
 *   BGR_KNOB_EXH_FRAME_CAP     exhaustive pass 1: search frames (depth-first) or levels (level search) per wave, 0 = default;
 *                              a tiny cap pushes most reads through the later passes
 *   BGR_KNOB_EXH_SEARCH        0 = choose per graph and budget, 1 = depth-first search, 2 = level search
 *   BGR_KNOB_BATCH_SPLIT_LIMIT bgr_align_batch maps a batch in pieces beyond this many path-arena ints, 0 = default (~2^32)
 *   BGR_KNOB_DEBUG_STOP        diagnostic builds (-DBGR_PHASE_TIMING) only: 1 = stop after packing, 2 = after the position scan
 *   BGR_KNOB_GREEDY_JUMP       greedy mode: 1 = the anchor scan ignores the graph's jump index (bgr_graph_info: jump_entries), 0 = it uses it (default);
 *                              the results are the same either way */
#define BGR_KNOB_EXH_FRAME_CAP 1u
#define BGR_KNOB_EXH_SEARCH 2u
#define BGR_KNOB_BATCH_SPLIT_LIMIT 3u
#define BGR_KNOB_DEBUG_STOP 4u
#define BGR_KNOB_BATCH_OVERLAP 8u /* bgr_align_batch of >= 512 k reads: 0 = in four pieces on two streams, copies under kernels (default), 1 = one launch */
#define BGR_KNOB_ANCHORS_FAST 7u /* anchors mode: 0 = four-reads-per-wave first pass + the one-read-per-wave kernel for the rest (default), 1 = without it */
#define BGR_KNOB_EXH_FAST 6u    /* exhaustive mode: 0 = four-reads-per-wave first pass + the level / depth-first passes for the rest (default), 1 = without it */
#define BGR_KNOB_EXH_MEMO_CAP 9u /* exhaustive mode, last pass (the reference's recursion memoised on (overlap, position): polynomial on any unitig set): entries per wave of
                                   its table of remembered calls in the FIRST run, 0 = from the read length (>= 1024).  A read whose search fills the table is run again with a table
                                   16 times as large, until it fits (bgr_aligner_last_pass_runs); tests set 8 to walk that path with small inputs */
#define BGR_KNOB_GREEDY_PREPASS 10u /* a launch handed ASCII reads, greedy / exhaustive mode: 0 = the mapping kernels stage their reads straight from the characters (default), 1 = a pre-pass writes 2-bit planes first (rounds 2-4; what anchors mode does) */
#define BGR_KNOB_KERNEL_EVENTS 11u /* 1 = a HIP event in front of a mapping launch and behind each of its kernels (default: bgr_aligner_kernel_times reports them), 0 = none (a caller that never asks for the times: bgr_align_all without its timing option) */
#define BGR_KNOB_ABUNDANCE_FORM 12u /* the abundance kernel (bgr_aligner_abundance_enable): 0 = choose per graph and batch, 1 = form A (64-bit atomics on the table in HBM), 2 = form B where its table fits and no counter can wrap
                                      (32-bit counters in each workgroup's LDS, flushed once); same table either way */
#define BGR_KNOB_LINKS_FORM 13u /* the links kernel (bgr_aligner_links_enable): 0 = choose per graph, 1 = form A (every traversal is an insert into the table in device memory), 2 = form B (a table of 2048 links per
                                  workgroup in LDS, flushed once; what finds no place in it goes the way of form A); same counts either way */
#define BGR_KNOB_GREEDY_JUMP 15u /* greedy mode, sixteen-reads-per-wave pass with the key table in LDS: 0 = the anchor scan jumps over verified unitig interiors when the graph has a jump index (bgr_graph_info: jump_entries; default), 1 = it ignores the index (same results: the index is a hint) */
#define BGR_KNOB_GREEDY_FAST 5u /* greedy mode: 0 = sixteen-reads-per-wave pass + general kernel for the rest (default), 1 = general kernel only */
#define BGR_KNOB_DEVICE_OVERLAP 14u /* consecutive bgr_align_device launches (greedy / anchors mode) that nobody waited for: 0 = they take turns on two streams with two sets of
                                       launch buffers, so that one starts on the CU slots the one before frees (default), 1 = every launch on the aligner's own stream and buffers */
int bgr_aligner_set_knob(bgr_aligner* a, uint32_t knob, uint64_t value);
/* The launch geometry by itself (bgreat_amd/csrc/launch_plan.h: a pure function of these numbers; no device, no graph object needed -- CPU tests sweep
 * it over synthetic graph headers).  Zero fields of the device part mean "an MI355X" (256 CUs, 160 KB of LDS per CU, the shipped kernels' occupancies).
 * pass[]: 0 the mode's general kernel, 1 greedy sixteen-reads-per-wave, 2 exhaustive eight-reads-per-wave, 3 anchors four-reads-per-wave,
 * 4 exhaustive depth-first over what the level search listed, 5 exhaustive last pass.  BGR_E_ARG (message: bgr_last_error) when the batch cannot
 * be mapped in one launch (a read too long for the LDS layouts, a batch beyond the 32-bit path arena). */
typedef struct bgr_plan_input {
    uint32_t k, slot_fill_x100, table_bytes, has_exceptions, anchors, anchor_levels;   /* graph header */
    uint64_t graph_bases, n_unitigs, max_unitig_len;
    uint32_t num_cus, resident_waves[7];                                                /* device (0: MI355X defaults) */
    uint64_t lds_per_cu;
    uint32_t cfg_waves, cfg_blocks_per_cu, cfg_lds_mphf;                                /* bgr_aligner_configure */
    uint32_t mode, max_mismatch, partial, max_read_len;                                 /* batch */
    uint64_t n_reads, total_bases;
    uint32_t wide_keys, reserved0;                                                      /* graph header: two-word keys (k > 32) */
} bgr_plan_input;
typedef struct bgr_plan_pass { uint32_t used, blocks, waves_per_block, lds_bytes, table_staged; } bgr_plan_pass;
typedef struct bgr_plan_output {
    bgr_plan_pass pass[6];
    uint32_t level_search, deep_only, x4_levels, memo_cap;
    uint64_t deep_scratch_bytes, arena_ints;
} bgr_plan_output;
int bgr_plan_launch(const bgr_plan_input* in, bgr_plan_output* out);

/* Exhaustive mode: how often the last pass ran for the launch last settled (1 = once, as enqueued; more: reads whose table of remembered calls filled
 * up were run again) and the table size (entries per wave) of its final run.  0 / 0 when the last launch had no last pass (greedy, anchors mode). */
int bgr_aligner_last_pass_runs(const bgr_aligner* a, uint32_t* runs, uint32_t* memo_cap);

/* ---- read files (host) ----------------------------------------------------------------------------
 * Replaces Aligner::getReads (aligner.cpp:46-117) for a whole file: the accepted (header, read) records
 * in file order with the reference's drop rules (characters outside ACGTN, size <= 2, FASTA size <= k,
 * multi-line FASTA, the FASTQ phantom record).  Buffers are owned by the returned object. */
typedef struct bgr_readset bgr_readset;
int bgr_readset_load(const char* path, int fastq, uint32_t k, bgr_readset** out);
/* Same records in the same order, parsed by `threads` host threads over chunks of ~chunk_bytes (0 = default). */
int bgr_readset_load_parallel(const char* path, int fastq, uint32_t k, uint32_t threads, uint64_t chunk_bytes, bgr_readset** out);
uint64_t bgr_readset_count(const bgr_readset* rs);
/* reads_concat / read_offsets[n+1] / headers_concat / header_offsets[n+1] */
int bgr_readset_view(const bgr_readset* rs, const char** reads, const uint64_t** read_offsets, const char** headers, const uint64_t** header_offsets);
void bgr_readset_destroy(bgr_readset* rs);

/* Output formatting of printPath + the fwrite sites (aligner.cpp:600-609, alignerGreedy.cpp:406-427):
 * appends "header\n" + "int." * n + "\n" records for mapped reads to `paths_file` and "header\nread\n" for the
 * others to `notaligned_file` (both FILE* opened by the caller, passed as void*). */
int bgr_write_records(void* paths_file, void* notaligned_file, uint64_t n_reads, const char* headers, const uint64_t* header_offsets,
                      const char* reads, const uint64_t* read_offsets, const int32_t* paths, const uint64_t* path_offsets);

/* ---- whole run -------------------------------------------------------------------------------------
 * Batch form of Aligner::alignAll (aligner.cpp:550-597): maps every file of the comma-separated list `reads_csv`
 * and writes `paths_file` / `notaligned_file` (opened "wb" like aligner.h:85-86) with the bytes the reference
 * produces at -t 1, whatever the thread / GPU count.  Two routes per batch, same bytes: the device takes FASTA text and
 * returns the bytes to write (`route`), or the host pipeline parses chunk-parallel, packs into pinned batches and formats
 * range-parallel; two streams per device, one ordered writer.  counters_out as bgr_aligner_counters. */
typedef struct {
    uint64_t struct_size;      /* sizeof(bgr_run_options) of the header the caller was built with (see bgr_text_batch.struct_size): zero the struct, set this */
    uint32_t n_gpus;           /* devices 0..n_gpus-1 (0 = 1)                                                  */
    uint32_t threads;          /* host threads for parsing / gathering / formatting (-t; 0 = 1)                */
    uint64_t batch_reads;      /* target reads per device batch (0 = default: 128k on the host route, 256k as text)  */
    uint64_t chunk_bytes;      /* parser chunk size (0 = default 8 MiB)                                         */
    uint32_t fastq;            /* -q                                                                            */
    uint32_t write_exhaustive; /* exhaustive mode writes nothing in the reference; 1 = write  */
    uint32_t echo_files;       /* print what the reference's workers print to stdout while mapping, in its -t 1 order: each file
                                  name (aligner.cpp:559,576) and, in exhaustive mode, the block after every tenth getReads()
                                  call (alignerExhaustive.cpp:306-316)                                              */
    uint32_t correction;       /* -c: write header + the read as spelled by its path (recoverPath, aligner.cpp:270-290,
                                  alignerGreedy.cpp:394-404) instead of the path; greedy mode only                 */
    const char* no_overlap_file; /* optional third output (NULL = the reference's behaviour): reads WITHOUT any anchor go
                                  here instead of notAligned.fa -- the split README.md:47-52 documents and
                                  alignerGreedy.cpp:414-419 disables                                               */
    uint32_t first_device;     /* devices first_device .. first_device + n_gpus - 1 (one process per GPU under a launcher
                                  that does not hide the others: first_device = the rank's local index, n_gpus = 1)   */
    uint32_t route;            /* 0 = automatic: FASTA input without -c / --no-overlap / -b progress blocks goes through the device as
                                  text (bgr_align_fasta_text: parsing, packing, mapping and record formatting on the GPU; pieces of an
                                  irregular shape fall back to the host parser one by one); 1 = host parser + host formatter always */
    uint32_t numa;             /* 0 = while the run lasts, its threads (the caller's included) and the page-locked memory they allocate are kept
                                  on the CPUs next to the run's devices when all of them share one NUMA node, and the pool of host threads is
                                  clamped to that CPU set; 1 = the caller's affinity is left alone                          */
    uint32_t split_output;     /* 0 = the reference's two files.  1 = one pipeline PER DEVICE: device d of the run maps the d-th of n_gpus
                                  contiguous shares of the input (cut at record starts, over the files of the list taken together) and writes
                                  its own pair `<paths_file>.<d>` / `<notaligned_file>.<d>`; the pairs concatenated in device order are the
                                  reference's -t 1 bytes.  One ordered stream into ONE file is bound by what a single writer gets out of the
                                  file system (~6-13 GB/s: 125-250 Mreads/s at ~50 bytes per read) whatever the number of GPUs; this form has
                                  no stage shared between devices.  FASTA input without -c, --no-overlap and -b progress blocks; any
                                  other run ignores the flag.                                                                  */
    uint32_t gaf;              /* --gaf: the paths file holds one GAF line per mapped read, in input order, instead of header + path ints (0 = the
                                  reference's records).  Tab separated: name (the header line without its first character, up to the first space
                                  or tab; '*' if empty), read size L, query start, query end, '+', the path's segments ('>' id for a unitig read
                                  forward, '<' id for its reverse complement; ids are the 1-based ordinals of the paths file), walk size, path
                                  start, path end, matches, block size, 255, NM:i:mismatches.  The walk is the one -c spells (recoverPath,
                                  aligner.cpp:270-290), the orientations the ones compactionEnd glued on; cl = min(L, walk size - path[0])
                                  characters are covered.  A read mapped on its reverse complement (BGR_ST_RC) is described as it stands in
                                  the input: its path reversed with every orientation flipped, query [L - cl, L), path start = walk size -
                                  (path[0] + cl); a forward read: query [0, cl), path start = path[0].  The segments spelled and cut to
                                  [path start, path end) are the read -c writes; NM = the positions where it differs from the read's
                                  characters (an N always differs), matches = cl - NM, block size = cl.  Greedy modes (also -G, -q,
                                  --no-overlap, several devices, the host route, k up to 64); refused with BGR_E_ARG on a graph with non-ACGT
                                  unitig characters (has_exceptions: reversing a path does not reverse what it spells there), in exhaustive
                                  mode and together with `correction`.  A path that spells no walk ends the run as -c's does
                                  (BGR_E_COMPACTION).  split_output is ignored, as with -c.                                          */
    uint32_t abundance;        /* --abundance: every aligner of the run counts, per unitig, the reads, bases and k-mers mapped onto it; the tables of all
                                  aligners and devices are summed when the run ends and kept in the graph (bgr_graph_abundance) until the next such run.
                                  Greedy modes, where a mapped read's row is [off, id_1 .. id_n] (the offset in the walk, then signed 1-based unitig ids).
                                  With K1 = k - 1, len_j = the length of unitig |id_j| and L the read's length, the walk's extents are s_1 = 0,
                                  e_j = s_j + len_j, s_(j+1) = e_j - K1, plen = e_n; cl = max(0, min(L, plen - off)) and the read covers the walk
                                  positions [off, off + cl).  For every occurrence j, with o_j = max(0, min(off + cl, e_j) - max(off, s_j)):
                                  reads[|id_j|] += 1 (every occurrence, whatever o_j: what counting the ids of the paths file gives),
                                  bases[|id_j|] += o_j (the k-1 characters two neighbours share count for both), kmers[|id_j|] += max(0, o_j - K1).
                                  An occurrence whose id is 0 or beyond n_unitigs (the mapper writes none) adds nothing and has len_j = 0 in the walk;
                                  the next e then lies in front of it, and plen is the largest e_j of such a row.
                                  Neither a unitig's orientation nor the read's strand enters; unmapped reads add nothing; integer adds commute, so
                                  the totals do not depend on batches, routes, streams or devices.  Any graph greedy mode maps (k up to 64, exception
                                  planes), together with fastq, correction, gaf, no_overlap_file, several devices, split_output, both routes; the
                                  run's files and counters are what they are without it.  Refused with BGR_E_ARG in exhaustive mode (other rows).
                                  A run that fails (BGR_E_COMPACTION too) leaves no totals.  (The field took the struct's four bytes of tail padding:
                                  sizeof is unchanged.) */
} bgr_run_options;
/* bgr_align_all keeps its page-locked staging buffers for the next call of the process (they cost ~0.2 s per GB to allocate);
 * this frees them. */
void bgr_host_cache_release(void);
int bgr_align_all(bgr_graph* g, const bgr_params* p, const bgr_run_options* o, const char* reads_csv, const char* paths_file,
                  const char* notaligned_file, uint64_t counters_out[5], double* mapping_seconds);

/* The totals of the last bgr_align_all with bgr_run_options.abundance = 1 on this graph (n_rows must be its n_unitigs; row i = unitig id i + 1);
 * BGR_E_ARG if there are none.  bgr_write_abundance (host code, deterministic bytes) writes such a table as text: the line
 * "#unitig<TAB>length<TAB>reads<TAB>bases<TAB>kmers", then one line per unitig 1 .. n in order, zero rows included, decimal, tab separated;
 * the lengths come from the graph (one with a host blob). */
int bgr_graph_abundance(const bgr_graph* g, bgr_unitig_abundance* out, uint64_t n_rows);
int bgr_write_abundance(const char* path, const bgr_graph* g, const bgr_unitig_abundance* rows, uint64_t n_rows);

/* The read-supported graph of a whole run.  bgr_run_options has no room left (its size is part of the ABI), so the switch is the graph's:
 * bgr_graph_links_enable(g, 1) is sticky, and every later bgr_align_all on the graph counts unitig abundance (as with bgr_run_options.abundance) and
 * links (bgr_link above) in every aligner of the run; the tables of all aligners and devices are summed when the run ends and kept in the graph:
 * bgr_graph_abundance has the unitigs' totals, bgr_graph_links the links (canonical, sorted by key, counts > 0; *n = their number, BGR_E_CAPACITY
 * with *n set when cap is smaller; BGR_E_ARG if there are none).  With the switch on, exhaustive mode is refused before any device work (BGR_E_ARG;
 * the message names -b and --gfa); a run that fails (BGR_E_COMPACTION too) leaves no totals; a run with the switch off leaves the last totals alone.
 * The run's files, counters and stdout are what they are without it.
 * bgr_write_gfa (host code, deterministic bytes) writes GFA 1.0: the line "H<TAB>VN:Z:1.0"; for every unitig i = 1 .. n in order
 * "S<TAB>i<TAB>sequence<TAB>LN:i:length<TAB>RC:i:reads<TAB>KC:i:kmers" (zero rows included; the sequence as bgr_graph_unitigs holds it, non-ACGT
 * characters kept; reads and kmers from abundance_rows); for every link with count > 0, in the order given -- which must be ascending by key, as
 * bgr_graph_links delivers -- "L<TAB>|from|<TAB>+ or -<TAB>|to|<TAB>+ or -<TAB>(k-1)M<TAB>RC:i:count".  Every line ends with a newline.  The ids are the
 * 1-based ordinals of the paths file and of --gaf: every GAF line of the same run walks L lines of this file.  BGR_E_ARG on a wrong n_rows, a link
 * beyond the graph or out of order, or a graph without unitig characters; BGR_E_IO on a path it cannot write. */
int bgr_graph_links_enable(bgr_graph* g, uint32_t on);
int bgr_graph_links_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_links(const bgr_graph* g, bgr_link* out, uint64_t cap, uint64_t* n);
int bgr_write_gfa(const char* path, const bgr_graph* g, const bgr_unitig_abundance* abundance_rows, uint64_t n_rows, const bgr_link* links, uint64_t n_links);

/* Bubbles: the variants the graph already holds.  A variant that was abundant enough to enter a compacted de Bruijn graph is no mismatch anywhere
 * (bgr_variant_site is silent about it): a unitig s leaves through two links to two branch unitigs that both rejoin one unitig t, and the reads of
 * either allele map onto their own branch.  The bubbles are a function of a set of counted links alone:
 *   input      canonical links with counts (bgr_link) and a threshold min_link >= 1
 *   supported  a link with count >= min_link
 *   edges      a supported canonical link (a, b) is the oriented edge a -> b and its strand mate -b -> -a (one edge when b == -a).  out(x) = the
 *              supported successors of the signed id x; in(x) has as many members as out(-x)
 *   bubble     an oriented s opens the bubble (s, t, b, c) when |out(s)| == 2 with out(s) = {b, c}; |in(b)| == |in(c)| == 1; |out(b)| == |out(c)| == 1
 *              and both lead to the same t; |in(t)| == 2; and |s|, |b|, |c|, |t| are four different unitigs
 *   mates      (s, t, b, c) and (-t, -s, -b, -c) are one bubble read from the two strands: it is reported once, under whichever of (s, t) and
 *              (-t, -s) has the smaller key (bgr_link_canonical's order; never equal, because |s| != |t|)
 *   record     source = s, sink = t, branch[0] the branch with the smaller (|id|, id < 0), count = the traversals of source -> branch[0],
 *              branch[0] -> sink, source -> branch[1], branch[1] -> sink
 *   order      by (|source|, source < 0): an oriented id opens at most one bubble, so the order is total
 * Exact integers, independent of batching, routes, streams and devices.  For an isolated SNV both branches are 2k - 1 long and differ at index k - 1;
 * three alleles at one site give |out(s)| == 3 and no bubble.
 * The device side (bgreat_amd/csrc/bubbles_kernels.h) runs four launches in stream order over {key, count} pairs in HBM -- adjacency with one 32-bit
 * atomic per oriented edge (the first two successors of an id are kept, later ones only counted), a count per tile of BGR_BUBBLES_TILE oriented ids,
 * a scan, and the emit at each record's final place: no sort, no atomics on the output, no workgroup waits for another -- in 56 bytes of scratch per
 * unitig (222 MB on the chr1-scale graph), allocated for the call and freed behind it: BGR_E_NOMEM, with nothing left allocated, when the device
 * does not have it.  All three calls set *n to the number of bubbles, always, and return BGR_E_CAPACITY with nothing copied when cap is smaller.
 * bgr_links_bubbles: a list (sorted by key, canonical, ids within 1 .. n_unitigs, as bgr_aligner_links delivers it -- anything else, min_link == 0
 * and n_unitigs >= 2^30 are BGR_E_ARG before any device work) is uploaded to `device` and called there.
 * bgr_aligner_bubbles: the aligner's live table of links is called where it lies, its streams waited for; only the records cross to the host.
 * BGR_E_ARG when links were never enabled, BGR_E_CAPACITY (with a message) when the table has overflowed, as bgr_aligner_links.
 * bgr_aligner_bubbles_times: the last such call's four launches in milliseconds (zeroes when events are switched off).
 * bgr_graph_bubbles_enable(g, on, min_link) is a sticky switch like bgr_graph_links_enable and implies it for the run (BGR_E_ARG for min_link == 0,
 * a graph without a host blob or with non-ACGT unitig characters): at the end of a successful bgr_align_all the run's merged links -- gathered on
 * the host exactly as without the switch -- are uploaded once (16 bytes per link) to the device of the first aligner that was collected and called
 * there; bgr_graph_bubbles delivers the records (BGR_E_ARG when there are none: a failed run, BGR_E_COMPACTION too, leaves no totals).  Merging the
 * aligners' tables on the device instead is out of scope here.
 * bgr_write_bubbles (host code, deterministic bytes; BGR_E_ARG on a graph created from a blob, which carries no unitig characters, and for a record
 * that names a unitig the graph does not have) writes the line "#source sink branch1 branch2 len1 len2 in1 out1 in2 out2 kind diff" and one line per
 * record, all tab-separated: the four signed ids as in the paths file, the branches' lengths, count[0 .. 3], and how the two branches compare as
 * oriented (a branch with a negative id is reverse-complemented): kind "snv" (equal length, exactly one position differs) with diff "pos:X>Y", pos
 * 0-based on oriented branch1, X its letter and Y branch2's; "mnv" (equal length otherwise) and "indel" (lengths differ), both with diff ".". */
#define BGR_BUBBLES_TILE 1024u
typedef struct { int32_t source, sink, branch[2]; uint64_t count[4]; } bgr_bubble;
int bgr_links_bubbles(int device, const bgr_link* links, uint64_t n_links, uint64_t n_unitigs, uint64_t min_link, bgr_bubble* out, uint64_t cap, uint64_t* n);
int bgr_aligner_bubbles(bgr_aligner* a, uint64_t min_link, bgr_bubble* out, uint64_t cap, uint64_t* n);
int bgr_aligner_bubbles_times(bgr_aligner* a, double ms[4]);
int bgr_graph_bubbles_enable(bgr_graph* g, uint32_t on, uint64_t min_link);
int bgr_graph_bubbles_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_bubbles(const bgr_graph* g, bgr_bubble* out, uint64_t cap, uint64_t* n);
int bgr_write_bubbles(const char* path, const bgr_graph* g, const bgr_bubble* bubbles, uint64_t n);

/* Triples: which way INTO a unitig goes with which way OUT of it -- what only a whole read knows, and what neither the links nor the bubbles keep.
 * A mapped read's row in the greedy modes is [off, id_1 .. id_n] with signed 1-based ids; every three consecutive ids (a, b, c) =
 * (id_j, id_j+1, id_j+2), j = 1 .. n-2, are one traversal of a triple: a row of n ids gives n - 2.  (a, b, c) and (-c, -b, -a) are one triple read
 * from the two strands: the canonical form is the one with the smaller tuple (|a|, a < 0, |b|, b < 0, |c|, c < 0), compared lexicographically (the two
 * always differ: b != -b), and count[canonical triple] += 1 per traversal.  Neither the status nor off enters; a triple in which any id is 0 or beyond
 * n_unitigs is skipped (INT32_MIN counts as beyond); a row that is not wholly inside the arena is skipped, as the links kernel skips it.  The counts
 * are exact 64-bit integers and do not depend on batching, routes, streams or devices.
 * Counted on the device as the links are: off unless enabled; while enabled every greedy / anchors launch of the aligner, through every entry point,
 * is followed on its stream by one kernel ("bgr_triples_kernel" in bgr_aligner_kernel_times while a slot is free; sixteen lanes per read, behind the
 * links kernel) that adds the launch's triples to an open-addressed hash table {u64 k0, u64 k1, u64 count} in device memory, k0 = the link key of
 * (a, b), k1 = |c| << 1 | (c < 0).  The 93-bit key does not fit one compare-and-swap: a slot is claimed word by word, each word by one CAS from 0,
 * lock-free and without any thread waiting for another (bgreat_amd/csrc/triples_kernels.hip has the insert and why no key lands in two slots).
 * The table is sized when counting is first enabled, from the graph (one with a host blob, fewer than 2^30 unitigs): a walk glues unitigs only
 * where they overlap in exactly k-1 characters, so bgr_graph_triples_bound = the sum over the unitigs u of (oriented unitigs that end with u's first
 * (k-1)-mer) x (oriented unitigs that begin with its last) bounds the distinct canonical triples any rows on the graph can hold
 * (bgreat_amd/csrc/triples_kernels.h has the argument); the capacity is the power of two that is at least twice that, at least 1024, 24 bytes per
 * slot: BGR_E_NOMEM, with nothing left allocated, when the device does not have it.  Should an insert find no place all the same, it is counted in
 * an overflow word, and bgr_aligner_triples / the run return BGR_E_CAPACITY with a message until bgr_aligner_reset_triples.  The internal streams
 * of overlapped batches add to the same table.  An exhaustive launch on an enabled aligner is refused (BGR_E_ARG); disabling keeps the table; a
 * launch that fails afterwards may have added part of its rows.  There is one form of the kernel, every traversal an insert in device memory: on a
 * graph of a handful of triples all adds of a launch meet in a few addresses and serialise (no table in LDS in front, as the links have).
 * bgr_aligner_triples synchronises and delivers the canonical triples with a count, sorted by the tuple above; *n = their number, always,
 * BGR_E_CAPACITY when cap is smaller (the call with cap 0 moves two words, not the table) or the table has overflowed; BGR_E_ARG when triples were
 * never enabled.  bgr_aligner_triples_info: out = {slots of the table, the graph's bound, traversals that found no place, used slots}.
 * bgr_triple_canonical: the canonical form of (a, b, c) by the code the kernel runs (BGR_E_ARG for an id that is 0 or not below 2^30 in size).
 * bgr_graph_triples_enable(g, 1) is sticky like bgr_graph_links_enable: every later bgr_align_all on the graph counts unitig abundance and triples
 * in every aligner of the run; each aligner's used slots are gathered on the host, merged and sorted when the run ends, and bgr_graph_triples
 * delivers them (BGR_E_ARG when there are none: a failed run, BGR_E_COMPACTION too, leaves no totals).  Exhaustive mode is refused before any device
 * work.  bgr_write_triples (host code, deterministic bytes; the triples sorted as delivered, ids within the graph) writes "#from via to count" and
 * one tab-separated line per triple with a count above 0. */
typedef struct { int32_t from, via, to, reserved; uint64_t count; } bgr_triple;   /* reserved is 0 */
int bgr_aligner_triples_enable(bgr_aligner* a, uint32_t on);
int bgr_aligner_triples(bgr_aligner* a, bgr_triple* out, uint64_t cap, uint64_t* n);
int bgr_aligner_reset_triples(bgr_aligner* a);
int bgr_aligner_triples_info(bgr_aligner* a, uint64_t out[4]);
int bgr_triple_canonical(int32_t a, int32_t b, int32_t c, bgr_triple* out);
int bgr_graph_triples_bound(bgr_graph* g, uint64_t* bound);
int bgr_graph_triples_enable(bgr_graph* g, uint32_t on);
int bgr_graph_triples_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_triples(const bgr_graph* g, bgr_triple* out, uint64_t cap, uint64_t* n);
int bgr_write_triples(const char* path, const bgr_graph* g, const bgr_triple* triples, uint64_t n);

/* Read-backed phasing of neighbouring bubbles.  Two heterozygous sites close together are two bubbles that share a unitig; the reads that cross
 * both say which alleles go together.  Take bubbles as bgr_graph_bubbles delivers them, each read in both orientations, (s, t, b, c) and
 * (-t, -s, -b, -c).  Oriented bubbles X and Y are neighbours through m when X's sink is m and Y's source is m; the mate pair through -m is the same
 * pair and is reported once, in the reading with m > 0.  An oriented id is the source of at most one bubble and the sink of at most one, so the
 * pairs form chains.  A record: via = m, source = X's source, in[0 .. 1] = X's branches as oriented in this reading in (|id|, id < 0) order,
 * out[0 .. 1] = Y's branches likewise, sink = Y's sink, count[2 i + j] = the count of the canonical triple of (in[i], m, out[j]) -- n11, n12, n21,
 * n22.  Every neighbour pair is a record, those no read crosses too; the records are ordered by via.  Everything is integers.
 * bgr_bubbles_phase: host code (a binary search over the sorted triples per count; a few thousand records at a run's end are no hot path).  The
 * triples must be canonical and strictly ascending, as bgr_aligner_triples / bgr_graph_triples deliver them, every id non-zero and below 2^30 in
 * size: BGR_E_ARG otherwise.  *n = the number of records, always; BGR_E_CAPACITY with nothing copied when cap is smaller.
 * bgr_graph_phase_enable(g, on, min_link) is sticky and implies the triples, bubbles and links switches for the run (BGR_E_ARG for min_link == 0, a
 * graph without a host blob or with non-ACGT unitig characters -- the bubbles' refusal).  The run's bubbles are called with min_link -- with the
 * bubbles' own threshold when bgr_graph_bubbles_enable is on as well: a run has one set of bubbles -- and joined with its merged triples behind the
 * bubbles' end; bgr_graph_phase delivers the records, bgr_graph_bubbles and bgr_graph_triples what they were joined from.
 * bgr_write_phase (host code, deterministic bytes) writes "#via source in1 in2 out1 out2 sink n11 n12 n21 n22 phase" and one tab-separated line
 * per record; phase is "cis" when n11 + n22 > n12 + n21, "trans" when it is smaller, "." when they are equal, zero included. */
typedef struct { int32_t via, source, in[2], out[2], sink, reserved; uint64_t count[4]; } bgr_phase;   /* reserved is 0 */
int bgr_bubbles_phase(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_triple* triples, uint64_t n_triples, bgr_phase* out, uint64_t cap, uint64_t* n);
int bgr_graph_phase_enable(bgr_graph* g, uint32_t on, uint64_t min_link);
int bgr_graph_phase_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_phase(const bgr_graph* g, bgr_phase* out, uint64_t cap, uint64_t* n);
int bgr_write_phase(const char* path, const bgr_graph* g, const bgr_phase* records, uint64_t n);

/* Haplotype blocks: the phased pairs chained.  A phase file is a list of pairs; a block says which bubbles hang together, in what order, and which
 * branch of each lies on the haplotype of the first bubble's first branch.  Input: `bubbles` as bgr_graph_bubbles / bgr_links_bubbles deliver them
 * (sorted, canonical reading), `phase` as bgr_bubbles_phase makes them from exactly these bubbles, and a threshold min_phase >= 1.
 * Nodes: node 2 i is bubble record i as given, (s, t, b0, b1) with the branches in (|id|, id < 0) order; node 2 i + 1 is its mate
 * (-t, -s, -b0, -b1); bubble(x) = x >> 1, reversed(x) = x & 1, mate(x) = x ^ 1.
 * Decided link: a phase record through m joins X (sink m) to Y (source m); it is decided when |(n11 + n22) - (n12 + n21)| >= min_phase (sums
 * that do not wrap, as in bgr_write_phase), with parity 0 when cis and 1 when trans.  A decided record gives the link X -> Y and the mate link
 * mate(Y) -> mate(X) with the same parity (its four counts are the transposed matrix: cis stays cis); an undecided record gives no link.  With
 * min_phase == 1, decided is exactly "the phase file says cis or trans".
 * Components: every node has at most one successor and one predecessor, so the components are paths and rings.  A component and its mate (every
 * node mated, the order reversed) are two readings of one block; a component cannot be its own mate (that needs a node equal to its mate, or a
 * link x -> mate(x), whose via would be its own negative), so every bubble record appears in exactly one reported block, exactly once.
 * The reading that is reported: the first node of a path is its head, the first node of a ring its smallest node index, and the block is reported
 * in the reading whose first node is smaller.  A ring is opened at the link that enters its first node, which becomes the head; every entry of it
 * carries BGR_BLOCK_CIRCULAR, and BGR_BLOCK_CONFLICT as well when the parity of the removed link differs from the haplotype of the ring's last
 * node: an odd number of trans links around the ring, phasing that contradicts itself.
 * Haplotype: hap(head) = 0, hap(next(x)) = hap(x) ^ parity(x -> next(x)); branch[hap] of the bubble's record lies on haplotype A, the other on B.
 * Order: blocks by their first node's index, numbered from 1; within a block the entries in chain order; a bubble with no decided link is a block
 * of size 1, read as given.  An entry: block (1-based), index (0-based place in the block), size (the block's length), bubble (0-based index into
 * the list of bubbles), flags.  Everything is integers and the result is deterministic.
 * bgr_phase_blocks uploads the two lists to `device` and chains them there (bgreat_amd/csrc/blocks_kernels.h has the passes: an index of the
 * nodes by source, one thread per phase record for the links, pointer jumping towards the heads with the parity carried along, rings opened and
 * ranked again, then count / scan / place per tile of BGR_BLOCKS_TILE nodes; launches in stream order on one stream, no workgroup waits for
 * another, no sort, no atomics on the output).  The lists are checked on the host first -- ids not 0, below 2^30 and within n_unitigs, the bubbles
 * canonical and strictly ascending by source, the phase records strictly ascending by a positive via -- and the links on the device: a source two
 * nodes share, a record whose bubbles are missing or differ from its in / out / sink, a second link into or out of a node.  All of these are
 * BGR_E_ARG with a message and nothing copied.  *n is always set; for valid input it equals n_bubbles; BGR_E_CAPACITY with nothing copied when cap
 * is smaller; n_bubbles == 0 is BGR_OK with *n = 0 and no device work; BGR_E_ARG for min_phase == 0.  The scratch (136 bytes per bubble and 8
 * per unitig) lives for the call: BGR_E_NOMEM, with nothing left allocated, when the device does not have it.  bgr_phase_blocks_times: the
 * milliseconds of the calling thread's last call -- index + link, ranking (all rounds), place (events on the call's stream), and the whole call with its
 * allocations, copies and waits on the host's clock -- zeroes when the last call did no device work.
 * bgr_graph_blocks_enable(g, on, min_link, min_phase) is sticky and implies the phase switch for the run, with its rule for whose min_link the
 * run's one set of bubbles is called with (the bubbles' own when bgr_graph_bubbles_enable is on, else the phase's when bgr_graph_phase_enable is
 * on, else this one) and its refusals, min_phase == 0 too.  When the run ends, its bubbles and phase records are uploaded once to the device of the
 * first aligner it collected and chained there; bgr_graph_blocks delivers the entries (BGR_E_ARG when there are none: a failed run,
 * BGR_E_COMPACTION too, leaves none).
 * bgr_write_blocks (host code, deterministic bytes) writes "#block index size bubble source sink hapA hapB strand ring" and one tab-separated line
 * per entry: bubble the 1-based line ordinal of the record in the bubbles file of the same run; source, sink, hapA, hapB the signed ids as the
 * block's reading orients them (for a reversed entry -sink, -source, -branch[hap], -branch[1 - hap]); strand + or -; ring ".", "circular" or
 * "conflict".  Spelling the haplotypes' sequences from the blocks: bgr_haplotype, below. */
typedef struct { uint32_t block, index, size, bubble; uint32_t flags; uint32_t reserved; } bgr_block_entry;   /* 24 bytes, reserved is 0 */
#define BGR_BLOCK_REVERSED 1u   /* the bubble is read as its mate */
#define BGR_BLOCK_HAP      2u   /* branch[1] of the record is on haplotype A */
#define BGR_BLOCK_CIRCULAR 4u   /* set on every entry of an opened ring */
#define BGR_BLOCK_CONFLICT 8u   /* likewise */
#define BGR_BLOCKS_TILE 1024u
int bgr_phase_blocks(int device, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_phase* phase, uint64_t n_phase, uint64_t n_unitigs,
                     uint64_t min_phase, bgr_block_entry* out, uint64_t cap, uint64_t* n);
int bgr_phase_blocks_times(double ms[4]);
int bgr_graph_blocks_enable(bgr_graph* g, uint32_t on, uint64_t min_link, uint64_t min_phase);
int bgr_graph_blocks_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_blocks(const bgr_graph* g, bgr_block_entry* out, uint64_t cap, uint64_t* n);
int bgr_write_blocks(const char* path, const bgr_graph* g, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries, uint64_t n);

/* The haplotypes' sequences: the two sequences every block stands for, spelled on the device from the graph's 2-bit store (every unitig lies there
 * in both strands, so an oriented unitig is a base offset and a length, and nothing is ever reversed).
 * Input: `bubbles` as bgr_graph_bubbles delivers them; `entries` as bgr_phase_blocks / bgr_graph_blocks deliver them for exactly these bubbles,
 * block after block, chain order inside a block; the graph's k; a threshold min_block >= 1.
 * Oriented ids of an entry (the ones bgr_write_blocks prints): (src, snk, a, b) = (source, sink, branch[hap], branch[1 - hap]) of the bubble's
 * record, with BGR_BLOCK_REVERSED (-sink, -source, -branch[hap], -branch[1 - hap]); hap = (flags >> 1) & 1.
 * Walks: a block with the entries e_0 .. e_{n-1} has two walks of 2 n + 1 oriented unitigs, walk_A = src_0, a_0, snk_0, a_1, snk_1, .., a_{n-1},
 * snk_{n-1}, and walk_B the same with b_i in the place of a_i.  snk_i == src_{i+1} must hold -- that is what a decided link is; entries for which
 * it does not, entries that are not block after block in chain order, and what bgr_write_blocks refuses are BGR_E_ARG, checked on the host with
 * nothing copied.
 * Spelling: the oriented unitig w_0 goes in whole, every later w_j without its first k - 1 characters; a negative id is the reverse complement.
 * Length = the sum of the 2 n + 1 lengths - 2 n (k - 1).
 * Rings: an opened ring is spelled as the linear walk it was opened into: its first and last unitig are the same one.  The ring flags travel into
 * the record and the header line; a `conflict` ring is spelled all the same.
 * Junctions: junction j >= 1 of a walk is good when the last k - 1 characters of oriented w_{j-1} equal the first k - 1 of oriented w_j.  On lists
 * that come from a run every junction is good (a path glues unitigs only where they overlap in exactly k - 1); on arbitrary lists the spelling is
 * still defined as above, and the call delivers the number of bad junctions over all kept sequences (2 n per sequence are looked at) as one
 * 64-bit count.
 * Kept blocks and order: blocks with size >= min_block are kept; the sequences come in block order, A before B; a sequence's ordinal counts kept
 * blocks only.  A record: block (the entries' number), hap (0 = A, 1 = B), size, flags (the ring bits only), and offset, length into one byte
 * buffer of ACGT characters, the sequences back to back.  Everything is integers and the bytes are deterministic.
 * bgr_blocks_haplotypes uploads the two lists to `device`, where the graph must be resident (bgr_graph_device_blob non-NULL: BGR_E_ARG otherwise),
 * and spells there (bgreat_amd/csrc/haplotypes_kernels.h has the passes: one thread per (entry, hap) for the pieces, lengths and junctions, a
 * 64-bit scan, the spelling assigned by output in aligned 16-byte stores, the records; launches in stream order on one stream, no workgroup waits
 * for another, no atomics on the output).  BGR_E_ARG too for a graph with exception planes (non-ACGT unitig characters), min_block == 0, malformed
 * lists and ids outside the graph.  *n, *seq_bytes and *bad_junctions are always set for valid input; when cap < *n or seq_cap < *seq_bytes the call
 * returns BGR_E_CAPACITY with nothing copied, and only the first two passes have run: the sizing call is cheap.  n_entries == 0 is BGR_OK with
 * zeroes and no device work.  The scratch (128 bytes per entry) and the output live on the device for the call: BGR_E_NOMEM, with nothing left
 * allocated, when it lacks them.  bgr_blocks_haplotypes_times: the milliseconds of the calling thread's last call -- items + scan, spell, records
 * (events on the call's stream; the one in front of the spell launch is recorded behind the sizing copies, the wait and the allocations of the
 * output, so the spell stage is the kernel alone), and the whole call with its allocations, copies and waits on the host's clock -- zeroes when the
 * last call did no device work (a sizing call reports its first stage and the whole).
 * bgr_graph_haplotypes_enable(g, on, min_link, min_phase, min_block) is sticky and implies the blocks switch for the run, with its rules for the
 * thresholds and its refusals, min_block == 0 too.  When the run ends, its bubbles and entries are spelled once on the device of the first aligner
 * it collected; bgr_graph_haplotypes delivers the records and bytes of the last successful run (BGR_E_ARG when there are none: a failed run,
 * BGR_E_COMPACTION too, leaves none; BGR_E_CAPACITY with both sizes and nothing copied when either capacity is smaller).  A run whose spelling
 * finds a bad junction fails with BGR_E_INTERNAL.
 * bgr_write_haplotypes (host code, deterministic bytes) writes per record the line
 *   >block<b>_<A|B> bubbles=<size> length=<L> ring=<.|circular|conflict> walk=<w>
 * and the sequence on one line; w is the walk in GAF notation (">12<7>9": > forward, < reverse complement, unitig ids from 1), built from the
 * entries and the bubbles on the host.  Records that are not those of the entries' kept blocks, back to back in seq_bytes bytes, are BGR_E_ARG. */
typedef struct { uint32_t block, hap, size, flags; uint64_t offset, length; } bgr_haplotype;   /* 32 bytes */
int bgr_blocks_haplotypes(const bgr_graph* g, int device, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries, uint64_t n_entries,
                          uint64_t min_block, bgr_haplotype* out, uint64_t cap, uint64_t* n, char* seq, uint64_t seq_cap, uint64_t* seq_bytes, uint64_t* bad_junctions);
int bgr_blocks_haplotypes_times(double ms[4]);
int bgr_graph_haplotypes_enable(bgr_graph* g, uint32_t on, uint64_t min_link, uint64_t min_phase, uint64_t min_block);
int bgr_graph_haplotypes_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_haplotypes(const bgr_graph* g, bgr_haplotype* out, uint64_t cap, uint64_t* n, char* seq, uint64_t seq_cap, uint64_t* seq_bytes);
int bgr_write_haplotypes(const char* path, const bgr_graph* g, const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries, uint64_t n_entries,
                         const bgr_haplotype* haps, uint64_t n, const char* seq, uint64_t seq_bytes);

/* Re-compaction: a kept subset of the graph's unitigs merged into maximal non-branching chains and spelled as new unitigs -- the graph the reads
 * support, as a unitig file that a next run takes as its graph.  All integers, every byte deterministic (tests/recompact_ref.py is the executable
 * definition).
 * Terms: K = k - 1.  An oriented id x is +u or -u with 1 <= u <= n; spell(x) is unitig u, or its reverse complement when x is negative; first(x)
 * and last(x) are the first and last K characters of spell(x).  Nodes are ordered by (|x|, x < 0).  keep[u] is 0 or 1 per unitig.
 * Edges: x -> y is an edge when both are kept and last(x) == first(y); y may be x or -x, and two different unitigs with equal ends both count.
 * out(x) is the number of edges leaving x, in(x) = out(-x); the mate of x -> y is -y -> -x.
 * Merge links: x -> y is a merge link when out(x) == 1, in(y) == 1 and |x| != |y| (no self-loop x -> x, no hairpin x -> -x).  Every node has at
 * most one merge successor and one predecessor, the links are closed under mating, the components are paths and rings, and no component holds both
 * z and -z.
 * Chains: a component and its mate are two readings of one chain, reported once, in the reading whose first node is smaller: a path's first node
 * is its head (head is compared with -tail; a single unitig is reported as +u); a ring's first node is its smallest node, so it is read in the
 * direction in which its smallest-|id| unitig is forward, opened at the link that enters that node and flagged circular.
 * Sequence: the first unitig goes in whole, every later one without its first K characters: length = the sum of the lengths - (m - 1) K.  An opened
 * ring is spelled as the linear walk: its last K characters equal its first K.
 * Order: chains are ordered by first node ascending and numbered from 1.
 * Properties: every kept unitig lies in exactly one chain; the multiset of canonical k-mers of the output equals that of the kept unitigs;
 * compacting the output again with everything kept merges nothing.
 * A record: seq_off, seq_len into one byte buffer of ACGT characters (the chains back to back), walk_off into one array of oriented ids (the chains'
 * walks back to back), n_unitigs, flags (BGR_CHAIN_CIRCULAR).
 * bgr_graph_recompact works on `device`, where the graph must be resident, for any subset: keep has one byte per unitig 1..n and n_keep must equal
 * the graph's number of unitigs (bgreat_amd/csrc/recompact_kernels.h has the passes: the ends counted in a table indexed by meta's key indices,
 * unique successors, pointer jumping with rings cut, count / scan / place, the spelling assigned by output in aligned 16-byte stores, the records;
 * launches in stream order on one stream, no workgroup waits for another, no atomics on any output).  *n, *walk_n and *seq_bytes are set once the
 * sizing passes have run; when a capacity is smaller the call returns BGR_E_CAPACITY with nothing copied (a call with capacities of 0 is the
 * sizing call).  BGR_E_ARG with nothing copied for a graph with exception planes (non-ACGT unitig characters), a wrong n_keep, or a graph not on
 * the device.  The scratch (169 bytes per unitig and 16 per key index) and the output live on the device for the call: BGR_E_NOMEM, with nothing
 * left allocated, when it lacks them.  bgr_graph_recompact_times: the milliseconds of the calling thread's last call -- ends + successors, ranking,
 * place + scans, spell, records (events on the call's stream).
 * bgr_graph_recompact_enable(g, on, min_reads) is sticky and implies unitig abundance for the run: when the run ends,
 * keep[u] = (reads[u] >= min_reads) from the run's summed abundance (reads counts the occurrences of u in the paths of MAPPED reads; min_reads 0
 * keeps everything) is uploaded once to the device of the first aligner the run collected and compacted there; bgr_graph_recompact_result delivers
 * the last successful run's records, walk and characters with the same two-call convention (BGR_E_ARG when there are none: a failed run,
 * BGR_E_COMPACTION too, leaves none).  Exhaustive mode is refused as with abundance.
 * bgr_write_recompact (host code, deterministic bytes) writes FASTA that a next run reads as its unitig file; per chain the line
 *   >{ordinal} LN:i:{length} unitigs={m} ring={.|circular} walk={>12<7>9}
 * (the walk in GAF notation over the 1-based ordinals of the INPUT graph) and the sequence on one line.  Records that do not lie back to back in
 * walk and seq, or a walk id outside the graph, are BGR_E_ARG. */
#define BGR_CHAIN_CIRCULAR 1u
typedef struct { uint64_t seq_off, seq_len, walk_off; uint32_t n_unitigs, flags; } bgr_chain;   /* 32 bytes */
int bgr_graph_recompact(const bgr_graph* g, int device, const uint8_t* keep, uint64_t n_keep, bgr_chain* out, uint64_t cap, uint64_t* n, int32_t* walk, uint64_t walk_cap,
                        uint64_t* walk_n, char* seq, uint64_t seq_cap, uint64_t* seq_bytes);
int bgr_graph_recompact_times(double ms[5]);
int bgr_graph_recompact_enable(bgr_graph* g, uint32_t on, uint64_t min_reads);
int bgr_graph_recompact_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_recompact_result(const bgr_graph* g, bgr_chain* out, uint64_t cap, uint64_t* n, int32_t* walk, uint64_t walk_cap, uint64_t* walk_n, char* seq, uint64_t seq_cap,
                               uint64_t* seq_bytes);
int bgr_write_recompact(const char* path, const bgr_graph* g, const bgr_chain* chains, uint64_t n, const int32_t* walk, uint64_t walk_n, const char* seq, uint64_t seq_bytes);

/* Haplotags: which haplotype of which block a READ lies on, from blocks that are given -- the --blocks file of an earlier run on the same unitig
 * file, or its structs -- so the reads tagged need not be the reads the blocks were phased from.  All integers, every result deterministic.
 * The tag table: uint32_t table[n_unitigs + 1], table[0] = 0; table[u] = block << 1 | hap with block >= 1 when unitig u is the branch of a bubble
 * that lies on haplotype A (hap 0) or B (hap 1) of that block, 0 when it is no branch of a tagged block.  Orientation never enters.
 *   bgr_blocks_tag_table: for every entry e of a block with size >= min_block, with r = bubbles[e.bubble] and h = (e.flags >> 1) & 1
 *   (BGR_BLOCK_HAP): |r.branch[h]| gets e.block << 1, |r.branch[1 - h]| gets e.block << 1 | 1; BGR_BLOCK_REVERSED and the ring flags do not matter.
 *   bgr_read_blocks_tags: per line of the file |hapA| gets block << 1 and |hapB| block << 1 | 1; every block of the file tags.
 *   Both write n_unitigs + 1 words to table_out and the number of non-zero entries to *n_tagged_out (may be null).  BGR_E_ARG with a message (the
 *   file form names the line) for: an id that is 0 or beyond n_unitigs; a block that is 0 or >= 2^31; |hapA| == |hapB|; a unitig that would receive
 *   two different tags (on lists from a run it cannot: a branch has one way in and one way out); an entry that names no bubble; a first line that is
 *   not exactly the header bgr_write_blocks writes; a line without ten tab-separated fields; a block, hapA or hapB that is not a decimal integer
 *   (an optional '-', then digits).  The last line may lack its newline; a file of the header alone tags nothing.  BGR_E_IO for a file that cannot
 *   be read.
 * The tag of a read: for a mapped row [off, id_1 .. id_n] the VOTES are table[|id_j|] for every j whose |id_j| (taken in 64 bits: INT32_MIN is
 * merely out of range) lies in 1 .. n_unitigs and whose entry is not 0.  No votes: all zeros.  Else block = the smallest block number among the
 * votes (independent of the strand), a and b = the votes of that block for A and for B, others = the votes for any other block.  An unmapped read,
 * and a row that is not wholly inside the launch's arena (results[i][0] + ints > bgr_aligner_arena_ints), give zeros.
 * bgr_aligner_haplotag_enable(a, table, n_rows) uploads the table to the aligner's device (n_rows must be n_unitigs + 1: BGR_E_ARG; BGR_E_NOMEM
 * with nothing left allocated); a null table switches the feature off and frees the copy.  An internal twin is BGR_E_ARG.
 * bgr_aligner_haplotags(a, n_reads, out): one kernel over the rows of the aligner's last launch (greedy or anchors mode), on the stream and the
 * buffers that ran it, and one copy; it blocks.  A 16-lane group per read: lane i takes id i of a pass of sixteen, one 4-byte gather per id, the
 * minimum and the three counts by reductions inside the sixteen lanes; no atomics, no LDS (bgreat_amd/csrc/haplotag_device.h).  BGR_E_ARG when no
 * table is enabled, after an exhaustive launch, when n_reads is not the launch's, for an internal twin.
 * GAF: with a table enabled, bgr_align_fasta_text with want_output 3 runs tagged instances of the GAF kernels; the line of a read with
 * block != 0 gains, behind NM:i:<n> and in front of the newline,
 *   \tPS:i:<block>\tHP:i:<h>\tha:i:<a>\thb:i:<b>\tho:i:<others>        h = 1 when a > b, 2 when b > a, 0 when they are equal
 * and a read with block == 0 keeps the exact line it has without a table.  Without a table the kernels launched are the untagged ones.
 * bgr_graph_haplotag_enable(g, table, n_rows) is sticky: the graph keeps a copy, null switches it off.  A bgr_align_all with the switch on is
 * BGR_E_ARG without bgr_run_options.gaf; with it every aligner of the run gets the table on its device and both routes write tagged lines (pieces
 * formatted on the host are tagged there, from the path ints the formatter holds).  notAligned, the counters and stdout do not change; the
 * refusals are those of gaf. */
typedef struct { uint32_t block, a, b, others; } bgr_read_tag;   /* 16 bytes */
int bgr_blocks_tag_table(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_block_entry* entries, uint64_t n_entries, uint64_t n_unitigs, uint64_t min_block,
                         uint32_t* table_out, uint64_t* n_tagged_out);
int bgr_read_blocks_tags(const char* path, uint64_t n_unitigs, uint32_t* table_out, uint64_t* n_tagged_out);
int bgr_aligner_haplotag_enable(bgr_aligner* a, const uint32_t* table, uint64_t n_rows);
int bgr_aligner_haplotags(bgr_aligner* a, uint64_t n_reads, bgr_read_tag* out);
int bgr_graph_haplotag_enable(bgr_graph* g, const uint32_t* table, uint64_t n_rows);
int bgr_graph_haplotag_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */

/* The pileup of a whole run (bgr_pileup_base above).  The switch is the graph's, as bgr_graph_links_enable is: bgr_graph_pileup_enable(g, 1) is
 * sticky (BGR_E_ARG on a graph with non-ACGT unitig characters or without a host blob), and every later bgr_align_all on the graph counts unitig
 * abundance and the pileup in every aligner of the run; the tables of all aligners and devices are summed (mod 2^32: the differences commute) when
 * the run ends and kept in the graph, guarded by the summed abundance: BGR_E_CAPACITY from the run when a unitig's reads reach 2^32.  With the switch
 * on, exhaustive mode is refused before any device work (BGR_E_ARG; the message names -b, --pileup and --depth); a run that fails (BGR_E_COMPACTION
 * too) leaves no totals; a run with the switch off leaves the last totals alone.  The run's files, counters and stdout are what they are without it.
 * bgr_graph_pileup delivers the totals (n_bases as above; *skipped, if not NULL, the rows that spelled no walk); BGR_E_ARG if there are none.
 * The writers (host code, deterministic bytes) write the graph's totals as text: bgr_write_pileup the line
 * "#unitig<TAB>pos<TAB>ref<TAB>depth<TAB>A<TAB>C<TAB>G<TAB>T<TAB>N", then one line per position where at least one of the six numbers is not zero,
 * in (unitig, pos) order, ids the 1-based ordinals of the paths file, pos 0-based, ref the unitig's character; bgr_write_depth, bedGraph-like,
 * "unitig<TAB>start<TAB>end<TAB>depth" per maximal run of equal non-zero depth inside a unitig, 0-based and half-open.  BGR_E_IO on a path they
 * cannot write.  Host memory: the graph keeps the summed table, 20 bytes per base (7.3 GiB on the chr1-scale graph), until the next run with the
 * switch on or bgr_graph_destroy; while a run ends, each further aligner's table passes through a second buffer of that size before it is added, so the
 * peak is 40 bytes per base; the writers convert unitig by unitig and add nothing to that, bgr_graph_pileup fills the caller's 24 bytes per base. */
int bgr_graph_pileup_enable(bgr_graph* g, uint32_t on);
int bgr_graph_pileup_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_pileup(const bgr_graph* g, bgr_pileup_base* out, uint64_t n_bases, uint64_t* skipped);
int bgr_write_pileup(const char* path, const bgr_graph* g);
int bgr_write_depth(const char* path, const bgr_graph* g);

/* The SNV sites of a whole run (bgr_variant_site above).  bgr_graph_variants_enable(g, &params) is a sticky switch on the graph like
 * bgr_graph_links_enable (NULL switches it off; BGR_E_ARG for thresholds out of range, non-ACGT unitig characters, no host blob): every later
 * bgr_align_all counts unitig abundance and the pileup in every aligner.  When the run collects its aligners, the first table becomes the run's --
 * its device buffer is moved, nothing is allocated -- and every further aligner's table is added into it on the device (bgr_aligner_pileup_add's two
 * ways); at the run's end the summed abundance guards it (BGR_E_CAPACITY), the five launches run once and the graph keeps the sites and the
 * thresholds they were called with.  No table crosses to the host unless bgr_graph_pileup_enable is on as well, in which case its totals are gathered
 * exactly as without this switch, in addition.  Refusals and failed runs as the pileup's (exhaustive mode: BGR_E_ARG, the message names --vcf).
 * bgr_graph_variants: the sites of the last such run (*n always; BGR_E_CAPACITY when cap is smaller; BGR_E_ARG when there are none);
 * bgr_graph_variants_params: the thresholds of those sites.
 * bgr_write_vcf (host code, deterministic bytes; needs the graph's host blob for the reference letters) writes `sites` -- in (unitig, pos) order, as
 * delivered -- as VCF 4.2: "##fileformat=VCFv4.2", "##source=bgreat-mi355x", "##bgreat_thresholds=<min_depth=..,min_alt=..,min_af_ppm=..>", the INFO
 * lines of DP, AD and NN, one "##contig=<ID=id,length=len>" per unitig that carries a site, the "#CHROM POS ID REF ALT QUAL FILTER INFO" line, and per
 * site: id, pos + 1, ".", the unitig's letter, the passing alleles (by count descending, ties A < C < G < T) comma-separated, ".", "PASS",
 * "DP=depth;AD=ref,alt1,..;NN=n" with ref = depth - (a + c + g + t + n).  BGR_E_ARG for a site outside the graph, out of order or without a passing allele.
 * bgr_parse_af_ppm: an allele fraction written as a decimal ("0", "1", "0.2", "0.000001": digits, at most six decimals, value <= 1) -> parts per
 * million, exactly; BGR_E_ARG for anything else. */
int bgr_graph_variants_enable(bgr_graph* g, const bgr_variant_params* params);
int bgr_graph_variants_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_variants(const bgr_graph* g, bgr_variant_site* out, uint64_t cap, uint64_t* n);
int bgr_graph_variants_params(const bgr_graph* g, bgr_variant_params* out);
int bgr_write_vcf(const char* path, const bgr_graph* g, const bgr_variant_params* params, const bgr_variant_site* sites, uint64_t n);
int bgr_parse_af_ppm(const char* text, uint32_t* ppm);

/* Strands in a whole run (the definitions stand at bgr_aligner_pileup_strands_enable).  bgr_graph_pileup_strands_enable(g, 1) is sticky and switches
 * bgr_graph_pileup_enable on as well (0 leaves that on): every aligner of a later bgr_align_all also counts the forward table, and the forward totals
 * are gathered on the host next to the totals -- HOST MEMORY DOUBLES: 40 bytes per base kept in the graph, 60 at the peak while a run ends.
 * bgr_graph_pileup_forward delivers them (BGR_E_ARG when the last successful run had the switch off); bgr_write_pileup_strands writes
 * bgr_write_pileup's lines -- the same selection: any of the six TOTAL numbers non-zero -- with the six forward numbers appended, under the header
 * "#unitig pos ref depth A C G T N depth+ A+ C+ G+ T+ N+" (tab-separated).
 * bgr_graph_variants_strands_enable(g, &params) is bgr_graph_variants_enable with the strand filter (NULL switches both off; a later
 * bgr_graph_variants_enable switches the filter and the forward table off again): the forward table travels with the run's table -- moved from the
 * first aligner, added on the device from the others, staged across devices -- and the run's end keeps 64-byte records: bgr_graph_variant_strand_sites
 * (as bgr_graph_variants; BGR_E_ARG when the last run had no strands).  bgr_graph_variants then delivers the same sites without the forward numbers.
 * bgr_write_vcf_strands is bgr_write_vcf for such records: the thresholds line ends in ",min_alt_strand=..>", the INFO lines of ADF and ADR follow
 * AD's, ALT lists the alleles that pass the strand filter too, and INFO is "DP=..;AD=..;ADF=..;ADR=..;NN=.." with ADF = forward ref, then the forward
 * count of each ALT, forward ref = fdepth - (fa + fc + fg + ft + fn), and ADR = AD - ADF element by element.  BGR_E_ARG also for a record whose
 * forward numbers do not fit its totals. */
int bgr_graph_pileup_strands_enable(bgr_graph* g, uint32_t on);
int bgr_graph_pileup_strands_enabled(const bgr_graph* g);   /* the switch as it stands: 1 or 0 */
int bgr_graph_pileup_forward(const bgr_graph* g, bgr_pileup_base* out, uint64_t n_bases);
int bgr_graph_variants_strands_enable(bgr_graph* g, const bgr_variant_strand_params* params);
int bgr_graph_variant_strand_sites(const bgr_graph* g, bgr_variant_strand_site* out, uint64_t cap, uint64_t* n);
int bgr_write_pileup_strands(const char* path, const bgr_graph* g);
int bgr_write_vcf_strands(const char* path, const bgr_graph* g, const bgr_variant_strand_params* params, const bgr_variant_strand_site* sites, uint64_t n);
int bgr_parse_min_alt_strand(const char* text, uint32_t* out);   /* the CLI's --min-alt-strand: digits only, at most nine; BGR_E_ARG for anything else */

/* The CPUs next to a device (the `local_cpulist` of its PCI function in sysfs, e.g. "0-63,128-191"): threads that feed a GPU and the
 * page-locked memory they allocate belong on its NUMA node.  BGR_E_IO when the platform does not say. */
int bgr_device_local_cpus(int device, char* cpulist_out, uint64_t cap);

/* Device memory for callers of bgr_align_device that have no HIP runtime of their own (a cgo / ctypes host parks its batches in HBM
 * through these three); any other device pointer of the same process works as well.  upload / download are blocking copies. */
int bgr_device_alloc(int device, uint64_t bytes, void** out);
int bgr_device_free(int device, void* p);
int bgr_device_upload(int device, void* dst_device, const void* src_host, uint64_t bytes);
int bgr_device_download(int device, void* dst_host, const void* src_device, uint64_t bytes);

/* Page-locked host memory for batches handed to bgr_align_batch (faster H2D/D2H); plain memory works too. */
int bgr_host_alloc(uint64_t bytes, void** out);
int bgr_host_free(void* p);

#ifdef __cplusplus
}
#endif
#endif
