// capi_text.hip -- the C-ABI's text route: FASTA / FASTQ bytes in, record bytes out (text_kernels.h has the kernels' launch interface, text_epochs.h
// the book of their epochs, tickets and info blocks; the state is TextRoute in capi_internal.h).  bgr_align_fasta_text as a row of named steps,
// bgr_aligner_fetch_text, and the stages through which a caller uploads the next piece ahead of its call (bgr_text_stage_*).  What the CLI runs for
// every piece of every read file: default output, -c, --gaf, --haplotag, --cs (the switches of the cs:Z: field are here too).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "text_kernels.h"

namespace {

using bgr::TextEpochs;

double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int launched(hipError_t e, const char* what) { return e == hipSuccess ? BGR_OK : fail(BGR_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

// What the steps of one bgr_align_fasta_text hand to each other (the aligner's TextRoute has what outlives the call)
struct TextCall {
    bgr_aligner* a;
    const bgr_params* p;
    bgr_text_batch* b;
    uint32_t nbytes = 0, rec_lines = 0;   // the piece's bytes; lines per record of a FASTQ piece (0: FASTA, records start at '>' lines)
    uint32_t R_cap = 0, R = 0, n_acc = 0, bases = 0, max_len = 0;   // room for records; records found; accepted ones, their bases, the longest
    uint32_t* info = nullptr;             // the piece's info block on the device
    uint32_t h[TXT_INFO_WORDS];           // ... and on the host: as the parse launch left it, then as the format step did
    uint64_t pcap_dev = 0, ncap_dev = 0;  // default output: the capacities the format launch wrote below
    uint32_t format_runs = 0;             // times the format step has run
    double tw = 0;                        // BGREAT_TIMING: the wall clock at the last mark
    void lap(int i) { const double t = wall_now(); a->text.phase_s[i] += t - tw; tw = t; }
};
// what a step returns besides BGR_OK (go on) and an error: the call has ended well in it; the format step has to run again
const int kCallDone = 1, kRunAgain = 2;

// TXT_INFO_WORDS u32 behind cursor / counters / CSR total -- two such blocks, taken in turn (text_epochs.h)
uint32_t* info_block(const bgr_aligner* a, uint32_t which) { return reinterpret_cast<uint32_t*>(a->launch.small.as<char>() + bgr::kSmallTextInfo + bgr::kSmallTextInfoBytes * which); }
static_assert(TXT_INFO_WORDS * 4 == bgr::kSmallTextInfoBytes, "two info blocks at small + kSmallTextInfo");
// tickets and chains of the two one-launch kernels (text_kernels.hip) in TextRoute::state: never cleared between launches -- every launch gets a fresh epoch
uint32_t* tickets_of(const TextRoute& t) { return t.state.as<uint32_t>(); }
uint64_t* chains_of(const TextRoute& t) { return reinterpret_cast<uint64_t*>(t.state.as<char>() + 64); }

// ---- bgr_aligner_fetch_text ---------------------------------------------------------------------------------------------------------
// The write launch of the piece in the buffers, by its kind of output: the streams into pout / nout from the offsets its sizes were scanned into.
hipError_t write_gaf(const bgr_aligner* a, const TextRoute& t) {
    return bgr::launch_text_gaf_write(a->dg, t.text, (t.view ? a->launch.rows_view : a->launch.results).as<uint2>(), a->launch.arena.as<int32_t>(), t.rec.as<uint4>(), t.accrec.as<uint32_t>(), (uint32_t)t.n_acc, t.poff.as<uint32_t>(),
                                      t.noff.as<uint32_t>(), t.psz.as<uint32_t>(), t.idx.as<uint32_t>(), t.gaf.as<uint4>(), t.pout.as<uint8_t>(), t.nout.as<uint8_t>(),
                                      t.tagged ? t.tags.as<uint4>() : nullptr, t.with_cs ? t.cs.as<uint32_t>() : nullptr, a->stream);
}
hipError_t write_corrected(const bgr_aligner* a, const TextRoute& t) {
    return bgr::launch_text_correct_write(a->dg, t.text, a->launch.results.as<uint2>(), a->launch.arena.as<int32_t>(), t.rec.as<uint4>(), t.accrec.as<uint32_t>(), (uint32_t)t.n_acc,
                                          t.poff.as<uint32_t>(), t.noff.as<uint32_t>(), t.idx.as<uint32_t>(), t.pout.as<uint8_t>(), t.nout.as<uint8_t>(), a->stream);
}
hipError_t write_records(const bgr_aligner* a, const TextRoute& t) {
    return bgr::launch_text_write(t.text, a->launch.results.as<uint2>(), a->launch.arena.as<int32_t>(), t.rec.as<uint4>(), t.accrec.as<uint32_t>(), (uint32_t)t.n_acc, t.poff.as<uint32_t>(),
                                  t.noff.as<uint32_t>(), t.pout.as<uint8_t>(), t.nout.as<uint8_t>(), a->stream);
}

// Reads the sizes of the two streams of the last piece (TextRoute::pbytes / nbytes) and, where the format launch has not written them already, the
// offsets; leaves the sizes in the batch and, with want_output and room for them, the bytes in the caller's buffers (the stream waited for).
int fetch_text_impl(bgr_aligner* a, bgr_text_batch* b) {
    TextRoute& t = a->text;
    b->paths_bytes = t.pbytes;
    b->notaligned_bytes = t.nbytes;
    if (!b->want_output || t.n_acc == 0) return BGR_OK;
    if (t.pbytes > b->paths_cap || t.nbytes > b->notaligned_cap || (t.pbytes && !b->paths_out) || (t.nbytes && !b->notaligned_out))
        return fail(BGR_E_CAPACITY, "bgr_align_fasta_text: output buffer too small (paths_bytes / notaligned_bytes say what is needed; bgr_aligner_fetch_text)");
    if (!t.written) {   // (correction mode; GAF; streams larger than the buffers the format launch wrote into; a second fetch)
        HIP_TRY(t.pout.ensure(t.pbytes + 64));
        HIP_TRY(t.nout.ensure(t.nbytes + 64));
        const hipError_t e = t.want == 3 ? write_gaf(a, t) : t.want == 2 ? write_corrected(a, t) : write_records(a, t);
        if (e != hipSuccess) return launched(e, "text write launch");
        t.written = true;
    }
    if (t.pbytes) HIP_TRY(hipMemcpyAsync(b->paths_out, t.pout.p, t.pbytes, hipMemcpyDeviceToHost, a->stream));
    if (t.nbytes) HIP_TRY(hipMemcpyAsync(b->notaligned_out, t.nout.p, t.nbytes, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    return BGR_OK;
}

// ---- the stages -------------------------------------------------------------------------------------------------------------------
// The parts laid end to end into the stage's buffer on its copy stream, zero padded, the "it has arrived" event behind them (`who`: the public function)
int stage_upload(bgr_text_stage* s, const std::string& who, uint32_t n_parts, const char* const* parts, const uint64_t* part_bytes) {
    uint64_t bytes = 0;
    for (uint32_t i = 0; i < n_parts; ++i) { if (part_bytes[i] && !parts[i]) return fail(BGR_E_ARG, who + ": null part"); bytes += part_bytes[i]; }
    if (bytes >= (1ull << 31)) return fail(BGR_E_ARG, who + ": piece of 2 GiB or more; cut it");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));  // (a piece still on its way: the buffer may grow, i.e. move)
    s->settle();
    HIP_TRY(s->buf.ensure(bytes + 128));
    if (s->timing) { HIP_TRY(hipEventRecord(s->ev0, s->stream)); s->pending = true; }
    HIP_TRY(hipMemsetAsync(s->buf.as<char>() + (bytes & ~63ull), 0, 128, s->stream));   // (from an aligned address: one fill; the copies below lay the text over its start)
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_parts; ++i) {
        if (part_bytes[i]) HIP_TRY(hipMemcpyAsync(s->buf.as<char>() + at, parts[i], part_bytes[i], hipMemcpyHostToDevice, s->stream));
        at += part_bytes[i];
    }
    HIP_TRY(hipEventRecord(s->ev, s->stream));
    s->bytes = bytes;
    return BGR_OK;
}

// ---- the steps of bgr_align_fasta_text ------------------------------------------------------------------------------------------------
// Reads the caller's three arguments and the graph's header; leaves nothing behind: BGR_OK, or the refusal of a call this route does not take.
int check_text_call(const bgr_aligner* a, const bgr_params* p, const bgr_text_batch* b) {
    if (!a || !p || !b) return fail(BGR_E_ARG, "bgr_align_fasta_text: null argument");
    if (b->struct_size != sizeof(bgr_text_batch)) return fail(BGR_E_ARG, "bgr_align_fasta_text: bgr_text_batch.struct_size is not this library's sizeof(bgr_text_batch): the caller was built against another header (zero the struct, set struct_size)");
    if (b->text_bytes && !b->text && !b->stage) return fail(BGR_E_ARG, "bgr_align_fasta_text: null argument");
    if (b->record_info_out && b->text_bytes >= (1ull << 30)) return fail(BGR_E_ARG, "bgr_align_fasta_text: record_info_out holds a read's length in 30 bits: pieces below 2^30 bytes");
    if (b->text_bytes >= (1ull << 31)) return fail(BGR_E_ARG, "bgr_align_fasta_text: piece of 2 GiB or more; cut it");
    if (b->want_output > 3) return fail(BGR_E_ARG, "bgr_align_fasta_text: want_output must be 0, 1, 2 or 3");
    if (b->fastq > 2) return fail(BGR_E_ARG, "bgr_align_fasta_text: fastq must be 0, 1 (four-line records) or 2 (header and read lines only)");
    if (b->fastq && b->text_bytes && b->text && b->text[b->text_bytes - 1] != '\n' && !b->stage)
        return fail(BGR_E_ARG, "bgr_align_fasta_text: a FASTQ piece holds whole four-line records and ends with a newline");
    if (b->want_output == 2 && (a->graph->header.has_exc || p->mode == BGR_MODE_EXHAUSTIVE))
        return fail(BGR_E_ARG, "bgr_align_fasta_text: correction on the device needs a graph of ACGT-only unitigs and greedy mode (format such a run on the host)");
    if (b->want_output == 3 && (a->graph->header.has_exc || (p->mode == BGR_MODE_EXHAUSTIVE && !a->sh->exhaustive_paths)))
        return fail(BGR_E_ARG, "bgr_align_fasta_text: GAF output needs a graph of ACGT-only unitigs (a path read backwards does not spell the reverse complement on one with other characters) and a greedy mode");
    // (the GAF lines of an exhaustive launch, bgr_aligner_exhaustive_paths_enable: the record info is what the caller prints the -b progress blocks from)
    const bool info_with_gaf = b->want_output == 3 && p->mode == BGR_MODE_EXHAUSTIVE;
    if (b->record_info_out && ((b->want_output >= 2 && !info_with_gaf) || b->record_info_cap < b->text_bytes / 24 + 1024))
        return fail(BGR_E_ARG, "bgr_align_fasta_text: record_info_out needs room for text_bytes / 24 + 1024 words and is not available in correction mode or with GAF output");
    return BGR_OK;
}

// 1. Reads the batch's text or stage; leaves the piece in HBM, zero padded, and TextRoute::text pointing at it: uploaded ahead of this call by a stage
// (bgr_text_stage_upload, a copy stream of its own: the aligner's stream waits for its event), or copied now into TextRoute::in.
int place_piece(TextCall& c) {
    bgr_aligner* a = c.a;
    TextRoute& t = a->text;
    const bgr_text_batch* b = c.b;
    if (b->stage) {
        if (b->stage->device != a->device || b->stage->bytes != b->text_bytes) return fail(BGR_E_ARG, "bgr_align_fasta_text: the stage holds another piece / lives on another device");
        HIP_TRY(hipStreamWaitEvent(a->stream, b->stage->ev, 0));
        t.text = b->stage->buf.as<const uint8_t>();
        return BGR_OK;
    }
    if (!b->text) return fail(BGR_E_ARG, "bgr_align_fasta_text: null text");
    HIP_TRY(t.in.ensure((uint64_t)c.nbytes + 128));
    HIP_TRY(hipMemsetAsync(t.in.as<char>() + (c.nbytes & ~63ull), 0, 128, a->stream));   // (64 zero bytes behind the piece at least; from an aligned address: ONE fill, and the copy below lays the text over its start)
    HIP_TRY(hipMemcpyAsync(t.in.p, b->text, c.nbytes, hipMemcpyHostToDevice, a->stream));
    t.text = t.in.as<const uint8_t>();
    return BGR_OK;
}

// 2a. Reads the piece's size; leaves R_cap -- room for one record per 24 bytes of text (a sequencing read with its header is several times that): a
// piece with more record starts goes to the host parser --, every buffer of the records and the scans at that size, and the chain state with the
// epochs of this call reserved: zeroed when it is new or the call could run out of them (text_epochs.h).
int size_text_buffers(TextCall& c) {
    TextRoute& t = c.a->text;
    c.R_cap = c.nbytes / 24 + 1024;
    const uint64_t chain_words = std::max<uint64_t>(3ull * bgr::text_tiles(c.nbytes), 2ull * bgr::format_tiles(c.R_cap));
    const size_t had = t.state.cap;
    HIP_TRY(t.state.ensure(64 + chain_words * 8));
    const bool fresh = t.state.cap != had;
    if (t.epochs.begin_call(fresh, fresh ? (uint32_t)bgr::opt("test.text_epoch") : 0u)) {   // (the hook: 0 but in tests)
        const hipError_t e = hipMemsetAsync(t.state.p, 0, t.state.cap, c.a->stream);
        if (e != hipSuccess) { t.epochs.zero_failed(); return launched(e, "bgr_align_fasta_text: clearing the chain state"); }
    }
    HIP_TRY(t.sums.ensure((2ull * bgr::scan_tiles(c.R_cap) + 16) * 4));   // (correction mode's scans)
    for (DevBuf* d : {&t.idx, &t.accrec, &t.accsrc, &t.psz, &t.nsz, &t.poff, &t.noff}) HIP_TRY(d->ensure(((uint64_t)c.R_cap + 4) * 4));
    HIP_TRY(t.rec.ensure(((uint64_t)c.R_cap + 1) * 16));
    HIP_TRY(t.offs.ensure(((uint64_t)c.R_cap + 2) * 8));
    return BGR_OK;
}

// 2b. Reads the piece; leaves its records on the device -- starts, extents, shape, accept test; the accepted ones compacted in input order -- and their
// counts in the batch and the call: n_records, irregular, n_accepted, bases, max_len.  The launch also clears the info block of the NEXT piece and the
// mapping launch's cursor; the flip is committed behind it.  kCallDone: nothing for the mapping kernels (the host parser decides, or nothing was kept).
int parse_piece(TextCall& c) {
    bgr_aligner* a = c.a;
    TextRoute& t = a->text;
    bgr_text_batch* b = c.b;
    c.info = info_block(a, t.epochs.block());
    uint32_t* info_next = info_block(a, t.epochs.next_block());
    const uint32_t epoch = t.epochs.next_epoch();
    if (!epoch) return fail(BGR_E_INTERNAL, "bgr_align_fasta_text: more launches than the epochs reserved for a call");
    const hipError_t e = bgr::launch_text_parse(t.text, c.nbytes, c.rec_lines, a->dg.k, tickets_of(t), t.epochs.ticket_base(TextEpochs::kParse), epoch, chains_of(t), t.rec.as<uint4>(),
                                                t.idx.as<uint32_t>(), t.accrec.as<uint32_t>(), t.accsrc.as<uint32_t>(), t.offs.as<uint64_t>(), c.info, c.R_cap, a->launch.small.as<uint32_t>(),
                                                bgr::kCurWords, info_next, TXT_INFO_WORDS, a->stream);
    if (e != hipSuccess) return launched(e, "text record launches");
    t.epochs.commit_flip();
    t.epochs.took_tickets(TextEpochs::kParse, bgr::text_tiles(c.nbytes));   // (as many tickets as workgroups will take)
    HIP_TRY(hipMemcpyAsync(c.h, c.info, sizeof(c.h), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    c.lap(0);
    c.R = c.h[TXT_INFO_N_REC];
    b->n_records = c.R;
    if (c.R == 0 || c.R > c.R_cap) { b->irregular = 1; return kCallDone; }  // no record start in the bytes, or far more than a read file has: the host parser decides
    c.lap(1);
    if (c.h[TXT_INFO_IRREGULAR]) { b->irregular = 1; return kCallDone; }
    c.n_acc = c.h[TXT_INFO_N_ACC]; c.bases = c.h[TXT_INFO_BASES]; c.max_len = c.h[TXT_INFO_MAX_LEN];
    b->n_accepted = c.n_acc;
    if (c.n_acc == 0) {
        if (b->record_info_out) memset(b->record_info_out, 0, (size_t)c.R * 4);  // (nothing kept: every record a dropped one)
        return kCallDone;
    }
    return BGR_OK;
}

// 4. The sizes launch of the wanted output, one function each: reads the mapping launch's results and the records; leaves the sizes of the records in
// psz / nsz (default output: the offsets, the totals and, below the capacities, the bytes at once) and the first read whose path spells no walk in
// the info block's BUG word (idx is free again behind the compaction: it takes the lengths of the names / of the corrected reads).
int gaf_sizes(TextCall& c) {
    bgr_aligner* a = c.a;
    TextRoute& t = a->text;
    HIP_TRY(t.gaf.ensure(((uint64_t)c.n_acc + 1) * 16));
    t.tagged = a->tag.table.p != nullptr;   // (an aligner with a tag table: the tagged instances of both GAF kernels)
    if (t.tagged) HIP_TRY(t.tags.ensure(((uint64_t)c.n_acc + 1) * 16));
    t.with_cs = a->gaf_cs;                 // (bgr_aligner_gaf_cs_enable: the instances whose lines end in the cs:Z: field)
    if (t.with_cs) HIP_TRY(t.cs.ensure(((uint64_t)c.n_acc + 1) * 4));
    // an exhaustive launch (bgr_aligner_exhaustive_paths_enable): both GAF kernels read its rows without their end offset -- the view, made here every time this
    // step runs (the second time, behind a launch that had to be settled, from the final rows)
    t.view = c.p->mode == BGR_MODE_EXHAUSTIVE;
    if (t.view) { if (const int rc = view_launch(a, c.n_acc, a->last_arena_cap); rc != BGR_OK) return rc; }
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c.info + TXT_INFO_BUG), -1, 1, a->stream));
    return launched(bgr::launch_text_gaf_sizes(a->dg, t.text, (t.view ? a->launch.rows_view : a->launch.results).as<uint2>(), a->launch.arena.as<int32_t>(), t.rec.as<uint4>(), t.accrec.as<uint32_t>(), c.n_acc, t.psz.as<uint32_t>(),
                                               t.nsz.as<uint32_t>(), t.idx.as<uint32_t>(), t.gaf.as<uint4>(), c.info + TXT_INFO_BUG, t.tagged ? a->tag.table.as<uint32_t>() : nullptr,
                                               t.tags.as<uint4>(), t.with_cs ? t.cs.as<uint32_t>() : nullptr, a->stream),
                    "text size launches");
}
int correct_sizes(TextCall& c) {
    bgr_aligner* a = c.a;
    TextRoute& t = a->text;
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c.info + TXT_INFO_BUG), -1, 1, a->stream));
    return launched(bgr::launch_text_correct_sizes(a->dg, a->launch.results.as<uint2>(), a->launch.arena.as<int32_t>(), t.rec.as<uint4>(), t.accrec.as<uint32_t>(), c.n_acc, t.psz.as<uint32_t>(),
                                                   t.nsz.as<uint32_t>(), t.idx.as<uint32_t>(), c.info + TXT_INFO_BUG, a->stream),
                    "text size launches");
}
// sizes, offsets and bytes in one launch, into device buffers of the caller's capacities (at most twice the piece + 1 MB each: a piece whose
// streams need more -- paths of very many unitigs -- is written by bgr_text_write_kernel from the offsets once the totals are known)
int format_streams(TextCall& c) {
    bgr_aligner* a = c.a;
    TextRoute& t = a->text;
    c.pcap_dev = c.b->paths_out ? std::min<uint64_t>(c.b->paths_cap, 2ull * c.nbytes + (1ull << 20)) : 0;
    c.ncap_dev = c.b->notaligned_out ? std::min<uint64_t>(c.b->notaligned_cap, 2ull * c.nbytes + (1ull << 20)) : 0;
    HIP_TRY(t.pout.ensure(c.pcap_dev + 64));
    HIP_TRY(t.nout.ensure(c.ncap_dev + 64));
    const uint32_t epoch = t.epochs.next_epoch();
    if (!epoch) return fail(BGR_E_INTERNAL, "bgr_align_fasta_text: more launches than the epochs reserved for a call");
    const hipError_t e = bgr::launch_text_format(t.text, a->launch.results.as<uint2>(), a->launch.arena.as<int32_t>(), t.rec.as<uint4>(), t.accrec.as<uint32_t>(), c.n_acc, tickets_of(t) + 1,
                                                 t.epochs.ticket_base(TextEpochs::kFormat), epoch, chains_of(t), t.poff.as<uint32_t>(), t.noff.as<uint32_t>(), t.pout.as<uint8_t>(),
                                                 t.nout.as<uint8_t>(), c.pcap_dev, c.ncap_dev, c.info, a->stream);
    if (c.n_acc && e == hipSuccess) t.epochs.took_tickets(TextEpochs::kFormat, bgr::format_tiles(c.n_acc));   // (as many tickets as workgroups ran: launch_text_format launches nothing for zero reads)
    return launched(e, "text size launches");
}

// Behind the wait for the mapping launch, its cursor block in `cur`: the launch settled (arena flag; exhaustive mode: reads the last pass handed back
// are mapped again, settle_launch).  BGR_OK: the results were final when the kernels behind the launch read them; kRunAgain: they were not
int settle_text_launch(bgr_aligner* a, uint32_t* cur) {
    const bool handed_back = a->deep.open && cur[bgr::list_word(bgr::List::kRetry)] != 0;
    const bool counts = a->deep_count.open;
    const int rc = settle_launch(a, cur);
    // (bgr_aligner_exhaustive_paths_enable: the counting kernels, queued by settle_launch, read the piece -- the pileup its characters --, and the caller's
    // stage may take the next piece once this call returns: they have run when it does)
    if (rc == BGR_OK && counts) HIP_TRY(wait_stream(a));
    return rc != BGR_OK ? rc : handed_back ? kRunAgain : BGR_OK;
}

// 4. Everything behind the mapping launch reads its results.  In exhaustive mode those are final only once the launch is settled (reads the last pass
// handed back for a larger table are mapped again: settle_launch) -- which hardly ever happens: so the kernels here are enqueued at once, the cursor
// comes back with the wait this call makes anyway, and only a launch that did hand reads back is settled and this step run AGAIN (a wait between the
// mapping launch and them cost -b a fifth of its end-to-end rate).  Reads the results, the records, n_acc; leaves the record info in the caller's
// buffer, the sizes and offsets of the wanted output on the device and the piece's info block in c.h.  BGR_OK: settled, all of that final; kRunAgain:
// settled, but made from results that were not final; kCallDone: settled, and a call without output ends here.
int format_once(TextCall& c) {
    bgr_aligner* a = c.a;
    TextRoute& t = a->text;
    bgr_text_batch* b = c.b;
    if (b->record_info_out) {  // what became of every record (the -b progress blocks of the caller), on its way to the host behind the mapping launch
        HIP_TRY(t.info.ensure((uint64_t)c.R * 4));
        const uint32_t* idx = t.idx.as<uint32_t>();
        if (b->want_output == 3) {   // (the GAF sizes launch below takes idx for the lengths of the names: this step may run again and needs it as it was)
            const uint64_t bytes = ((uint64_t)c.R_cap + 4) * 4;
            HIP_TRY(t.idx_kept.ensure(bytes));
            if (c.format_runs == 0) HIP_TRY(hipMemcpyAsync(t.idx_kept.p, t.idx.p, bytes, hipMemcpyDeviceToDevice, a->stream));
            idx = t.idx_kept.as<uint32_t>();
        }
        ++c.format_runs;
        const hipError_t e = bgr::launch_text_record_info(t.rec.as<uint4>(), idx, a->launch.results.as<uint2>(), c.R, t.info.as<uint32_t>(), a->stream);
        if (e != hipSuccess) return launched(e, "record info launch");
        HIP_TRY(hipMemcpyAsync(b->record_info_out, t.info.p, (size_t)c.R * 4, hipMemcpyDeviceToHost, a->stream));
    }
    if (!b->want_output) {  // counters only: the launch still has to be settled
        uint32_t cur[bgr::kCurWords];
        HIP_TRY(hipMemcpyAsync(cur, a->launch.small.p, sizeof(cur), hipMemcpyDeviceToHost, a->stream));
        HIP_TRY(wait_stream(a));
        const int rc = settle_text_launch(a, cur);
        if (rc == kRunAgain && b->record_info_out) return kRunAgain;  // (the record info was made from results that were not final)
        return rc == BGR_OK || rc == kRunAgain ? kCallDone : rc;
    }
    int rc = b->want_output == 3 ? gaf_sizes(c) : b->want_output == 2 ? correct_sizes(c) : format_streams(c);
    if (rc != BGR_OK) return rc;
    if (b->want_output >= 2) {
        rc = launched(bgr::launch_scan2_u32(t.psz.as<uint32_t>(), t.nsz.as<uint32_t>(), t.poff.as<uint32_t>(), t.noff.as<uint32_t>(), c.n_acc, nullptr, t.sums.as<uint32_t>(),
                                            c.info + TXT_INFO_PBYTES, c.info + TXT_INFO_NBYTES, a->stream),
                      "text size launches");
        if (rc != BGR_OK) return rc;
    }
    uint32_t all[bgr::kSmallBytes / 4];   // the cursor block (at its start) and the info block lie in the same `small` buffer: one copy
    HIP_TRY(hipMemcpyAsync(all, a->launch.small.p, sizeof(all), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    memcpy(c.h, all + (c.info - a->launch.small.as<uint32_t>()), sizeof(c.h));
    c.lap(2);
    return settle_text_launch(a, all);   // (kRunAgain: sizes and offsets once more, from the final results)
}

// 5. Reads the info block as the last format step left it; leaves the sizes of the two streams in TextRoute and the batch, and with want_output
// the bytes in the caller's buffers (fetch_text_impl) -- or irregular = 2 for a path that does not spell a walk: the reference prints "bug compaction"
// and exits (aligner.cpp:280-283); the caller reproduces that on the host.
int finish_text_call(TextCall& c) {
    TextRoute& t = c.a->text;
    if (c.b->want_output >= 2 && c.h[TXT_INFO_BUG] != 0xFFFFFFFFu) {
        c.b->irregular = 2;
        t.n_acc = 0;
        return BGR_OK;
    }
    t.pbytes = c.h[TXT_INFO_PBYTES];
    t.nbytes = c.h[TXT_INFO_NBYTES];
    t.written = c.b->want_output == 1 && t.pbytes <= c.pcap_dev && t.nbytes <= c.ncap_dev;   // (every workgroup's stretch ended below the capacities)
    const int frc = fetch_text_impl(c.a, c.b);
    c.lap(3);
    t.phase_s[4] += 1;
    return frc;
}

}  // namespace

int bgr_aligner_gaf_cs_enable(bgr_aligner* a, int on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_gaf_cs_enable: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_gaf_cs_enable: an internal twin (the switch belongs to the aligner it was made for)");
    a->gaf_cs = on != 0;   // (read when a piece's sizes are launched; the write launch follows what that launch was)
    return BGR_OK;
}

int bgr_graph_gaf_cs_enable(bgr_graph* g, int on) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_gaf_cs_enable: null graph");
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->gaf_cs_on = on != 0;
    return BGR_OK;
}

int bgr_graph_gaf_cs_enabled(const bgr_graph* g) { return g && g->gaf_cs_on ? 1 : 0; }

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
    return stage_upload(s, "bgr_text_stage_upload", 1, &text, &bytes);
}

int bgr_text_stage_upload_parts(bgr_text_stage* s, uint32_t n_parts, const char* const* parts, const uint64_t* part_bytes) {
    if (!s || (n_parts && (!parts || !part_bytes))) return fail(BGR_E_ARG, "bgr_text_stage_upload_parts: null argument");
    return stage_upload(s, "bgr_text_stage_upload_parts", n_parts, parts, part_bytes);
}

int bgr_align_fasta_text(bgr_aligner* a, const bgr_params* p, bgr_text_batch* b) {
    int rc = check_text_call(a, p, b);
    if (rc != BGR_OK) return rc;
    TextCall c{a, p, b};
    c.tw = wall_now();
    c.rec_lines = b->fastq == 2 ? 2u : b->fastq ? 4u : 0u;
    TextRoute& t = a->text;
    t.want = b->want_output;
    b->irregular = 0;
    b->n_records = b->n_accepted = b->paths_bytes = b->notaligned_bytes = 0;
    forget_launch(a);
    t.n_acc = t.pbytes = t.nbytes = 0;
    if (b->text_bytes == 0) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    c.nbytes = (uint32_t)b->text_bytes;
    if ((rc = place_piece(c)) != BGR_OK) return rc;
    if ((rc = size_text_buffers(c)) != BGR_OK) return rc;
    if ((rc = parse_piece(c)) != BGR_OK) return rc == kCallDone ? BGR_OK : rc;
    // 3. the mapping launch, its reads where they lie in the text (planes by the pre-pass, or -- greedy mode -- staged by the mapping kernels themselves)
    if (p->mode == BGR_MODE_EXHAUSTIVE && !bgr::opt("test.keep_rows")) {
        // The last pass writes no row for a read it hands back (exhaustive_kernels.hip), and format_once reads the rows before the launch is settled: until
        // then they say "no path", not what the buffer held (a new aligner's first piece, a buffer that grew: a row of anything sends the format kernel anywhere)
        HIP_TRY(a->launch.results.ensure((uint64_t)c.n_acc * 8));
        HIP_TRY(hipMemsetAsync(a->launch.results.p, 0, (uint64_t)c.n_acc * 8, a->stream));
    }
    rc = align_device_impl(a, p, t.text, t.offs.p, c.n_acc, c.bases, c.max_len, false, t.accsrc.p, c.nbytes, true);
    if (rc != BGR_OK) return rc;
    forget_launch(a);  // (bgr_aligner_fetch has no host read_offsets to pair its rows with: the text form hands out text)
    t.n_acc = c.n_acc;
    t.written = false;
    rc = kRunAgain;
    for (uint32_t run = 0; run < bgr::kTextFormatRuns && rc == kRunAgain; ++run) {   // (a second time only behind a launch that had to be settled: text_epochs.h reserves the epochs of both)
        rc = format_once(c);
    }
    if (rc == kRunAgain) return fail(BGR_E_INTERNAL, "bgr_align_fasta_text: a settled launch handed reads back");
    if (rc != BGR_OK) return rc == kCallDone ? BGR_OK : rc;
    return finish_text_call(c);
}
