// text_kernels.h -- launch interface of the text route's kernels (FASTA text in, formatted records out): text_kernels.hip (the streaming kernels: scan,
// parse, record info, write, format), text_correct.hip (correction mode), text_gaf.hip (GAF lines, path stats); see there.
#ifndef BGREAT_AMD_TEXT_KERNELS_H
#define BGREAT_AMD_TEXT_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "graph_layout.h"

// words of the small device `info` block of a text batch
#define TXT_INFO_N_REC 0      /* record starts found */
#define TXT_INFO_N_ACC 1      /* records accepted (aligner.cpp:78-88) */
#define TXT_INFO_BASES 2      /* bases of the accepted records */
#define TXT_INFO_MAX_LEN 3
#define TXT_INFO_IRREGULAR 4  /* the piece is not of the shape this route takes: the caller parses it on the host */
#define TXT_INFO_PBYTES 5     /* bytes of the paths stream */
#define TXT_INFO_NBYTES 6     /* bytes of the notAligned stream */
#define TXT_INFO_BUG 7        /* correction mode: the first accepted read whose path does not spell a walk ("bug compaction"), else ~0 */
#define TXT_INFO_WORDS 8
#include "text_epochs.h" /* BGR_TEXT_EPOCH_MAX, and the host's book of the epochs */

namespace bgr {

// exclusive scan of two u32 arrays of equal length at once, over their first min(n, *n_dev) entries (n_dev: a count on the device, or null); sums: 2 * scan_tiles(n) words
hipError_t launch_scan2_u32(const uint32_t* inA, const uint32_t* inB, uint32_t* outA, uint32_t* outB, uint32_t n, const uint32_t* n_dev, uint32_t* sums, uint32_t* totalA,
                            uint32_t* totalB, hipStream_t stream);
uint32_t scan_tiles(uint32_t n);
uint32_t text_tiles(uint32_t bytes);     // workgroups (= chain entries) of the parse launch
uint32_t format_tiles(uint32_t n_acc);   // ... of the format launch
// The piece in one launch: info[N_REC, N_ACC, BASES, MAX_LEN, IRREGULAR]; rec[0 .. min(N_REC, rec_cap)); the accepted records compacted in input order: acc_rec (which
// record), acc_src (where its read starts in the text), read_offs (base offsets, N_ACC + 1 of them); acc_idx[j] = a for accepted record j.
// fastq_lines: 0 FASTA, else lines per FASTQ record (4, 2).  Running totals pass between the launch's workgroups through `chains` (3 * text_tiles(n) u64), tagged
// with `epoch` (1 .. BGR_TEXT_EPOCH_MAX, a fresh one per launch; the chains are zero before epoch 1 is used; any other value: hipErrorInvalidValue and no launch -- the
// kernels would wait for ever), the workgroups numbered by *ticket - ticket_base (*ticket grows by text_tiles(n) per launch).  words_a words at zero_a and words_b at zero_b (at most 1024 each) are cleared: words only later launches read.
hipError_t launch_text_parse(const uint8_t* text, uint32_t n, uint32_t fastq_lines, uint32_t k, uint32_t* ticket, uint32_t ticket_base, uint32_t epoch, uint64_t* chains,
                             uint4* rec, uint32_t* acc_idx, uint32_t* acc_rec, uint32_t* acc_src, uint64_t* read_offs, uint32_t* info, uint32_t rec_cap, uint32_t* zero_a,
                             uint32_t words_a, uint32_t* zero_b, uint32_t words_b, hipStream_t stream);
// Sizes, stream offsets and the bytes of the records in one launch: info[PBYTES, NBYTES] (saturating at 2^32 - 1); poff/noff as launch_text_write takes them; the bytes
// where a workgroup's whole stretch ends below pcap / ncap.  chains: 2 * format_tiles(n_acc) u64; ticket / epoch as above.
hipError_t launch_text_format(const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec, const uint32_t* acc_rec, uint32_t n_acc, uint32_t* ticket,
                              uint32_t ticket_base, uint32_t epoch, uint64_t* chains, uint32_t* poff, uint32_t* noff, uint8_t* pout, uint8_t* nout, uint64_t pcap, uint64_t ncap,
                              uint32_t* info, hipStream_t stream);
hipError_t launch_text_write(const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec, const uint32_t* acc_rec, uint32_t n_acc,
                             const uint32_t* poff, const uint32_t* noff, uint8_t* pout, uint8_t* nout, hipStream_t stream);
// one word per record, record order: kept << 31 | mapped << 30 | read length (bgr_text_batch.record_info_out)
hipError_t launch_text_record_info(const uint4* rec, const uint32_t* acc_idx, const uint2* results, uint32_t n_rec, uint32_t* out, hipStream_t stream);
// correction mode (-c): mapped reads are written as header + the read spelled by its path (recoverPath, aligner.cpp:270-290)
hipError_t launch_text_correct_sizes(const BgrDeviceGraph& g, const uint2* results, const int32_t* arena, const uint4* rec, const uint32_t* acc_rec, uint32_t n_acc, uint32_t* psz,
                                     uint32_t* nsz, uint32_t* clen, uint32_t* bug, hipStream_t stream);
hipError_t launch_text_correct_write(const BgrDeviceGraph& g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec, const uint32_t* acc_rec, uint32_t n_acc,
                                     const uint32_t* poff, const uint32_t* noff, const uint32_t* clen, uint8_t* pout, uint8_t* nout, hipStream_t stream);
// GAF output (--gaf, want_output 3): a mapped read's record is one GAF line -- name, query interval, the path's segments with their orientations, path interval,
// matches, NM (text_gaf.hip).  Sizes (psz / nsz, scanned by launch_scan2_u32), then the bytes; nlen (characters of the name), rows ({walk size low, high,
// characters covered, NM} per accepted read) and psz pass from the first to the second.  *bug as launch_text_correct_sizes sets it.
hipError_t launch_text_gaf_sizes(const BgrDeviceGraph& g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec, const uint32_t* acc_rec, uint32_t n_acc,
                                 uint32_t* psz, uint32_t* nsz, uint32_t* nlen, uint4* rows, uint32_t* bug, const uint32_t* tag_table, uint4* tags, uint32_t* csb, hipStream_t stream);
hipError_t launch_text_gaf_write(const BgrDeviceGraph& g, const uint8_t* text, const uint2* results, const int32_t* arena, const uint4* rec, const uint32_t* acc_rec, uint32_t n_acc,
                                 const uint32_t* poff, const uint32_t* noff, const uint32_t* psz, const uint32_t* nlen, const uint4* rows, uint8_t* pout, uint8_t* nout,
                                 const uint4* tags, const uint32_t* csb, hipStream_t stream);   // tag_table / tags (bgr_read_tag per read) null: the untagged kernels; else the tagged instances (haplotag_device.h)
// csb (a word per accepted read: the bytes of its cs:Z: ops) null: the kernels as ever; else the instances whose lines end in that field (gaf_cs_device.h)
// bgr_aligner_path_stats: per read of a bgr_align_device launch six words {walk size low, high, path start low, high, characters covered, NM | 1 << 31 "spells no walk"}
// (zeros for an unmapped read, and for a row that does not lie wholly inside the launch's arena_ints)
hipError_t launch_path_stats(const BgrDeviceGraph& g, const uint8_t* reads, const uint64_t* read_offs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n,
                             uint32_t* out, hipStream_t stream);
// bgr_aligner_path_diffs: cnt[r] = the differences of read r (what path stats reports as NM; 0 for a row it reports zeros or "no walk" for); then, with doff the
// exclusive scan of cnt, the differences themselves at out[doff[r] ...], two words each (bgr_path_diff), ascending read position
hipError_t launch_path_diffs_count(const BgrDeviceGraph& g, const uint8_t* reads, const uint64_t* read_offs, const uint2* results, const int32_t* arena, uint64_t arena_ints, uint32_t n,
                                   uint32_t* cnt, hipStream_t stream);
hipError_t launch_path_diffs_fill(const BgrDeviceGraph& g, const uint8_t* reads, const uint64_t* read_offs, const uint2* results, const int32_t* arena, uint32_t n, const uint32_t* cnt,
                                  const uint32_t* doff, uint2* out, hipStream_t stream);
// the pre-pass (batch_kernels.hip) over reads that lie scattered in a text: read r's characters start at reads + src_off[r]
hipError_t launch_pack_reads_at(const uint8_t* text, const uint32_t* src_off, const uint64_t* read_offs, uint32_t n, uint64_t text_bytes, uint64_t total_bases,
                                uint64_t* fw3, uint64_t* nmw, uint32_t* hasn, hipStream_t stream);

}  // namespace bgr

#endif
